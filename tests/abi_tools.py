"""What the CPU-only checks of the libraries' C ABIs share (tests/test_*_abi.py, tests/test_build_table.py): read a header's
declarations and a library's exports, compile a C11 consumer, list a library's kernels, run the exec-mask audit, fake
modification times for build.stale().  A helper module: it holds no test."""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_kernel_resources import LLVM, _kernels        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')


def needs_llvm(tool):
    return pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, tool)), reason='needs the ROCm LLVM binutils')


def declared_functions(header, prefix):
    """The sorted names starting with `prefix` that include/<header> declares as functions."""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(%s[a-z_]+)\s*\(' % prefix, src)))


def compile_c11(tmp_path, include_dir, text):
    """`text` compiles as strict C11 against the headers of `include_dir`."""
    src = tmp_path / 'use.c'
    src.write_text(text)
    subprocess.check_call(['gcc', '-std=c11', '-pedantic', '-Wall', '-Werror', '-I', include_dir, '-c', str(src),
                           '-o', str(tmp_path / 'use.o')])


def exported_symbols(so):
    """The sorted atacom_* symbols that the library defines and exports."""
    nm = os.path.join(LLVM, 'llvm-nm')
    out = subprocess.run([nm if os.path.exists(nm) else 'nm', '-D', '--defined-only', so], capture_output=True, text=True,
                         check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith('atacom_'))


def one_symbol_set(so, header, prefix, binding):
    """Declared in the header, exported by the library and bound by the ctypes module: one set of names, which is returned."""
    names = declared_functions(header, prefix)
    exported = exported_symbols(so)
    assert exported == names, exported
    assert sorted(binding.EXPORTS) == names
    return names


def kernel_rows(so, tmp):
    """test_kernel_resources._kernels of `so`, sorted, the libraries' own namespaces dropped from the names.  The code objects
    stay in `tmp` as dev<offset>.elf."""
    return sorted((re.sub(r'\batacom_\w+::', '', k[0]),) + k[1:] for k in _kernels(str(tmp), so=so))


def function_bodies(so, tmp):
    """[(code object, first line, disassembly)] of every function in the library's gfx950 code objects."""
    kernel_rows(so, tmp)
    out = []
    for elf in sorted(f for f in os.listdir(str(tmp)) if f.startswith('dev') and f.endswith('.elf')):
        asm = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--demangle', os.path.join(str(tmp), elf)],
                             capture_output=True, text=True, check=True).stdout
        out += [(elf, body.split('\n', 1)[0], body) for body in re.split(r'\n(?=[0-9a-f]+ <)', asm)]
    return out


def exec_audit(so):
    """profiles/tools/exec_restore_audit.py finds no register copy under a narrowed exec mask."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'profiles', 'tools', 'exec_restore_audit.py'), '--so', so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 copies' in r.stdout, r.stdout


def fake_mlp(**kw):
    """An atacom_mlp that passes every check of the policy validator, with `kw` applied: for calls that the host refuses."""
    import ctypes
    from rl_on_manifold_amd import _lib
    m = _lib.AtacomMlp()
    m.struct_size = ctypes.sizeof(_lib.AtacomMlp)
    m.n_in, m.hidden, m.n_out = 20, 64, 2
    for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        setattr(m, k, 0x1000)                        # never dereferenced
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def fake_mtimes(monkeypatch, build):
    """Every library of build.TARGETS exists and every file is as old as it, except the files whose base names are in the
    returned list: no source is edited."""
    libs = [t.lib for t in build.TARGETS.values()]
    touched = []
    real_exists = os.path.exists
    monkeypatch.setattr(build.os.path, 'exists', lambda p: p in libs or real_exists(p))
    monkeypatch.setattr(build.os.path, 'getmtime', lambda p: 2.0 if os.path.basename(p) in touched else 1.0)
    return touched
