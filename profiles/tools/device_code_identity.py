"""Is the device code of two builds of the package's libraries the same, function by function?  No GPU needed.

    python profiles/tools/device_code_identity.py DIR_A DIR_B [LIB ...]     (each holding the lib*.so of a build; default: LIBS)

For every library, every gfx950 code object inside .hip_fatbin is extracted (as tests/test_kernel_resources.py does) and
each FUNC symbol's slice of its .text is hashed.  Compared per mangled symbol: the same set of symbols, and identical
bytes of each.  Prints a markdown summary (profiles/host_scaffolding_identity.md is one); exit status 1 if anything differs.
The standard a change of host code alone is held to: speed and numerics of the kernels cannot have moved.
"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from rl_on_manifold_amd import build                  # noqa: E402
from test_kernel_resources import LLVM, _kernels      # noqa: E402

LIBS = tuple(build.naming(name).file for name in build.TARGETS)      # every library of the table, by the name build.py gives it


def _readelf(flag, elf):
    return subprocess.run([os.path.join(LLVM, 'llvm-readelf'), flag, elf], capture_output=True, text=True, check=True).stdout


def functions(so):
    """(number of kernels, {mangled FUNC symbol: sorted hashes of its instruction bytes, one per distinct copy})"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        n_kernels = len(_kernels(tmp, so))                   # leaves the code objects in tmp as dev<offset>.elf
        for elf in sorted(glob.glob(os.path.join(tmp, 'dev*.elf'))):
            m = re.search(r'\s\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', _readelf('-SW', elf))
            addr, off, size = (int(x, 16) for x in m.groups())
            with open(elf, 'rb') as fh:
                fh.seek(off)
                text = fh.read(size)
            for ln in _readelf('-sW', elf).split('\n'):
                if ' FUNC ' in ln:
                    f = ln.split()
                    start = int(f[1], 16) - addr
                    out.setdefault(f[-1], set()).add(hashlib.sha256(text[start:start + int(f[2])]).hexdigest())
    return n_kernels, {k: sorted(v) for k, v in out.items()}


def main(dir_a, dir_b, libs=LIBS):
    print('| library | kernels A / B | function symbols A / B | in one build only | compared | differing |')
    print('|---|---|---|---|---|---|')
    bad, detail = 0, []
    for lib in libs:
        (ka, A), (kb, B) = functions(os.path.join(dir_a, lib)), functions(os.path.join(dir_b, lib))
        only = sorted(set(A) ^ set(B))
        differing = sorted(k for k in set(A) & set(B) if A[k] != B[k])
        print('| `%s` | %d / %d | %d / %d | %d | %d | %d |' % (lib, ka, kb, len(A), len(B), len(only), len(set(A) & set(B)),
                                                          len(differing)))
        detail += ['- `%s` %s: `%s`' % (lib, 'in one build only' if k in only else 'bytes differ', k) for k in only + differing]
        bad += len(only) + len(differing) + (ka != kb)
    print('\n'.join([''] + detail) if detail else '\nEvery function of every code object is byte-identical.')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2], tuple(sys.argv[3:]) or LIBS))
