"""Kernel-by-kernel comparison of two builds of libatacom_hip.so (registers, scratch, LDS, code size), read from the code
objects inside the libraries -- no GPU needed.  The A/B evidence behind "option X costs nothing while it is off".

    python profiles/tools/kernel_table_diff.py build/ab/libatacom_nonoise.so rl_on_manifold_amd/libatacom_hip.so [filter] [--code]

--code also compares each kernel's instruction bytes (its symbol's slice of the code object's .text) and the host .text of
the two libraries: "the same machine code", the standard a refactor of the kernel sources can be held to.
"""
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from test_kernel_resources import LLVM, _kernels      # noqa: E402


def _readelf(flag, elf):
    return subprocess.run([os.path.join(LLVM, 'llvm-readelf'), flag, elf], capture_output=True, text=True, check=True).stdout


def _text(elf):
    """(address, bytes) of the ELF file's .text section"""
    m = re.search(r'\s\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)', _readelf('-SW', elf))
    addr, off, size = (int(x, 16) for x in m.groups())
    with open(elf, 'rb') as fh:
        fh.seek(off)
        return addr, fh.read(size)


def _code(tmp):
    """{kernel name as _kernels reports it: the sha256 of its instruction bytes (one per distinct copy)}, from the device
    code objects _kernels(tmp, ...) extracted into tmp (dev<offset>.elf)"""
    funcs = []
    for elf in sorted(glob.glob(os.path.join(tmp, 'dev*.elf'))):
        addr, text = _text(elf)
        for ln in _readelf('-sW', elf).split('\n'):
            if ' FUNC ' in ln:
                f = ln.split()
                start = int(f[1], 16) - addr
                funcs.append((f[-1], hashlib.sha256(text[start:start + int(f[2])]).hexdigest()[:16]))
    names = subprocess.run(['c++filt'] + [n for n, _ in funcs], capture_output=True, text=True).stdout.strip().split('\n')
    out = {}
    for n, (_, h) in zip(names, funcs):
        out.setdefault(re.sub(r'\(.*', '', n).replace('atacom::', '').replace('void ', ''), []).append(h)
    return {k: tuple(sorted(set(v))) for k, v in out.items()}      # (readelf -s lists .dynsym and .symtab)


args = [x for x in sys.argv[1:] if x != '--code']
code = '--code' in sys.argv
a, b = args[0], args[1]
flt = args[2] if len(args) > 2 else ''
with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
    A = {k[0]: k[1:] for k in _kernels(t1, a)}
    B = {k[0]: k[1:] for k in _kernels(t2, b)}
    if code:
        CA, CB = _code(t1), _code(t2)
        A = {k: v + (CA.get(k),) for k, v in A.items()}
        B = {k: v + (CB.get(k),) for k, v in B.items()}
same = diff = 0
print('%-62s %-28s %-28s' % ('kernel', os.path.basename(a), os.path.basename(b)))
print('%-62s %-28s %-28s' % ('', 'LDS scratch VGPR AGPR code', 'LDS scratch VGPR AGPR code'))
for name in sorted(set(A) | set(B)):
    if flt not in name:
        continue
    ra, rb = A.get(name), B.get(name)
    if ra == rb:
        same += 1
        continue
    diff += 1
    f = lambda r: '-' if r is None else '%3d %5d %4d %4d %6d' % r[:5]      # noqa: E731
    insn = '  (instruction bytes differ)' if ra and rb and ra[:5] == rb[:5] else ''
    print('%-62s %-28s %-28s%s' % (name[:62], f(ra), f(rb), insn))
both = sum(1 for k in set(A) & set(B) if flt in k)
print('%d kernels in both builds, %d in one only' % (both, same + diff - both))
print('%d kernels identical in every column%s, %d differ' % (same, ' and in their instruction bytes' if code else '', diff))
if code:
    print('host .text: %s' % ('identical' if _text(a)[1] == _text(b)[1] else 'DIFFERS'))
