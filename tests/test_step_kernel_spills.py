"""The 8-lane float32 iiwa step kernel carries nothing across its sub-step loop in the lanes of a vector register.

Params is a by-value kernel argument of about 100 dwords; loaded whole at kernel entry, the constants that are first read
behind the loop (puck, reward, observation) did not fit into the scalar registers next to the solver and were spilled into
lanes of a vector register: 38 v_writelane and 86 v_readlane in `k_step<float, Iiwa, 8, true, false, 0, false>`.  The kernel
now reads them again from the kernel-argument segment behind the loop (csrc/atacom_kernels.h: PARAMS_REREAD;
profiles/step_spill_traffic.md).  Read from the code objects inside the built libatacom_hip.so, no GPU needed.

The kernels the change reaches are listed in CHANGED: the single-step kernel alone.  The T-step kernels of the family
(`k_rollout`, `k_rollout_mlp`) keep the parent's text -- with the same treatment they still spill (110 and 160 scalar
registers, 20 and 18 vector registers: their step loop holds the kernel's pointers and the solver's copies across everything),
which is what this test would refuse."""
import os
import re
import struct
import subprocess

import pytest

LLVM = '/opt/rocm/lib/llvm/bin'
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
CHANGED = ['k_step<float, Iiwa, 8, true, false, 0, false>']

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')


def _short(mangled):
    names = subprocess.run(['c++filt'] + mangled, capture_output=True, text=True).stdout.strip().split('\n')
    return [re.sub(r'\(.*', '', n).replace('atacom::', '').replace('void ', '') for n in names]


@pytest.fixture(scope='module')
def code_objects(tmp_path_factory):
    """[(path of a gfx950 code object of the library, its metadata notes)]"""
    from rl_on_manifold_amd import build
    so = build.build(verbose=False)
    tmp = str(tmp_path_factory.mktemp('spills'))
    fat = os.path.join(tmp, 'fat.bin')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '--dump-section', '.hip_fatbin=' + fat, so,
                           os.path.join(tmp, 'copy.so')])
    data = open(fat, 'rb').read()
    out = []
    for m in re.finditer(MAGIC, data):                       # one bundle per translation unit
        p = m.start()
        n_entries = struct.unpack_from('<Q', data, p + 24)[0]
        off = p + 32
        for _ in range(n_entries):
            o, size, id_len = struct.unpack_from('<QQQ', data, off)
            ident = data[off + 24:off + 24 + id_len].decode()
            off += 24 + id_len
            if 'gfx950' not in ident or size == 0:
                continue
            elf = os.path.join(tmp, 'dev%d.elf' % p)
            open(elf, 'wb').write(data[p + o:p + o + size])
            out.append((elf, subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', elf], capture_output=True,
                                            text=True, check=True).stdout))
    return out


def _metadata(code_objects):
    """{kernel: (code object, mangled name, sgpr spills, vgpr spills, scratch bytes per lane)}"""
    rows = []
    for elf, notes in code_objects:
        for blk in notes.split('  - .agpr_count:')[1:]:
            g = lambda k: re.search(r'\.' + k + r':\s+(\S+)', blk).group(1)      # noqa: E731
            rows.append((elf, g('name'), int(g('sgpr_spill_count')), int(g('vgpr_spill_count')),
                         int(g('private_segment_fixed_size'))))
    return dict(zip(_short([r[1] for r in rows]), rows))


@pytest.mark.parametrize('kernel', CHANGED)
def test_no_register_spills_and_no_private_segment(code_objects, kernel):
    md = _metadata(code_objects)
    assert kernel in md, sorted(k for k in md if k.startswith('k_step<float, Iiwa, 8'))
    _, _, sgpr_spills, vgpr_spills, scratch = md[kernel]
    print('%s: sgpr_spill_count %d, vgpr_spill_count %d, private segment %d bytes' % (kernel, sgpr_spills, vgpr_spills, scratch))
    assert sgpr_spills == 0
    assert vgpr_spills == 0
    assert scratch == 0


@pytest.mark.parametrize('kernel', CHANGED)
def test_no_scalar_value_travels_in_the_lanes_of_a_vector_register(code_objects, kernel):
    elf, mangled = _metadata(code_objects)[kernel][:2]
    dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--disassemble-symbols=' + mangled, elf],
                         capture_output=True, text=True, check=True).stdout
    assert dis.count('s_endpgm') >= 1 and len(re.findall(r'^\s+v_', dis, re.M)) > 4000        # the kernel was disassembled
    lane_moves = re.findall(r'^\s+(v_readlane_b32|v_writelane_b32)\b', dis, re.M)
    assert not lane_moves, '%d v_writelane, %d v_readlane' % (lane_moves.count('v_writelane_b32'), lane_moves.count('v_readlane_b32'))
