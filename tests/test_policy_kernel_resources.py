"""What the policy kernels occupy after the TD3 / DDPG exploration modes were added to k_rollout_mlp as launch-uniform options
(read from the built library's code objects; no GPU needed).

The modes are run-time options of the existing instantiations: the census stays at 445 kernels.  PARENT holds what every
k_rollout_mlp kernel used before the modes existed -- (scratch bytes per lane, VGPRs = architectural + accumulation
registers, AGPRs), read from the code objects of the build without them.  Most of these kernels sit at the edge of the
register file (512 registers, the accumulation half used as spill space), where any added live value moves spills.  The
modes are written so that they add no value live across the network or the solver (csrc/atacom_kernels.h: the
Ornstein-Uhlenbeck state is advanced before the network, in the registers of the noise, and read from memory every step);
what remains is register-allocation noise of a few registers, bounded here by what was measured when the modes went in:
  * VGPRs and AGPRs: at most 5 more than PARENT (the 8-lane iiwa kernel with held q, the one the 8192-environment collection
    runs: 195 AGPRs against 190 -- spill space; its step time moved by +0.6 to +1.4 % in the same measurement, within the
    noise of one box);
  * scratch: at most 16 bytes per lane more in float32 (two rigid-body kernels: +16; the one-lane iiwa kernel of the
    65536-environment collection went from 176 to 168) and 96 in float64 (the float64 iiwa quad kernel with refreshed q:
    596 -> 676 bytes of spills).
A kernel beyond these bounds has lost registers to a change, and its step time must be measured before it is accepted."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = '/opt/rocm/lib/llvm/bin'

# (scratch bytes per lane, VGPRs, AGPRs) of every k_rollout_mlp kernel before the exploration modes
PARENT = {
    'k_rollout_mlp<double, Iiwa, 1, false, 64, false, 0, false>': (5828, 512, 256),
    'k_rollout_mlp<double, Iiwa, 1, true, 64, false, 0, false>': (5852, 512, 256),
    'k_rollout_mlp<double, Iiwa, 4, false, 64, false, 0, false>': (596, 512, 256),
    'k_rollout_mlp<double, Iiwa, 4, true, 64, false, 0, false>': (640, 512, 256),
    'k_rollout_mlp<double, Planar, 1, false, 64, false, 0, false>': (3484, 512, 256),
    'k_rollout_mlp<double, Planar, 1, true, 64, false, 0, false>': (3540, 512, 256),
    'k_rollout_mlp<double, Planar, 4, false, 64, false, 0, false>': (0, 450, 194),
    'k_rollout_mlp<double, Planar, 4, true, 64, false, 0, false>': (0, 450, 194),
    'k_rollout_mlp<float, Iiwa, 1, false, 64, false, 0, false>': (76, 512, 256),
    'k_rollout_mlp<float, Iiwa, 1, false, 64, false, 0, true>': (124, 512, 256),
    'k_rollout_mlp<float, Iiwa, 1, false, 64, false, 1, false>': (0, 496, 240),
    'k_rollout_mlp<float, Iiwa, 1, false, 64, true, 0, false>': (292, 512, 256),
    'k_rollout_mlp<float, Iiwa, 1, true, 64, false, 0, false>': (176, 512, 256),
    'k_rollout_mlp<float, Iiwa, 1, true, 64, false, 0, true>': (248, 512, 256),
    'k_rollout_mlp<float, Iiwa, 1, true, 64, false, 1, false>': (0, 468, 212),
    'k_rollout_mlp<float, Iiwa, 1, true, 64, true, 0, false>': (416, 512, 256),
    'k_rollout_mlp<float, Iiwa, 2, false, 64, false, 0, false>': (0, 418, 162),
    'k_rollout_mlp<float, Iiwa, 2, false, 64, false, 0, true>': (0, 417, 161),
    'k_rollout_mlp<float, Iiwa, 2, false, 64, false, 1, false>': (0, 512, 256),
    'k_rollout_mlp<float, Iiwa, 2, true, 64, false, 0, false>': (0, 434, 178),
    'k_rollout_mlp<float, Iiwa, 2, true, 64, false, 0, true>': (0, 422, 166),
    'k_rollout_mlp<float, Iiwa, 2, true, 64, false, 1, false>': (0, 512, 256),
    'k_rollout_mlp<float, Iiwa, 4, false, 64, false, 0, false>': (0, 466, 210),
    'k_rollout_mlp<float, Iiwa, 4, false, 64, false, 0, true>': (0, 416, 160),
    'k_rollout_mlp<float, Iiwa, 4, false, 64, false, 1, false>': (0, 492, 236),
    'k_rollout_mlp<float, Iiwa, 4, false, 64, true, 0, false>': (156, 512, 256),
    'k_rollout_mlp<float, Iiwa, 4, true, 64, false, 0, false>': (0, 434, 178),
    'k_rollout_mlp<float, Iiwa, 4, true, 64, false, 0, true>': (0, 398, 142),
    'k_rollout_mlp<float, Iiwa, 4, true, 64, false, 1, false>': (0, 404, 148),
    'k_rollout_mlp<float, Iiwa, 4, true, 64, true, 0, false>': (0, 439, 183),
    'k_rollout_mlp<float, Iiwa, 8, false, 64, false, 0, false>': (0, 435, 179),
    'k_rollout_mlp<float, Iiwa, 8, false, 64, false, 0, true>': (0, 399, 143),
    'k_rollout_mlp<float, Iiwa, 8, false, 64, false, 1, false>': (0, 482, 226),
    'k_rollout_mlp<float, Iiwa, 8, true, 64, false, 0, false>': (0, 446, 190),
    'k_rollout_mlp<float, Iiwa, 8, true, 64, false, 0, true>': (0, 386, 130),
    'k_rollout_mlp<float, Iiwa, 8, true, 64, false, 1, false>': (0, 396, 140),
    'k_rollout_mlp<float, Planar, 1, false, 64, false, 0, false>': (0, 344, 96),
    'k_rollout_mlp<float, Planar, 1, false, 64, false, 0, true>': (0, 352, 96),
    'k_rollout_mlp<float, Planar, 1, false, 64, false, 1, false>': (0, 354, 98),
    'k_rollout_mlp<float, Planar, 1, true, 64, false, 0, false>': (0, 348, 96),
    'k_rollout_mlp<float, Planar, 1, true, 64, false, 0, true>': (0, 352, 96),
    'k_rollout_mlp<float, Planar, 1, true, 64, false, 1, false>': (0, 344, 96),
    'k_rollout_mlp<float, Planar, 2, false, 64, false, 0, false>': (0, 264, 36),
    'k_rollout_mlp<float, Planar, 2, false, 64, false, 0, true>': (0, 268, 36),
    'k_rollout_mlp<float, Planar, 2, false, 64, false, 1, false>': (0, 296, 40),
    'k_rollout_mlp<float, Planar, 2, true, 64, false, 0, false>': (0, 260, 36),
    'k_rollout_mlp<float, Planar, 2, true, 64, false, 0, true>': (0, 264, 36),
    'k_rollout_mlp<float, Planar, 2, true, 64, false, 1, false>': (0, 296, 40),
    'k_rollout_mlp<float, Planar, 4, false, 64, false, 0, false>': (0, 220, 16),
    'k_rollout_mlp<float, Planar, 4, false, 64, false, 0, true>': (0, 228, 16),
    'k_rollout_mlp<float, Planar, 4, false, 64, false, 1, false>': (0, 260, 16),
    'k_rollout_mlp<float, Planar, 4, true, 64, false, 0, false>': (0, 220, 16),
    'k_rollout_mlp<float, Planar, 4, true, 64, false, 0, true>': (0, 228, 16),
    'k_rollout_mlp<float, Planar, 4, true, 64, false, 1, false>': (0, 248, 16),
    'k_rollout_mlp<float, Planar, 8, false, 64, false, 0, false>': (0, 212, 16),
    'k_rollout_mlp<float, Planar, 8, false, 64, false, 0, true>': (0, 224, 16),
    'k_rollout_mlp<float, Planar, 8, false, 64, false, 1, false>': (0, 260, 16),
    'k_rollout_mlp<float, Planar, 8, true, 64, false, 0, false>': (0, 212, 16),
    'k_rollout_mlp<float, Planar, 8, true, 64, false, 0, true>': (0, 228, 16),
    'k_rollout_mlp<float, Planar, 8, true, 64, false, 1, false>': (0, 216, 16),
}


def _kernels(tmp):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from test_kernel_resources import _kernels as read
    return read(tmp)


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')
def test_policy_kernels_keep_their_census_and_resources(tmp_path):
    ks = _kernels(str(tmp_path))
    assert len(ks) == 445, len(ks)                     # no new instantiation: the modes are launch-uniform options
    mlp = {k[0]: (k[2], k[3], k[4]) for k in ks if k[0].startswith('k_rollout_mlp<')}
    assert sorted(mlp) == sorted(PARENT)
    bad = []
    for name, (scratch, vgpr, agpr) in mlp.items():
        s0, v0, a0 = PARENT[name]
        slack = 96 if name.startswith('k_rollout_mlp<double') else 16
        if scratch > s0 + slack or vgpr > v0 + 5 or agpr > a0 + 5:
            bad.append((name, PARENT[name], (scratch, vgpr, agpr)))
    assert not bad, bad
    # the float32 lane-group kernels that ran without scratch still do
    assert not [n for n, r in mlp.items() if r[0] and not PARENT[n][0]]


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='needs the ROCm LLVM binutils')
def test_exec_mask_audit_still_finds_nothing(tmp_path):
    """The OU state is stored by the committing lane of a group: a lane-0-only store region of the kind
    profiles/tools/exec_restore_audit.py audits for register copies under a narrowed exec mask."""
    sys.path.insert(0, os.path.join(ROOT, 'profiles', 'tools'))
    from exec_restore_audit import audit_library
    from rl_on_manifold_amd import build
    found, n_objects = audit_library(build.build(verbose=False), str(tmp_path), LLVM)
    assert n_objects >= 13
    assert not found, [(f[1], [t for _, t in f[4]]) for f in found]
