"""The 8-lane float32 kernels return, bit for bit, what they returned before their broadcasts of row pairs
(csrc/atacom_quad.h: qbcast2) became row-wide 64-bit DPP moves: tests/golden/pair_broadcast_identity.npz was recorded on the
commit before that change (profiles/tools/gen_pair_broadcast_identity_golden.py), on the runs of
tests/pair_broadcast_identity_cases.py -- odd batches (a DPP row with one live and one switched-off group), environments
sitting a step out, the policy kernel, the planar T-step kernel."""
import os

import numpy as np
import pytest

import pair_broadcast_identity_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N_ARRAYS = {'step': 6 + 7, 'masked': 6, 'policy': 3, 'rollout': 7}


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'pair_broadcast_identity.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('kind,name', cases.CASES, ids=[cases.case_id(*c) for c in cases.CASES])
def test_eight_lane_kernels_are_bitwise_the_recorded_run(golden, kind, name):
    """Every step's returns (obs, reward, absorbing, last), the final state and the constraint statistics."""
    got = cases.run_case(kind, name)
    cid = cases.case_id(kind, name)
    want = {k: v for k, v in golden.items() if k.startswith(cid + '/')}
    assert sorted(got) == sorted(want)
    assert len(got) == N_ARRAYS[kind]
    for key in sorted(want):
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        # bytes, not values: NaN would compare unequal to itself, -0.0 equal to 0.0
        assert a.numel() > 0 and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
            '%s: %d of %d elements differ' % (key, int((a != b).sum()), a.numel())
    if kind == 'step':
        assert got[cid + '/last'][cases.HORIZON - 1].all()          # the horizon's reset was crossed
    if kind == 'masked':
        out = np.arange(cases.BATCH[name]) % 3 == 0                 # the environments that sat out did nothing
        assert not got[cid + '/reward'][:, out].any() and not got[cid + '/last'][:, out].any()
        assert got[cid + '/last'][cases.HORIZON - 1][~out].all()
