"""The 8-lane float32 iiwa kernels return, bit for bit, what they returned before the single-step kernel began to read the
parameters of its post-step code from the kernel-argument segment behind the sub-step loop (csrc/atacom_kernels.h:
PARAMS_REREAD): tests/golden/step_params_identity.npz was recorded on the commit before that change
(profiles/tools/gen_step_params_identity_golden.py), on the runs of tests/step_params_identity_cases.py -- in-kernel resets
that re-draw from the seed, a non-zero action penalty, environments sitting a step out, the T-step kernel beside them.  (The
policy kernel and the planar kernels keep the parent's machine code: profiles/step_spill_traffic.md, section 3.)"""
import os

import numpy as np
import pytest

import step_params_identity_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'step_params_identity.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('kind', cases.CASES)
def test_post_step_parameters_give_the_recorded_bits(golden, kind):
    """Every step's returns (obs, reward, absorbing, last), the final state and the constraint statistics."""
    got = cases.run_case(kind)
    cid = cases.case_id(kind)
    want = {k: v for k, v in golden.items() if k.startswith(cid + '/')}
    assert sorted(got) == sorted(want)
    assert len(got) == len(cases.FIELDS) + 2
    for key in sorted(want):
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        # bytes, not values: NaN would compare unequal to itself, -0.0 equal to 0.0
        assert a.numel() > 0 and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
            '%s: %d of %d elements differ' % (key, int((a != b).sum()), a.numel())
    # what the cases are for: resets inside the kernel that drew a new puck, and a penalty in the rewards
    last, obs = got[cid + '/last'], got[cid + '/obs']
    live = np.arange(cases.BATCH) % 3 != 0 if kind == 'masked' else np.ones(cases.BATCH, bool)
    assert last[cases.HORIZON - 1][live].all() and last[2 * cases.HORIZON - 1][live].all()
    # the puck's position in the second and the third episode: drawn per environment and per episode
    ep1, ep2 = obs[cases.HORIZON][live][:, :2], obs[2 * cases.HORIZON][live][:, :2]
    assert len(np.unique(ep1, axis=0)) == live.sum() and not np.array_equal(ep1, ep2)
    if kind == 'masked':
        assert not got[cid + '/reward'][:, ~live].any() and not last[:, ~live].any()
