"""libatacom_offgrad.so and libatacom_soft.so return, bit for bit, what they returned while each carried its own copy of the
backward pass, the row access, the float64 column pairs and the slice sum of the reduction, before those gave way to
csrc/mlp/atacom_mlp_backward.h: tests/golden/offgrad_identity.npz and tests/golden/soft_identity.npz were recorded on the commit
before that change (profiles/tools/gen_offpolicy_backward_identity_golden.py), on the runs of
tests/offpolicy_backward_identity_cases.py.  No tolerance anywhere: a bit that moves is an addition re-ordered, a hand-over slot
out of place or a contraction changed."""
import os

import numpy as np
import pytest

import offpolicy_backward_identity_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


def _load(name):
    with np.load(os.path.join(GOLDEN, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def offgrad_golden():
    return _load('offgrad_identity.npz')


@pytest.fixture(scope='module')
def soft_golden():
    return _load('soft_identity.npz')


def _same_bytes(got, golden, lib, case, dt):
    prefix = '%s/%s/' % (cases.case_id(lib, case), dt)
    want = {k: v for k, v in golden.items() if k.startswith(prefix)}
    assert sorted(got) == sorted(want) == sorted(prefix + f for f in cases.fields(lib, case))
    for key in sorted(want):
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        # bytes, not values: NaN would compare unequal to itself, -0.0 equal to 0.0
        assert a.numel() > 0 and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
            '%s: %d of %d elements differ' % (key, int((a != b).sum()), a.numel())
        assert np.isfinite(got[key]).all(), key
    return prefix


@pytest.mark.parametrize('dt', cases.DTYPES)
@pytest.mark.parametrize('case', cases.OFFGRAD_CASES, ids=str)
def test_ddpg_and_td3_gradients_give_the_recorded_bits(offgrad_golden, case, dt):
    """grad and stats of every critic of critic_gradient; grad, stats, action_out and dqda_out of actor_gradient."""
    got = cases.run_offgrad(case, dt)
    p = _same_bytes(got, offgrad_golden, 'offgrad', case, dt)
    assert got[p + 'critic0/flat'].any() and got[p + 'actor/flat'].any()
    if case[-2]:
        assert not np.array_equal(got[p + 'critic0/flat'], got[p + 'critic1/flat'])


@pytest.mark.parametrize('dt', cases.DTYPES)
@pytest.mark.parametrize('case', cases.SOFT_CASES, ids=str)
def test_sac_target_and_gradients_give_the_recorded_bits(soft_golden, case, dt):
    """y, action and logp of soft_td_target; grad and stats of every critic of soft_critic_gradient; the gradients of mu and of
    sigma, stats, action, logp, q and dq/da of soft_actor_gradient.  Two cases leave soft_critic_gradient out: the cases module
    says why."""
    got = cases.run_soft(case, dt)
    p = _same_bytes(got, soft_golden, 'soft', case, dt)
    assert got[p + 'actor/mu'].any() and got[p + 'actor/sigma'].any() and (not case[-2] or got[p + 'critic0/flat'].any())
    if case[-2] == 2:
        assert not np.array_equal(got[p + 'critic0/flat'], got[p + 'critic1/flat'])


def test_the_goldens_hold_nothing_else(offgrad_golden, soft_golden):
    for lib, golden, todo in (('offgrad', offgrad_golden, cases.OFFGRAD_CASES), ('soft', soft_golden, cases.SOFT_CASES)):
        want = ['%s/%s/%s' % (cases.case_id(lib, case), dt, f) for dt in cases.DTYPES for case in todo for f in cases.fields(lib, case)]
        assert sorted(golden) == sorted(want)
