"""libatacom_fit.so and libatacom_trust.so return, bit for bit, what they returned before the code they share -- the walk over
the rows, the transposition buffers, the backward pass, the hand-over and the slice sum of the reduction -- moved into
csrc/mlp/atacom_mlp_backward.h: tests/golden/mlp_backward_identity.npz was recorded on the commit before that change
(profiles/tools/gen_mlp_backward_identity_golden.py), on the runs of tests/mlp_backward_identity_cases.py.  No tolerance
anywhere: a bit that moves is an addition re-ordered or a contraction changed."""
import os

import numpy as np
import pytest

import mlp_backward_identity_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'mlp_backward_identity.npz')) as z:
        return {k: z[k] for k in z.files}


def _same_bytes(got, golden, cid, dt, fields):
    want = {k: v for k, v in golden.items() if k.startswith('%s/%s/' % (cid, dt))}
    assert sorted(got) == sorted(want) and len(got) == len(fields)
    for key in sorted(want):
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        # bytes, not values: NaN would compare unequal to itself, -0.0 equal to 0.0
        assert a.numel() > 0 and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
            '%s: %d of %d elements differ' % (key, int((a != b).sum()), a.numel())


@pytest.mark.parametrize('dt', cases.DTYPES)
@pytest.mark.parametrize('case', cases.FIT_CASES, ids=str)
def test_gradients_give_the_recorded_bits(golden, case, dt):
    """flat (dW1, db1, dW2, db2, dW3, db3 and, for the policy, d log std) and stats of value_gradient / policy_gradient."""
    got = cases.run_fit(case, dt)
    cid = cases.case_id('fit', case)
    _same_bytes(got, golden, cid, dt, cases.FIT_FIELDS)
    flat, stats = got['%s/%s/flat' % (cid, dt)], got['%s/%s/stats' % (cid, dt)]
    assert np.isfinite(flat).all() and flat.any() and np.isfinite(stats).all()
    if case[0] == 'ppo' and case[1] > 1:                  # what the wobble of logp_old is for: rows on both sides of the clip
        assert 0.0 < stats[1] < 1.0


@pytest.mark.parametrize('dt', cases.DTYPES)
@pytest.mark.parametrize('case', cases.TRUST_CASES, ids=str)
def test_products_give_the_recorded_bits(golden, case, dt):
    """F v + damping v of fisher_vector_product, the log-std block included."""
    got = cases.run_trust(case, dt)
    cid = cases.case_id('trust', case)
    _same_bytes(got, golden, cid, dt, cases.TRUST_FIELDS)
    out = got['%s/%s/product' % (cid, dt)]
    assert np.isfinite(out).all() and out.any()


def test_the_golden_holds_nothing_else(golden):
    n = len(cases.DTYPES) * (len(cases.FIT_CASES) * len(cases.FIT_FIELDS) + len(cases.TRUST_CASES) * len(cases.TRUST_FIELDS))
    assert len(golden) == n
