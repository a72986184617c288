"""The lane-group kernels return, bit for bit, what they returned before their butterfly sums (csrc/atacom_quad.h) were
handed from hand-written DPP blocks to the compiler: tests/golden/lane_group_identity.npz was recorded on the commit before
that change (profiles/tools/gen_lane_group_identity_golden.py), on the runs of tests/lane_group_identity_cases.py."""
import os

import numpy as np
import pytest

import lane_group_identity_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'lane_group_identity.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('name,dt,lanes,with_rollout', cases.CASES, ids=[cases.case_id(*c[:3]) for c in cases.CASES])
def test_lane_group_kernels_are_bitwise_the_recorded_run(golden, name, dt, lanes, with_rollout):
    """atacom_step at steps 1, 2, 119, 120, 121 and 130 (obs, reward, absorbing, last), the final state and the constraint
    statistics; for the 8-lane float32 mapping the same through the T-step kernel."""
    got = cases.run_case(name, dt, lanes, with_rollout)
    want = {k: v for k, v in golden.items() if k.startswith(cases.case_id(name, dt, lanes) + '/')}
    assert sorted(got) == sorted(want)
    assert len(got) == (4 * len(cases.CHECK) + 2) + (7 if with_rollout else 0)
    for key in sorted(want):
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert torch.equal(a, b), '%s: %d of %d elements differ' % (key, int((a != b).sum()), a.numel())
    assert got[cases.case_id(name, dt, lanes) + '/step%d/last' % cases.HORIZON].all()     # the horizon's reset was crossed
