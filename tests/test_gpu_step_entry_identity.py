"""The single-step kernels return, bit for bit, what they returned before k_step began to request its kernel arguments in
one batch in front of the bounds check (csrc/atacom_kernels.h: kernarg_request_lines; profiles/step_entry.md):
tests/golden/step_entry_identity.npz was recorded on the commit before that change
(profiles/tools/gen_step_entry_identity_golden.py), on the runs of tests/step_entry_identity_cases.py -- batches that leave
lanes and whole lane groups of the last wave behind the bounds check, in all three environments and in float64, through
step() and through step(mask=...) with nobody, everybody and every other environment taking part."""
import os

import numpy as np
import pytest

import step_entry_identity_cases as cases
from conftest import GOLDEN

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(GOLDEN, 'step_entry_identity.npz')) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('case', cases.CASES, ids=cases.case_id)
def test_entry_of_the_step_kernel_gives_the_recorded_bits(golden, case):
    """Every step's returns (obs, reward, absorbing, last), the final state and the constraint statistics."""
    got = cases.run_case(case)
    name, _, batch, _, mask_kind = case
    cfg, row = cases.config_id(case), cases.MASKS.index(mask_kind)
    want = {k[len(cfg) + 1:]: v[row] for k, v in golden.items() if k.startswith(cfg + '/')}
    assert sorted(got) == sorted(want)
    assert len(got) == len(cases.FIELDS) + 2
    for key in sorted(want):
        a, b = torch.from_numpy(got[key]), torch.from_numpy(want[key])
        assert a.dtype == b.dtype and a.shape == b.shape, key
        # bytes, not values: NaN would compare unequal to itself, -0.0 equal to 0.0
        assert a.numel() > 0 and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), \
            '%s: %d of %d elements differ' % (key, int((a != b).sum()), a.numel())
    assert got['obs'].shape[:2] == (cases.T, batch)
    # what the masks are for: an environment that sits a call out reports reward 0, absorbing 0, last 0 and keeps its state
    m = cases.mask_of(mask_kind, batch)
    unmasked = {k[len(cfg) + 1:]: v[cases.MASKS.index('none')] for k, v in golden.items() if k.startswith(cfg + '/')}
    if m is not None and not m.all():
        out = ~m
        assert not got['reward'][:, out].any() and not got['absorbing'][:, out].any() and not got['last'][:, out].any()
        assert not np.array_equal(unmasked['state'][out], got['state'][out])      # the same environments did move when they took part
    if mask_kind == 'ones':                  # everybody takes part: the bits of the unmasked kernel path
        for key in sorted(want):
            assert unmasked[key].tobytes() == got[key].tobytes(), key
