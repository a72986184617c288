"""Record tests/golden/offgrad_identity.npz and tests/golden/soft_identity.npz (GPU): what critic_gradient and actor_gradient of
libatacom_offgrad.so, and soft_td_target, soft_critic_gradient and soft_actor_gradient of libatacom_soft.so, return on the runs
of tests/offpolicy_backward_identity_cases.py, in float32 and float64.  Run on the build whose results are to be held fixed --
ATACOM_OFFGRAD_LIB and ATACOM_SOFT_LIB select it:

    ATACOM_OFFGRAD_LIB=<parent build>/libatacom_offgrad.so ATACOM_SOFT_LIB=<parent build>/libatacom_soft.so \
        python profiles/tools/gen_offpolicy_backward_identity_golden.py [output directory]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import offpolicy_backward_identity_cases as cases  # noqa: E402

where = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden')
for lib, todo, run in (('offgrad', cases.OFFGRAD_CASES, cases.run_offgrad), ('soft', cases.SOFT_CASES, cases.run_soft)):
    out = {}
    for dt in cases.DTYPES:
        for case in todo:
            out.update(run(case, dt))
    assert all(np.isfinite(v).all() for v in out.values())
    path = os.path.join(where, lib + '_identity.npz')
    np.savez_compressed(path, **out)
    print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
