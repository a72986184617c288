"""Record tests/golden/mlp_backward_identity.npz (GPU): what value_gradient, policy_gradient and fisher_vector_product return on
the seeded runs of tests/mlp_backward_identity_cases.py, in float32 and float64.  Run on the build whose results are to be held
fixed -- ATACOM_FIT_LIB and ATACOM_TRUST_LIB select it:

    ATACOM_FIT_LIB=<parent build>/libatacom_fit.so ATACOM_TRUST_LIB=<parent build>/libatacom_trust.so \
        python profiles/tools/gen_mlp_backward_identity_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import mlp_backward_identity_cases as cases  # noqa: E402

out = {}
for dt in cases.DTYPES:
    for case in cases.FIT_CASES:
        out.update(cases.run_fit(case, dt))
    for case in cases.TRUST_CASES:
        out.update(cases.run_trust(case, dt))
assert all(np.isfinite(v).all() for v in out.values())
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'mlp_backward_identity.npz')
np.savez_compressed(path, **out)
print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
