"""Record tests/golden/step_params_identity.npz (GPU): the returns of the 8-lane float32 iiwa kernels on the seeded runs of
tests/step_params_identity_cases.py.  Run on the build whose results are to be held fixed -- ATACOM_LIB selects it:

    ATACOM_LIB=<parent build>/libatacom_hip.so python profiles/tools/gen_step_params_identity_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import step_params_identity_cases as cases  # noqa: E402

out = {}
for kind in cases.CASES:
    out.update(cases.run_case(kind))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'step_params_identity.npz')
np.savez_compressed(path, **out)
print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
