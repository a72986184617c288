"""Record tests/golden/step_entry_identity.npz (GPU): the returns of the single-step kernels on the seeded runs of
tests/step_entry_identity_cases.py.  Run on the build whose results are to be held fixed -- ATACOM_LIB selects it:

    ATACOM_LIB=<parent build>/libatacom_hip.so python profiles/tools/gen_step_entry_identity_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import step_entry_identity_cases as cases  # noqa: E402

out = {}
for cfg in cases.CONFIGS:                # one array per configuration and field, the runs of cases.MASKS stacked
    runs = [cases.run_case(cfg + (m,)) for m in cases.MASKS]
    for field in runs[0]:
        out['%s/%s' % (cases.config_id(cfg), field)] = np.stack([r[field] for r in runs])
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'step_entry_identity.npz')
np.savez_compressed(path, **out)
print('%s: %d arrays, %d bytes' % (path, len(out), os.path.getsize(path)))
