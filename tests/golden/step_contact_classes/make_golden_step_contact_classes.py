"""Record tests/golden/step_contact_classes/step_contact_classes.npz: what the fused step kernel of the CURRENT build
computes over the four control steps of tests/test_gpu_step_contact_classes.py, for a later build to reproduce bit
for bit.

Test infrastructure only.  Needs the GPU and the built step library; run it on the commit whose results are to be
kept (the parent of a change that must not move a bit), then commit the file with the change.

Usage: python tests/golden/step_contact_classes/make_golden_step_contact_classes.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from tests import test_gpu_step_contact_classes as K  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else K.FIXTURE
    data = K.replay()
    counts = K.class_counts(np.stack([data[f"s{t}/contact_forces"] for t in range(K.STEPS)]))
    print(counts)
    assert K.holds_every_class(counts), counts
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"{out}: {len(data)} arrays, {os.path.getsize(out)} bytes")
