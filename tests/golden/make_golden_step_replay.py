"""Record tests/golden/step_replay/step_replay.npz: what the fused step kernel of the CURRENT build computes over the
six control steps of tests/test_gpu_step_replay.py (both variants), for a later build to reproduce bit for bit.

Test infrastructure only.  Needs the GPU and the built step library; run it on the commit whose results are to be
kept (the parent of a change that must not move a bit), then commit the file with the change.

Usage: python tests/golden/make_golden_step_replay.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_gpu_step_replay as R  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else R.FIXTURE
    data = {}
    for v in R.VARIANTS:
        data.update(R.replay(v))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"{out}: {len(data)} arrays, {os.path.getsize(out)} bytes")
