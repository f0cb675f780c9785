"""Record tests/golden/seg_layout/seg_pair.npz: t and cell of the segments of tests/test_gpu_seg_layout.py, each
searched on its own with the full candidate set by go1dc_terrain (seg_deepest) of the CURRENT build's test-only
library, in modes 0, 1 and 2 -- for a build that lays the sub-step's search out differently to reproduce bit for bit.

Test infrastructure only.  Needs the GPU and the built device-check library; run it on the commit whose results are
to be kept (the parent of a change that must not move a bit; GO1_DEVCHECK_LIB may name that commit's library), then
commit the file with the change.

Usage: python tests/golden/seg_layout/make_golden_seg_layout.py [OUT.npz]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(HERE))))

from tests import test_gpu_seg_layout as L  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else L.FIXTURE
    s = L.scene()
    data = {k: s[k].astype(np.float32) for k in ("A", "B", "r")}
    data["tile"] = s["tile"]
    for m in L.MODES:
        data[f"t{m}"], data[f"cell{m}"] = L.golden_run(m)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **data)
    print(f"{out}: {len(data)} arrays, {os.path.getsize(out)} bytes")
