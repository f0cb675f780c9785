"""Record tests/golden/ppo_replay/ppo_replay.json: the layout numbers and the per-call digests that the PPO update
engine of the CURRENT build gives on the cases of tests/test_gpu_ppo_replay.py, for a later build to reproduce bit
for bit.

Test infrastructure only.  Needs the GPU and the built libgo1_ppo.so; run it on the commit whose results are to be
kept (the parent of a change that must not move a bit; GO1_PPO_LIB_OVERRIDE names a library built elsewhere), then
commit the file with the change.

Usage: python tests/golden/make_golden_ppo_replay.py COMMIT [OUT.json]     COMMIT: the 40-digit id of that commit
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from tests import test_gpu_ppo_replay as R  # noqa: E402

if __name__ == "__main__":
    commit = sys.argv[1]
    assert len(commit) == 40 and int(commit, 16) >= 0, "COMMIT: the full id of the commit the library was built from"
    out = sys.argv[2] if len(sys.argv) > 2 else R.FIXTURE
    cases = {}
    for case in R.CASES:
        cases["-".join(case)] = dict(layout=R.layout(case), **R.replay(case))
        print("-".join(case), "recorded", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"recorded_from": commit, "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
                   "cases": cases}, f, indent=1)
        f.write("\n")
    print(f"{out}: {len(cases)} cases, {os.path.getsize(out)} bytes")
