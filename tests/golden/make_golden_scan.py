"""Record the reference's step at two height-scan grids other than the README's 21 x 11
(tests/golden/scan_fine.npz, scan_tiny.npz).

Test infrastructure only: make_golden.run, unchanged, with Cfg.terrain.measured_points_x / _y and
Cfg.env.num_observations overridden after train.py; _init_height_points (:1902-1916), _get_heights
(:1918-1965) and the height block of compute_observations (:388-423) are shape-generic.  The names do not
start with step_: the oracle the step_* fixtures replay through is fixed at 21 x 11.

  scan_fine  31 x 15, front half (rows 16 .. 30): 41 + 2 * 15 * 15 = 491 columns
  scan_tiny  5 x 3, full scan, uneven spacing, points beyond the 2 m wide tile (the index clip runs),
             fewer points per layer than the 16 lanes of an env: 41 + 2 * 15 = 71 columns

Usage: python tests/golden/make_golden_scan.py [--which scan_fine|scan_tiny|all]
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402

# name -> (measured_points_x, measured_points_y, measure_front_half); plain float lists: the overrides go
# into the fixture as JSON
CASES = {
    "scan_fine": (np.linspace(-1, 1, 31).tolist(), np.linspace(-0.5, 0.5, 15).tolist(), True),
    "scan_tiny": ([-0.3, 0.0, 0.25, 0.6, 2.5], [-1.5, 0.0, 0.2], False),
}


def width(x, y, front_half):
    rows = len(x) - (len(x) // 2 + 1) if front_half else len(x)
    return 41 + 2 * rows * len(y)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--which", default="all")
    a = ap.parse_args()
    if a.which == "all":
        # one fresh process per fixture: the reference mutates its module-level Cfg
        for w in CASES:
            subprocess.run([sys.executable, __file__, "--which", w], check=True)
    else:
        sys.path.insert(0, HERE)
        import make_golden
        x, y, fh = CASES[a.which]
        make_golden.run("single_path", 32, 4, 3, 21, os.path.join(HERE, a.which + ".npz"), counter_start=398,
                        events=True,
                        cfg_overrides={"terrain.measured_points_x": x, "terrain.measured_points_y": y,
                                       "env.num_observations": width(x, y, fh)},
                        front_half=fh)
