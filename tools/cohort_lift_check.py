#!/usr/bin/env python
"""Check that a change to the cohort kernels' source is bitwise-neutral: dump ``ops.cohort_effect``'s outputs (out,
sums, wsum) on shapes of tests/test_gpu_cohort_effect.py from one build, then compare a second build against the dump.

    python tools/cohort_lift_check.py --tree PARENT --dump before.npz   # PARENT: a built checkout of the parent commit
    python tools/cohort_lift_check.py --compare before.npz              # on the new tree

``--tree`` names the checkout whose package, library and tests/test_gpu_cohort_effect.py are used (default: the tree
this script lives in), so one copy of the script serves both sides.  The shapes include R = 4096 (the finalize sort
at its cap), R values that are no power of two (17, 65, 513) and several patient chunks.  ``--compare`` prints one
line per array and exits 1 if any differs.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv[1:-1]:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "ode-discovery-for-longitudinal-heterogeneous-treatment-effects-inference_amd"))

# rows of tests/test_gpu_cohort_effect.py's CASES, by index
SHAPES = (2, 4, 7, 8, 9)


def outputs(dev):
    import test_gpu_cohort_effect as TC
    res = {}
    for i in SHAPES:
        Rn, N, T, A, G, name, method, sub, weighting, off = TC.CASES[i]
        y0, u, arm_a, arm_b, coef = TC._inputs(Rn, N, T, A, name, method, sub)
        group = (np.arange(N) % G).astype(np.int32)
        out, sums, wsum = TC._run(dev, name, y0, u, arm_a, arm_b, coef, TC.Q5, method, sub, T, group, G, weighting,
                                  TC.SEED, off)
        key = TC._id(TC.CASES[i])
        res[key + "/out"], res[key + "/sums"], res[key + "/wsum"] = out, sums, wsum
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="the checkout to run (default: this script's)")
    ap.add_argument("--dump")
    ap.add_argument("--compare")
    a = ap.parse_args()
    if bool(a.dump) == bool(a.compare):
        raise SystemExit("one of --dump FILE and --compare FILE")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cohort_lift_check needs the GPU")
    from insite_amd import _lib
    print(f"library: {_lib.LIB_PATH}")
    res = outputs(torch.device("cuda:0"))
    if a.dump:
        os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
        np.savez(a.dump, **res)
        print(f"dumped {len(res)} arrays of {len(SHAPES)} shapes to {a.dump}")
        return
    before = np.load(a.compare)
    bad = 0
    for key in sorted(res):
        x, y = np.ascontiguousarray(before[key]), np.ascontiguousarray(res[key])
        same = x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))
        print(f"{key}: {x.shape} {'bitwise equal' if same else 'DIFFERS'}")
        bad += not same
    print(f"{len(res) - bad} of {len(res)} arrays bitwise equal")
    raise SystemExit(1 if bad else 0)


if __name__ == "__main__":
    main()
