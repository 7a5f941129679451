"""Capture tests/golden/convex_hull_I_car.npz: the per-step hull vertex list the reference's post-processing produces from the
tube of agent_e2e_I_car.npz.

Reference benchmarking/generate_convex_hull.py:87-100 (the ``[:200]`` slice, harmless at 8 samples, and the
``scipy.spatial.ConvexHull`` loop over the steps 1..H) is executed from the reference's source at capture time, the way
make_goldens.py executes lines 76-83 of the same file; nothing of it is copied here.  The fixture holds arrays only: the input
tube and one ``(n_v, 2)`` vertex array per step.

    python tests/golden/make_hull_golden.py [reference checkout]     (default: where make_goldens.py looks; needs scipy)
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else re.search(r'^REF = "(.*)"', open(f"{HERE}/make_goldens.py").read(), re.M).group(1)


def main():
    X_traj = np.load(f"{HERE}/agent_e2e_I_car.npz")["X_traj"]
    src = open(f"{REF}/benchmarking/generate_convex_hull.py").read().split("\n")
    code = "\n".join(src[86:100])
    assert "X_traj[:200" in code and "ConvexHull(pts_i)" in code and "hull_points.append" in code, "reference lines moved"
    assert "pickle" not in code and "open(" not in code
    ns = {"np": np, "X_traj": X_traj.copy()}
    exec(code, ns)
    hulls = ns["hull_points"]
    assert len(hulls) == X_traj.shape[2] - 1
    out = {"X_traj": X_traj, "n_steps": np.int64(len(hulls))}
    for i, h in enumerate(hulls):
        out[f"hull_{i}"] = np.asarray(h, dtype=np.float64)
    np.savez(f"{HERE}/convex_hull_I_car.npz", **out)
    print("convex_hull_I_car.npz written:", [len(h) for h in hulls], "vertices at steps 1..%d" % len(hulls))


if __name__ == "__main__":
    main()
