#!/usr/bin/env python3
"""Writes tests/golden/rollout_one_parent_xtraj.npz: X_traj of rollout_one_kernel (pendulum1D, mode R, Ns = 8, the LEAN
instantiation) for H = 12, 17 and 30, feedback on and off, as computed by the commit BEFORE the diagonal-tile inverse moved
into the next step's solve statement.  tests/test_hip_rollout_one_inverse.py compares the current kernel with it bit by bit
and takes its inputs from `inputs()` / `launch()` below, so both see the same seeded data.

    python tests/golden/make_rollout_one_parent_xtraj.py        (on the MI355X, with the parent commit's library built)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "rollout_one_parent_xtraj.npz")
PNAME = "params_pendulum1D_samples"
NS, H_MAX = 8, 30
GOLDEN_H = (12, 17, 30)


def inputs(sg, feedback):
    """(agent, base samples step-major for H_MAX steps, per-sample start states): one agent and one slab serve every H"""
    from sampling_gpmpc_amd.workloads import fs_params
    p = fs_params(PNAME, NS, H_MAX, nograd=False, feedback=feedback)
    p["common"]["use_cuda"] = True
    p["agent"]["base_sample_generator"] = "counter"
    agent = sg.Agent(p, sg.make_env(p))
    g = torch.Generator().manual_seed(77100 + NS)
    z = torch.randn(H_MAX, NS * 3, generator=g, dtype=torch.float64).clamp(-2.5, 2.5).to(agent.torch_device)
    x0 = torch.tensor(p["env"]["start"][:2], dtype=torch.float64) + 0.3 * torch.randn(NS, 2, generator=g, dtype=torch.float64)
    return agent, z, x0.to(agent.torch_device)


def launch(case, H, feedback, kernel, outputs=False):
    """one pinned launch; returns (X_traj, Y or None, info) as numpy arrays and asserts the path the launch took"""
    from sampling_gpmpc_amd import _lib
    from sampling_gpmpc_amd.rollout import rollout_device
    from sampling_gpmpc_amd.workloads import synthetic_u_ff
    lib = _lib.load()
    agent, z, x0 = case
    lib.gpmpc_rollout_pin_kernel(kernel)
    try:
        res = rollout_device(agent, synthetic_u_ff(1, H), z.reshape(-1), z.shape[1], H=H, mode=_lib.MODE_RECONDITIONED,
                             use_model_without_derivatives=False, use_feedback=feedback, x0=x0, var_zero_thr=-1.0,
                             want_samples=outputs)
        path = lib.gpmpc_debug_last_rollout_path()
        assert path == kernel, f"kernel path {path}, pinned {kernel}"
        return res.X_traj.cpu().numpy(), (res.Y.cpu().numpy() if outputs else None), res.info.cpu().numpy()
    finally:
        lib.gpmpc_rollout_pin_kernel(-1)


def key(H, feedback):
    return f"H{H}_fb{int(bool(feedback))}"


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    import sampling_gpmpc_amd as sg
    from sampling_gpmpc_amd import _lib
    _lib.load()
    out = {}
    for fb in (True, False):
        c = inputs(sg, fb)
        for H in GOLDEN_H:
            X, _, _ = launch(c, H, fb, _lib.KERNEL_ONE)
            assert np.isfinite(X).all()
            out[key(H, fb)] = X
    np.savez(sys.argv[1] if len(sys.argv) > 1 else OUT, **out)
    print({k: v.shape for k, v in out.items()})
