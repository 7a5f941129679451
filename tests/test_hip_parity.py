"""GPU parity tests: the HIP path (through the C-ABI, via the Agent facade) against the CPU oracle and against the
golden vectors captured from the reference's own code.  Run on the MI355X box with ``pytest -m gpu``.

Tolerance: BASELINE.json's north star asks for 1e-4 relative on the rollout outputs; the assertions below use
RTOL_TRAJ = 1e-6 (two orders tighter) and print the observed maximum error, which is expected around 1e-9
(FP64 throughout; the append-row factor differs from the oracle's from-scratch factor only by round-off times the
conditioning of K, ~1e5 pendulum / ~1e7 car).
"""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import agent_oracle as ao
from oracle.gp_oracle import F64, GPHyper, OracleGP
from tests.helpers import GOLDEN, fs_params, load_params, synthetic_u_ff

pytestmark = pytest.mark.gpu

RTOL_TRAJ = 1e-6
RTOL_NORTH_STAR = 1e-4


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")


@pytest.fixture(scope="module")
def sg():
    _require_gpu()
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


def relerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-300))


def make_agents(sg, p, erv=None):
    """Product Agent on the GPU and oracle Agent on the CPU sharing the same base samples."""
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    env = sg.make_env(pg)
    if erv is None:
        torch.manual_seed(123456)
        agent = sg.Agent(pg, env)
        erv = agent.epistimic_random_vector.cpu()
    else:
        # skip the (slow, reference-exact) generator: hand a tiny config to the constructor, then install erv
        small = {**pg, "common": {**pg["common"], "num_MPC_itrs": 1},
                 "optimizer": {**pg["optimizer"], "SEMPC": {**pg["optimizer"]["SEMPC"], "max_sqp_iter": 1}}}
        agent = sg.Agent(small, env)
        agent.params = pg
        agent.epistimic_random_vector = torch.as_tensor(erv, dtype=F64).to(agent.torch_device)
        # (the constructor sized the joint buffers for the tiny config: a factor cache that regrows mid-loop restarts from zero
        # cached rows, and the matrix-pipe path's results depend on the cache state to rounding - INTEGRATION.md)
        agent._ws_cache["joint_points_hint"] = int(pg["optimizer"]["SEMPC"]["max_sqp_iter"]) * int(pg["optimizer"]["H"])
    oenv = ao.make_oracle_env(p)
    oagent = ao.OracleAgent(p, oenv, torch.as_tensor(erv, dtype=F64).cpu())
    return agent, oagent


def test_device_selftest(sg):
    lib = sg._lib.load()
    sg._lib.check(lib.gpmpc_selftest(None), "gpmpc_selftest")
    name, cus, lds = sg._lib.device_info(0)
    print(f"device: {name}, {cus} CUs, {lds} B LDS/workgroup")
    assert "gfx950" in name


@pytest.mark.parametrize("pname,use_grad", [("params_pendulum1D_samples", True), ("params_car_residual", True),
                                            ("params_car_residual_fs", False)])
def test_plan_matches_dense_cholesky(sg, pname, use_grad):
    from sampling_gpmpc_amd.gp_model import GPHyperParams, RealDataPlan
    from oracle.gp_oracle import scaled_rbf_kernel
    p = load_params(pname)
    p["common"]["use_cuda"] = True
    env = sg.make_env(p)
    X, Y = env.initial_training_data()
    if not use_grad:
        Y = Y[:, :, [0]]
    plan = RealDataPlan(X.cuda(), Y.cuda(), GPHyperParams.from_params(p, use_grad))
    hy = GPHyper.from_params(p, use_grad)
    n = plan.n_r
    buf = plan.buf.cpu()
    n0, n1 = int(plan.desc.grid_n0), int(plan.desc.grid_n1)
    assert (n0, n1) == ((4, 9) if "pendulum" in pname else (5, 9)), "training grid not detected"
    # the plan's grid-root block and the mode-I table behind it (gpmpc_device.hpp: plan_doubles_per_output)
    c8 = lambda v: (v + 7) // 8
    tab_qa = 32
    tab_qb = tab_qa + 8 * c8(n0 * n0)
    tab_m1 = tab_qb + 8 * c8(n1 * n1)
    tab_m2 = tab_m1 + 8 * c8(n0 * n1)
    tab_len = 16 * ((tab_m2 + 8 * c8(n0 * n1) + 15) // 16)
    tab_ofs = (2 * n * n + 2 * n + n0 * n0 + n1 * n1 + 4 * n0 * n1 + 7) & ~7
    per = tab_ofs + tab_len
    for o in range(hy.ell.shape[0]):
        K = scaled_rbf_kernel(X, X, hy.ell[o], hy.outputscale[o], use_grad)
        T = hy.T
        obs = ~torch.isnan(Y[o].reshape(-1))
        K = (K + torch.diag(hy.noise_diag.repeat(X.shape[0])))[obs][:, obs]
        L = torch.linalg.cholesky(K)
        Linv = torch.linalg.inv(L)
        yo = Y[o].reshape(-1)[obs]
        blk = buf[o * per:(o + 1) * per]
        np.testing.assert_allclose(blk[:n * n].reshape(n, n).numpy(), L.numpy(), rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(blk[n * n:2 * n * n].reshape(n, n).T.numpy(), Linv.numpy(), rtol=1e-7,
                                   atol=1e-9 * float(Linv.abs().max()))
        np.testing.assert_allclose(blk[2 * n * n:2 * n * n + n].numpy(), (Linv @ yo).numpy(), rtol=1e-7,
                                   atol=1e-9 * float((Linv @ yo).abs().max()))
        alpha = torch.cholesky_solve(yo.unsqueeze(-1), L).squeeze(-1)
        np.testing.assert_allclose(blk[2 * n * n + n:2 * n * n + 2 * n].numpy(), alpha.numpy(), rtol=1e-6,
                                   atol=1e-7 * float(alpha.abs().max()))
        # grid root W = D^-1/2 (Qa (x) Qb)^T: W^T W = (K_rr + s2 I)^-1 and wE = W y (value-only real labels: n == N_r)
        assert n == n0 * n1
        g = blk[2 * n * n + 2 * n:]
        Qa, Qb = g[:n0 * n0].reshape(n0, n0), g[n0 * n0:n0 * n0 + n1 * n1].reshape(n1, n1)
        dsc, wE = g[n0 * n0 + n1 * n1:][:n], g[n0 * n0 + n1 * n1 + n:][:n]
        np.testing.assert_allclose((Qa.T @ Qa).numpy(), np.eye(n0), atol=1e-13)
        np.testing.assert_allclose((Qb.T @ Qb).numpy(), np.eye(n1), atol=1e-13)
        W = torch.diag(dsc / hy.outputscale[o]) @ torch.kron(Qa, Qb).T
        Kinv = torch.cholesky_inverse(L)
        assert float((W.T @ W - Kinv).abs().max()) < 1e-8 * float(Kinv.abs().max())
        assert float((W @ K @ W.T - torch.eye(n, dtype=K.dtype)).abs().max()) < 1e-9
        np.testing.assert_allclose(wE.numpy(), (W @ yo).numpy(), rtol=1e-7, atol=1e-9 * float((W @ yo).abs().max()))
        m1, m2 = g[n0 * n0 + n1 * n1 + 2 * n:][:n], g[n0 * n0 + n1 * n1 + 3 * n:][:n]
        np.testing.assert_allclose(m1.numpy(), (dsc * wE).numpy(), rtol=1e-14)
        np.testing.assert_allclose(m2.numpy(), (dsc * dsc).numpy(), rtol=1e-14)
        # mode-I table: axis points, Qa, Qb, m1, m2 packed in units of 8 doubles, zero padded
        tab = blk[tab_ofs:]
        Xc = X.cpu()
        ref = torch.zeros(tab_len, dtype=torch.float64)
        il = 1.0 / hy.ell[o].cpu() ** 2
        ha, hb = (Xc[-1, 0] - Xc[0, 0]) / (n0 - 1), (Xc[n1 - 1, 1] - Xc[0, 1]) / (n1 - 1)
        ref[0], ref[1], ref[2], ref[3] = Xc[0, 0], il[0] * ha, Xc[0, 1], il[1] * hb
        ka, kb = torch.arange(1, n0, dtype=torch.float64), torch.arange(1, n1, dtype=torch.float64)
        ref[4:4 + n0 - 1] = torch.exp(-0.5 * il[0] * (ka * ha) ** 2)
        ref[3 + n0:3 + n0 + n1 - 1] = torch.exp(-0.5 * il[1] * (kb * hb) ** 2)
        np.testing.assert_allclose(tab[:16].numpy(), ref[:16].numpy(), rtol=1e-14, atol=0)   # recurrence constants
        ref[:16] = tab[:16]
        ref[16:16 + n0] = Xc[::n1, 0]
        ref[16 + n0:16 + n0 + n1] = Xc[:n1, 1]
        ref[tab_qa:tab_qa + n0 * n0] = Qa.reshape(-1)
        ref[tab_qb:tab_qb + n1 * n1] = Qb.reshape(-1)
        ref[tab_m1:tab_m1 + n] = m1
        ref[tab_m2:tab_m2 + n] = m2
        np.testing.assert_array_equal(tab.numpy(), ref.numpy())


@pytest.mark.parametrize("tag,pname", [("R_pendulum1D", "params_pendulum1D_samples"),
                                       ("R_pendulum1D_nofb", "params_pendulum1D_samples"),
                                       ("I_car", "params_car_residual_fs"), ("R_car", "params_car_residual_fs")])
def test_rollout_against_reference_goldens(sg, tag, pname):
    """gpmpc_rollout == the reference Agent's code driven like simulate_forward_sampling_car.py (golden fixture)."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    d = np.load(os.path.join(GOLDEN, f"agent_e2e_{tag}.npz"))
    p = fs_params(pname, int(d["Ns"]), int(d["H_traj"]), nograd=bool(d["nograd"]), feedback=bool(d["feedback"]),
                  beta=float(d["beta"]))
    agent, _ = make_agents(sg, p, erv=d["epistimic_random_vector"])
    X, Y = forward_sampling_rollout(agent, d["u_ff"], return_samples=True)
    ex, ey = relerr(X, d["X_traj"]), relerr(Y, d["Y"])
    print(f"{tag}: rel err X_traj {ex:.2e}, Y {ey:.2e}")
    np.testing.assert_allclose(X, d["X_traj"], rtol=RTOL_TRAJ, atol=1e-9)
    np.testing.assert_allclose(Y, d["Y"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(agent.Hallcinated_X_train.cpu().numpy(), d["hall_X"], rtol=RTOL_TRAJ, atol=1e-9)
    np.testing.assert_allclose(agent.Hallcinated_Y_train.cpu().numpy(), d["hall_Y"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("pname,Ns,H,nograd,force_global", [
    ("params_pendulum1D_samples", 32, 10, False, False),      # BASELINE config 1 shape (LDS-resident factor)
    ("params_pendulum1D_samples", 32, 10, False, True),       # same through the HBM-workspace factor
    ("params_pendulum1D_samples", 48, 30, False, False),      # config 2 horizon, n_h up to 87 (2 rows per lane)
    ("params_car_residual_fs", 24, 40, False, False),         # config 3 horizon, T=3, n_h up to 117, HBM factor
    ("params_car_residual_fs", 64, 40, True, False),          # config 4 as shipped (mode I, T=1): thread-per-sample kernel
    ("params_car_residual_fs", 300, 7, True, False),          # mode I, ragged last workgroup (300 = 256 + 44)
    ("params_pendulum1D_samples", 40, 12, True, False),       # mode I on the 4x9 pendulum grid
])
def test_rollout_against_oracle(sg, pname, Ns, H, nograd, force_global, monkeypatch):
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    if force_global:
        monkeypatch.setenv("GPMPC_FORCE_GLOBAL_FACTOR", "1")
    p = fs_params(pname, Ns, H, nograd=nograd, beta=(3.0 if (not nograd and "car" in pname) else None))
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    X, Y = forward_sampling_rollout(agent, u_ff, return_samples=True)
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    ex, ey = relerr(X, Xo), relerr(Y, Yo)
    print(f"{pname} Ns={Ns} H={H} nograd={nograd} global={force_global}: rel err X_traj {ex:.2e}, Y {ey:.2e}")
    assert np.isfinite(X).all()
    assert ex < RTOL_TRAJ and ex < RTOL_NORTH_STAR
    np.testing.assert_allclose(Y, Yo, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("pname,Ns,H,feedback,n_data_x", [
    ("params_pendulum1D_samples", 6, 3, None, None),    # two appended points: one incomplete tile row
    ("params_pendulum1D_samples", 7, 12, None, None),   # ragged last wave (7 = 4 + 3 chains), 33 rows: every tile phase (n_h mod 4)
    ("params_pendulum1D_samples", 9, 30, None, None),   # configs[1] horizon: 87 rows = 22 tile rows, 12 resident + 10 streamed
    ("params_car_residual_fs", 3, 10, None, None),      # one sample = one wave (three outputs + the copy)
    ("params_car_residual_fs", 5, 40, None, None),      # configs[2] horizon: 117 rows = 30 tile rows
    ("params_car_residual_fs", 4, 43, False, None),     # the longest horizon the 32-tile kernel takes (126 rows), no feedback
    ("params_car_residual_fs", 3, 50, None, None),      # the shipped car horizon (params_car_residual.yaml): 147 rows, 40-tile kernel
    ("params_car_residual_fs", 2, 65, None, None),      # 192 rows: all 48 tile rows of the largest instance
    ("params_pendulum1D_samples", 5, 54, None, None),   # 159 rows of the 40-tile kernel, ragged wave
    ("params_pendulum1D_samples", 6, 60, None, None),   # 48-tile kernel
    ("params_pendulum1D_samples", 5, 25, None, 5),      # a 5 x 9 training grid
    ("params_car_residual_fs", 3, 40, None, 6),         # a 6 x 9 training grid (four registers of grid entries, 11 resident rows)
])
def test_tiled_rollout_against_oracle(sg, pname, Ns, H, feedback, n_data_x, monkeypatch):
    """rollout_tiles.hip (four chains per wave, forward substitution on the FP64 matrix pipe) is selected by size; forced
    here at small Ns against the oracle.  Same tolerances as the other rollout kernels."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    monkeypatch.setenv("GPMPC_ROLLOUT_TILES", "1")
    p = fs_params(pname, Ns, H, nograd=False, feedback=feedback, beta=(3.0 if "car" in pname else None))
    if n_data_x is not None:
        p["env"]["n_data_x"] = n_data_x
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    if H > 45:
        u_ff = u_ff * 0.5                                                   # keep the long rollouts near the data
    X, Y = forward_sampling_rollout(agent, u_ff, return_samples=True)
    assert sg._lib.load().gpmpc_debug_last_rollout_path() == 3, "the tiled kernel was not selected"
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    ex, ey = relerr(X, Xo), relerr(Y, Yo)
    print(f"tiled {pname} Ns={Ns} H={H} grid {n_data_x or 'shipped'} x 9: rel err X_traj {ex:.2e}, Y {ey:.2e}")
    assert np.isfinite(X).all()
    assert ex < RTOL_TRAJ and ex < RTOL_NORTH_STAR
    np.testing.assert_allclose(Y, Yo, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(agent.Hallcinated_X_train[:, 0].cpu().numpy(), oagent.Hallcinated_X_train[:, 0].numpy(), rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("Ns,H,feedback", [
    (1, 2, None),       # one appended point: the first group of diagonal tiles only
    (3, 3, None),       # two points: the first incomplete tile that wraps (rows 3, 4, 5)
    (7, 7, None),       # 18 rows: groups 2 and 3, a tile row that starts a group
    (5, 12, False),     # 33 rows, no feedback: every phase of n_h mod 4 and of the group boundaries
    (9, 22, None),      # 63 rows
    (6, 30, None),      # configs[1] horizon: 87 rows = all 22 tile rows, 122 panels
    (70, 30, None),     # more chains than a CU holds
])
def test_one_chain_mfma_rollout_against_oracle(sg, Ns, H, feedback, monkeypatch):
    """rollout_one.hip (one chain per wave, the factor as AGPR-pinned MFMA panels; BASELINE configs[1]'s kernel) against the
    oracle, the kernel asserted (path 4), and against rollout_fast_kernel (GPMPC_ROLLOUT_ONE=0) on the same base samples:
    two independent implementations of the same arithmetic agree to round-off."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    pname = "params_pendulum1D_samples"
    p = fs_params(pname, Ns, H, nograd=False, feedback=feedback)
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    lib = sg._lib.load()
    X, Y = forward_sampling_rollout(agent, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 4, "rollout_one_kernel was not selected"
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    monkeypatch.setenv("GPMPC_ROLLOUT_ONE", "0")
    agent2, _ = make_agents(sg, p, erv=agent.epistimic_random_vector.cpu().numpy())
    X1, Y1 = forward_sampling_rollout(agent2, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 1, "rollout_fast_kernel was not selected"
    ex, ey = relerr(X, Xo), relerr(Y, Yo)
    print(f"one-chain MFMA kernel Ns={Ns} H={H}: rel err X_traj {ex:.2e}, Y {ey:.2e}; vs rollout_fast max abs diff "
          f"X {np.abs(X - X1).max():.2e} Y {np.abs(Y - Y1).max():.2e}")
    assert np.isfinite(X).all()
    assert ex < RTOL_TRAJ and ex < RTOL_NORTH_STAR
    np.testing.assert_allclose(Y, Yo, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(agent.Hallcinated_X_train[:, 0].cpu().numpy(), oagent.Hallcinated_X_train[:, 0].numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(X, X1, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Y, Y1, rtol=1e-7, atol=1e-11)


@pytest.mark.parametrize("pname,Ns,H,n_data_x", [
    ("params_car_residual_fs", 90, 50, None),           # picked by itself: no tuned one-chain kernel for 147 rows, 270 chains
    ("params_car_residual_fs", 86, 30, 6),              # 6 x 9 grid
    ("params_pendulum1D_samples", 300, 20, 5),          # 5 x 9 grid
    ("params_pendulum1D_samples", 4100, 30, None),      # configs[1] shape at a sample count where four chains per wave win
])
def test_tiled_kernel_agrees_with_generic_kernel(sg, pname, Ns, H, n_data_x, monkeypatch):
    """Launch sizes at which the dispatcher picks the tiled kernel by itself (path 3), against the generic kernel
    (GPMPC_DISABLE_FAST_ROLLOUT=1, path 0) on the same base samples: round-off apart."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p = fs_params(pname, Ns, H, nograd=False, beta=(3.0 if "car" in pname else None))
    p["agent"]["base_sample_generator"] = "vectorized"
    if n_data_x is not None:
        p["env"]["n_data_x"] = n_data_x
    torch.manual_seed(5)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    agent = sg.Agent(pg, sg.make_env(pg))
    u_ff = synthetic_u_ff(agent.nu, H) * (0.5 if H > 45 else 1.0)
    lib = sg._lib.load()
    X_t, Y_t = forward_sampling_rollout(agent, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 3, "the tiled kernel was not selected"
    monkeypatch.setenv("GPMPC_DISABLE_FAST_ROLLOUT", "1")
    agent2 = sg.Agent(pg, sg.make_env(pg))
    agent2.epistimic_random_vector = agent.epistimic_random_vector.clone()
    X_g, Y_g = forward_sampling_rollout(agent2, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 0, "the generic kernel was not selected"
    print(f"{pname} Ns={Ns} H={H} grid {n_data_x or 'shipped'} x 9: tiled vs generic max abs diff X {np.abs(X_t - X_g).max():.2e} "
          f"Y {np.abs(Y_t - Y_g).max():.2e}")
    assert np.isfinite(X_t).all() and np.abs(X_t - X_g).max() > 0.0
    np.testing.assert_allclose(X_t, X_g, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(Y_t, Y_g, rtol=1e-6, atol=1e-10)


def test_rollout_sample_subset_invariance_full_size(sg):
    """BASELINE config 2 (Ns=1024, H=30): every sample's trajectory is independent of what else is in the launch
    (bit-exact on a re-launched subset), values are finite, and a 16-sample subset matches the oracle."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout, rollout_device
    from sampling_gpmpc_amd import _lib
    Ns, H = 1024, 30
    p = fs_params("params_pendulum1D_samples", Ns, H)
    p["agent"]["base_sample_generator"] = "vectorized"
    torch.manual_seed(7)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    agent = sg.Agent(pg, sg.make_env(pg))
    u_ff = synthetic_u_ff(1, H)
    X = forward_sampling_rollout(agent, u_ff)
    assert X.shape == (Ns, 2, H + 1) and np.isfinite(X).all()
    assert _lib.load().gpmpc_debug_last_rollout_path() == 4, "configs[1] is rollout_one_kernel's launch (the bench's kernel)"
    erv = agent.epistimic_random_vector
    per_slab = Ns * 3
    z = erv.reshape(-1)[per_slab:]
    sub = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, H=H, mode=_lib.MODE_RECONDITIONED,
                         use_model_without_derivatives=False, sample_slice=(500, 516))
    np.testing.assert_array_equal(sub.X_traj.cpu().numpy(), X[500:516])
    # oracle on the same 16 samples
    po = fs_params("params_pendulum1D_samples", 16, H)
    oagent = ao.OracleAgent(po, ao.make_oracle_env(po), erv[:, :, 500:516].cpu())
    Xo = ao.forward_sampling_rollout(oagent, u_ff)
    e = relerr(X[500:516], Xo)
    print(f"config 2 subset vs oracle: rel err {e:.2e}")
    assert e < RTOL_TRAJ
    # the sampled tube is a genuine spread around the mean trajectory
    assert X[:, 1, -1].std() > 1e-4


@pytest.mark.parametrize("pname,Ns,H,nograd", [("params_car_residual_fs", 262144, 40, True),     # BASELINE configs[3] as shipped
                                               ("params_car_residual_fs", 4096, 40, False),      # configs[2]
                                               ("params_car_residual_fs", 262144, 40, False)])   # configs[3] re-conditioned (T=3)
def test_car_rollout_full_size_properties(sg, pname, Ns, H, nograd, monkeypatch):
    """BASELINE full sizes of the car workloads (mode I, Ns=262144: the true-reachable-set launch of one GPU; mode R,
    Ns=4096; mode R at Ns=262144 - SURVEY cfg4's re-conditioned variant, 786432 chains, a 44 GB factor workspace): finite, error-free info words, every sample independent of what else is in the launch (bit-exact on
    re-launched subsets, incl. one that straddles workgroups and the ragged last one) and a 12-sample subset equal to
    the oracle."""
    from sampling_gpmpc_amd.rollout import rollout_device
    from sampling_gpmpc_amd import _lib
    p = fs_params(pname, Ns, H, nograd=nograd, beta=(None if nograd else 3.0))
    p["agent"]["base_sample_generator"] = "vectorized" if Ns * (1 if nograd else 3) < 500000 else "counter"   # counter: on the device
    torch.manual_seed(11)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    agent = sg.Agent(pg, sg.make_env(pg))
    u_ff = synthetic_u_ff(agent.nu, H)
    T = 1 if nograd else 3
    mode = _lib.MODE_INDEPENDENT if nograd else _lib.MODE_RECONDITIONED
    erv = agent.epistimic_random_vector
    per_slab = Ns * agent.g_ny * T
    z = erv.reshape(-1)[per_slab:]
    full = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, H=H, mode=mode, use_model_without_derivatives=nograd)
    X = full.X_traj
    assert X.shape == (Ns, 4, H + 1) and bool(torch.isfinite(X).all())
    assert int(full.info.max().item()) & (_lib.INFO_TRAIN_CHOL_FAIL | _lib.INFO_ROOT_FAIL) == 0
    path = _lib.load().gpmpc_debug_last_rollout_path()
    if not nograd:
        assert path == 3, "mode R at these sizes belongs to the four-chains-per-wave kernel"
        monkeypatch.setenv("GPMPC_ROLLOUT_TILES", "1")           # small launches pick the one-chain kernel by themselves:
    for lo, hi in ((0, 5), (Ns // 2 - 37, Ns // 2 + 91), (Ns - 3, Ns)):   # bit-exactness is a property of ONE kernel
        sub = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, H=H, mode=mode,
                             use_model_without_derivatives=nograd, sample_slice=(lo, hi))
        assert _lib.load().gpmpc_debug_last_rollout_path() == path
        assert torch.equal(sub.X_traj, X[lo:hi]), (lo, hi)
    lo = Ns // 3
    po = fs_params(pname, 12, H, nograd=nograd, beta=(None if nograd else 3.0))
    oagent = ao.OracleAgent(po, ao.make_oracle_env(po), erv[:, :, lo:lo + 12].cpu())
    Xo = ao.forward_sampling_rollout(oagent, u_ff)
    e = relerr(X[lo:lo + 12].cpu().numpy(), Xo)
    print(f"{pname} Ns={Ns} mode {'I' if nograd else 'R'}: 12-sample subset vs oracle rel err {e:.2e}")
    assert e < RTOL_TRAJ
    assert float(X[:, 1, -1].std()) > 1e-6                    # a genuine spread


@pytest.mark.parametrize("pname,Ns,H,feedback,x0", [
    ("params_car_residual_fs", 70, 40, False, None),                        # open loop (no feedback law)
    ("params_car_residual_fs", 9, 40, True, [0.5, 1.2, 0.1, 9.0]),          # another start state
    ("params_car_residual_fs", 6, 300, True, None),                         # H > 256: the input sequence is read from memory
    ("params_pendulum1D_samples", 66, 33, False, [2.4, -0.5]),
])
def test_mode_i_variants_against_oracle(sg, pname, Ns, H, feedback, x0):
    """Mode I beyond the shipped configuration: without the feedback law, from another start state, and with a horizon
    longer than the grid kernel stages in LDS (the input sequence is then read from memory)."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p = fs_params(pname, Ns, H, nograd=True, feedback=feedback)
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    if H > 100:
        u_ff = u_ff * 0.2                                                   # keep the long car rollout near the data
    X, Y = forward_sampling_rollout(agent, u_ff, x0=x0, return_samples=True)
    assert sg._lib.load().gpmpc_debug_last_rollout_path() == 2
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, x0=x0, return_samples=True)
    print(f"{pname} Ns={Ns} H={H} feedback={feedback} x0={x0}: rel err X_traj {relerr(X, Xo):.2e}, Y {relerr(Y, Yo):.2e}")
    assert np.isfinite(X).all() and relerr(X, Xo) < RTOL_TRAJ
    np.testing.assert_allclose(Y, Yo, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("path", ["auto", "mfma"])
def test_joint_draw_against_reference_golden(sg, path):
    """Mode J as the SQP loop drives it (two iterations; the second conditions on the first's 8 sampled points) against the outputs of
    the REFERENCE's own code (tests/golden/agent_e2e_J_pendulum1D.npz).  "auto": the dispatcher's choice (24 hallucinated slots: the VALU
    path); "mfma": the matrix-pipe path pinned - its second iteration runs joint_test_mfma_kernel (factor extension + test rows)."""
    lib = sg._lib.load()
    lib.gpmpc_joint_pin_path(sg._lib.JOINT_MFMA if path == "mfma" else sg._lib.JOINT_AUTO)
    try:
        _joint_draw_against_reference_golden(sg, path)
    finally:
        lib.gpmpc_joint_pin_path(sg._lib.JOINT_AUTO)


def _joint_draw_against_reference_golden(sg, path):
    d = np.load(os.path.join(GOLDEN, "agent_e2e_J_pendulum1D.npz"))
    p = load_params("params_pendulum1D_samples")
    Ns, H = int(d["Ns"]), int(d["H"])
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 2, 2
    agent, _ = make_agents(sg, p, erv=d["epistimic_random_vector"])
    K = np.array(p["optimizer"]["terminal_tightening"]["K"])
    x_equi = np.array(p["env"]["goal_state"])
    agent.mpc_iteration(0)
    for it in range(2):
        x_h = d[f"x_h_{it}"]
        agent.train_hallucinated_dynGP(it)
        bx = agent.get_batch_x_hat_u_diff(
            x_h, -(x_equi - x_h.reshape(H, Ns, -1)) @ K.T + np.tile(d["u_h"][:, None, :], (Ns, 1)))
        gp_val, y_grad, u_grad = agent.dyn_fg_jacobians(bx, it)
        if it >= 1:
            assert sg._lib.load().gpmpc_joint_last_path() == (sg._lib.JOINT_MFMA if path == "mfma" else sg._lib.JOINT_VALU)
        assert gp_val.dtype == np.float64 and gp_val.shape == (Ns, 2, H, 1)
        np.testing.assert_allclose(agent.model_i_call.mean.cpu().numpy(), d[f"mean_{it}"], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(agent.model_i_call.variance.cpu().numpy(), d[f"var_{it}"], rtol=1e-5, atol=1e-12)
        # The 24x24 posterior covariance is numerically singular: whether the un-jittered Cholesky "succeeds" is a
        # round-off coin flip, so samples are compared where both sides took the same branch.
        lvl = ((agent.model_i_call.last_info.cpu().numpy() >> 1) & 7)[:, 0]
        ref_lvl = (d[f"jitter_{it}"][:, 0] > 0).astype(int)
        print(f"J iter {it}: jitter levels hip {lvl} ref {ref_lvl}")
        # Samples are only well defined where BOTH sides took the jitter branch: an un-jittered factor of a singular
        # matrix has round-off sized trailing pivots (1e-12..1e-17), i.e. the sampled components are noise on both
        # sides and depend on the summation order of the factorisation.
        both_jit = (lvl == 1) & (ref_lvl == 1)
        if both_jit.any():
            np.testing.assert_allclose(gp_val[both_jit], d[f"gp_val_{it}"][both_jit], rtol=1e-5, atol=1e-8)
            np.testing.assert_allclose(y_grad[both_jit], d[f"y_grad_{it}"][both_jit], rtol=1e-4, atol=1e-7)
            np.testing.assert_allclose(u_grad[both_jit], d[f"u_grad_{it}"][both_jit], rtol=1e-4, atol=1e-7)
        # value components stay close even on the un-jittered branch (their variance is not the degenerate part)
        np.testing.assert_allclose(gp_val, d[f"gp_val_{it}"], rtol=0, atol=5e-3)
        # the next SQP iteration conditions on THIS iteration's draws: continue from the reference's own labels so
        # that a different coin flip above does not leak into the next comparison
        agent.Hallcinated_Y_train = torch.tensor(d[f"y_{it}"]).to(agent.torch_device)


@pytest.mark.parametrize("pname,Ns,H,iters", [
    ("params_pendulum1D_samples", 16, 30, 2),     # 91 / 181 label rows: 128- and 256-thread workgroups
    ("params_car_residual", 8, 12, 3),
    ("params_pendulum1D_samples", 6, 30, 7),      # up to 631 rows: 512-thread workgroups, then 1024 threads
    ("params_pendulum1D_samples", 3, 30, 13),     # up to 1171 rows: two rows per thread (beyond 1024 rows)
])
def test_joint_draw_against_oracle(sg, pname, Ns, H, iters):
    """sample_gp / dyn_fg_jacobians over several SQP iterations vs the oracle (mean, variance, covariance, samples)."""
    _joint_draw_against_oracle(sg, pname, Ns, H, iters)


@pytest.mark.parametrize("pname,Ns,H,iters,cache", [
    ("params_car_residual", 8, 40, 4, True),          # the closed loop's shape: 45 + 360 conditioning slots = 26 tiles at k = 3, 121 columns
    ("params_car_residual", 5, 40, 3, False),         # no caller-owned cache: the factor rows go through the workspace's temporary one
    ("params_pendulum1D_samples", 16, 30, 4, True),   # 36 real slots, 91 columns = 6 of the 8 column tiles
    ("params_car_residual", 8, 12, 3, True),          # 37 columns: 3 column tiles, a ragged last slot tile at every k
    # conditioning sets beyond one launch (416 slots): the test rows as TOP + BOTTOM launches (round 5c)
    ("params_car_residual", 4, 40, 5, True),          # k = 4: 45 + 480 slots = 26 + 7 tiles (the k = 0 draw of MPC steps >= 1 at configs[4])
    ("params_pendulum1D_samples", 6, 30, 6, True),    # k = 5: 36 + 450 = 486 slots, a ragged fifth bottom tile; 91 columns
])
def test_joint_draw_matrix_pipe_against_oracle(sg, pname, Ns, H, iters, cache):
    """The same comparison with the matrix-pipe path pinned (ABI 7: gpmpc_joint_pin_path): factor extension and test rows by
    joint_test_mfma_kernel (FP64 MFMA, X blocks in registers, L tiles streamed HBM -> LDS), Cholesky of the Schur complement
    and root + sample by joint_kernel's phases - against the oracle, which factorises everything from scratch in one piece
    (reference src/agent.py:629-641 per src/solver.py:84-94).  The path that ran is asserted."""
    lib = sg._lib.load()
    lib.gpmpc_joint_pin_path(sg._lib.JOINT_MFMA)
    try:
        _joint_draw_against_oracle(sg, pname, Ns, H, iters, expect_path=sg._lib.JOINT_MFMA, cache=cache)
    finally:
        lib.gpmpc_joint_pin_path(sg._lib.JOINT_AUTO)


def joint_draw_comparison_block(agent, oagent, p, it, outs, oouts, tag="", sigma_bound=None):
    """One joint draw of the HIP Agent against the same draw of the oracle Agent (both have just run ``dyn_fg_jacobians``, whose
    results are ``outs`` / ``oouts``; ``it``: the SQP iteration, ``agent.mpc_iter``: the MPC step of the base samples): mean, variance,
    covariance, the samples at the kernel's own jitter level on the oracle's covariance, the legitimacy of a retry, and the Jacobians
    where both sides took the same level.  ``sigma_bound``: absolute bound on max|Sigma - Sigma_o| (default: 1e-7 max|Sigma_o|).
    Returns the measured covariance error and its scale."""
    gp_val, y_grad, u_grad = outs
    ogp_val, oy_grad, ou_grad = oouts
    post, opost = agent.model_i_call, oagent.model_i_call
    Ns = int(opost.mean.shape[0])
    np.testing.assert_allclose(post.mean.cpu().numpy(), opost.mean.numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(post.variance.cpu().numpy(), opost.variance.numpy(), rtol=1e-4, atol=1e-12)
    S, So = post.covariance_matrix.cpu().numpy(), opost.covariance_matrix.numpy()
    err_S, scale_S = float(np.max(np.abs(S - So))), float(np.max(np.abs(So)))
    bound_S = 1e-7 * scale_S if sigma_bound is None else float(sigma_bound)
    print(f"{tag} it={it}: |Sigma - Sigma_o| {err_S:.2e} = {err_S / scale_S:.1e} max|Sigma_o| (bound {bound_S / scale_S:.1e})")
    assert err_S < bound_S
    lvl = ((post.last_info.cpu().numpy() >> 1) & 7)
    ojit = opost.root_info.jitter_added.numpy()
    olvl = np.where(ojit == 0, 0, np.round(np.log10(np.maximum(ojit, 1e-300) / p["agent"]["Dyn_gp_jitter"])) + 1)
    same = (lvl == olvl).all(axis=1)
    print(f"{tag} it={it}: n_h={oagent.model_i.train_inputs[0].shape[2]}, jitter levels agree on "
          f"{same.sum()}/{Ns} samples; max level {lvl.max()}")
    # Whether the un-jittered attempt on the numerically singular Sigma passes is a round-off coin flip (+-1e-17
    # pivots), so the retry LEVEL may differ between LAPACK and the kernel.  What is defined for EVERY sample: given
    # the level the kernel took, its draw is mu + chol(Sigma + level I) z on the oracle's Sigma (clipped), and a
    # retry is legitimate only if the level below fails or is borderline (pivot < 1e-12 max|Sigma|) there.
    jit0 = p["agent"]["Dyn_gp_jitter"]
    So_t, mu_o, var_o = opost.covariance_matrix, opost.mean, opost.variance
    n = So_t.shape[-1]
    eye = torch.eye(n, dtype=F64)
    lvl_t = torch.as_tensor(lvl.astype(np.int64))
    jit_k = torch.where(lvl_t == 0, torch.zeros(lvl_t.shape, dtype=F64), jit0 * 10.0 ** (lvl_t.to(F64) - 1))
    Lk, info_k = torch.linalg.cholesky_ex(So_t + jit_k[..., None, None] * eye)
    z_it = agent.epistimic_random_vector[agent.mpc_iter][it].cpu().to(F64)
    y_ref = mu_o + (Lk @ z_it.reshape(Ns, -1, n, 1)).reshape(mu_o.shape)
    sd = p["agent"]["Dyn_gp_beta"] * var_o.sqrt()
    y_ref = torch.min(torch.max(y_ref, mu_o - sd), mu_o + sd)
    ok_k = (info_k == 0)
    # (a level-0 pass of the kernel on a matrix LAPACK rejects at the same level is the coin flip itself: compare
    # those samples at the oracle's level instead - they are the `same == False` ones with lvl == 0)
    cmp = ok_k.all(dim=1).numpy()
    assert cmp.sum() >= Ns - (~same).sum(), "the kernel's level must factorise on the oracle's matrix"
    np.testing.assert_allclose(agent.model_i_samples.cpu().numpy()[cmp], y_ref.numpy()[cmp], rtol=2e-5, atol=1e-8)
    scale_o = So_t.abs().amax(dim=(-1, -2))
    jit_p = torch.where(lvl_t <= 1, torch.zeros(lvl_t.shape, dtype=F64), jit0 * 10.0 ** (lvl_t.to(F64) - 2))
    Lp, info_p = torch.linalg.cholesky_ex(So_t + jit_p[..., None, None] * eye)
    minpiv = (torch.diagonal(Lp, dim1=-1, dim2=-2) ** 2).amin(dim=-1)
    legit = (lvl_t == 0) | (info_p > 0) | (minpiv < 1e-12 * scale_o)
    assert bool(legit.all()), "a jitter retry on a matrix that is clearly positive definite one level below"
    print(f"    all {int(cmp.sum())}/{Ns} samples match mu + chol(Sigma + level I) z at the kernel's own level; retries legitimate")
    np.testing.assert_allclose(gp_val[same], ogp_val[same], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(y_grad[same], oy_grad[same], rtol=1e-3, atol=1e-6)
    np.testing.assert_allclose(u_grad[same], ou_grad[same], rtol=1e-3, atol=1e-6)
    return err_S, scale_S


def joint_call_state(sg, agent):
    """What the joint draw the Agent has just made was given and did, read BEFORE anything repeats the posterior (a later
    ``covariance_matrix`` is a second launch of the same posterior object and overwrites these attributes): cached rows, the pending
    mask the facade passed, the path that ran, and the launch plan of that very call (``gpmpc_debug_joint_plan`` with the call's own
    arguments under the current knobs)."""
    import ctypes
    lib = sg._lib.load()
    post, mdl = agent.model_i_call, agent.model_i
    fc = agent._ws_cache.get("joint_factor_cache")
    Ns, _, m, _ = post._x.shape
    n_ho = int(mdl.h_slots.numel())
    # (the facade hands the entry point its cache from 16 observed slots on: JointFactorCache.prepare)
    cache_rows = int(fc.rows) if (fc is not None and fc.enabled and fc.buf is not None and n_ho >= 16) else 0
    raw = ctypes.CDLL(sg._lib.LIB_PATH)
    raw.gpmpc_debug_joint_plan.argtypes = [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_int32] * 8 + [ctypes.c_char_p, ctypes.c_size_t]

    def plan(ns, rows, n_c, pend):
        buf = ctypes.create_string_buffer(512)
        rc = raw.gpmpc_debug_joint_plan(ctypes.addressof(mdl.plan.desc), int(ns), int(mdl.n_h), n_ho, int(m), rows, n_c, pend, 0, 0, buf, 512)
        assert rc == 0
        return buf.value.decode()

    # a cache that holds a prefix of the samples: two launches - the prefix with the cache, the rest without ("plan_rest")
    n_cs = int(fc.n_samples) if cache_rows else 0
    prefix = 0 < n_cs < Ns
    return {"n_cached_rows": int(post.n_cached_rows), "used_pending": bool(post.used_pending), "pending_mask": int(post.pending_mask),
            "cache_rows": cache_rows, "cache_samples": n_cs, "n_h": int(mdl.n_h), "n_ho": n_ho,
            "path": int(lib.gpmpc_joint_last_path()), "bits": int(post.last_bits),
            "plan": plan(n_cs if prefix else Ns, cache_rows, int(post.n_cached_rows), int(post.pending_mask)),
            "plan_rest": plan(Ns - n_cs, 0, 0, 0) if prefix else None}


def _joint_draw_against_oracle(sg, pname, Ns, H, iters, expect_path=None, cache=True, follow="oracle", check_call=None):
    """``follow``: whose hallucinated tensors both Agents continue from.  "oracle": the HIP Agent is ASSIGNED the oracle's after every
    iteration - a new hallucinated-set generation (Agent's property setters), so its factor cache is never hit.  "hip": the oracle adopts
    the HIP Agent's, whose attributes are never assigned: its generation survives, the cache is hit from the third iteration on and the
    draws use their predecessors' pending rows.  ``check_call(it, state)``: called with ``joint_call_state`` of every draw."""
    assert follow in ("oracle", "hip")
    p = load_params(pname)
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["agent"]["true_dyn_as_sample"] = False
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, iters
    if "car" in pname:
        p["agent"]["Dyn_gp_jitter"] = 1e-9     # keep the car on the Cholesky branch (1e-20 -> eigh, tested below)
    agent, oagent = make_agents(sg, p)
    nx, nu = agent.nx, agent.nu
    g = torch.Generator().manual_seed(5)
    x0 = np.array(p["env"]["start"], dtype=np.float64)
    for it in range(iters):
        x_h = np.tile(x0, (H, Ns)) + 0.05 * torch.randn(H, Ns * nx, generator=g, dtype=F64).numpy() \
            + 0.02 * np.arange(H)[:, None]
        u_h = 0.3 * torch.randn(H, Ns, nu, generator=g, dtype=F64).numpy()
        agent.train_hallucinated_dynGP(it)
        oagent.train_hallucinated_dynGP(it)
        bx = agent.get_batch_x_hat_u_diff(x_h, u_h)
        obx = oagent.get_batch_x_hat_u_diff(x_h, u_h)
        if not cache:
            from sampling_gpmpc_amd.gp_model import JointFactorCache
            off = JointFactorCache()
            off.enabled = False
            agent._ws_cache["joint_factor_cache"] = off
        outs = agent.dyn_fg_jacobians(bx, it)
        if expect_path is not None and it >= 1:
            assert sg._lib.load().gpmpc_joint_last_path() == expect_path, "the pinned joint path did not run"
        if check_call is not None:
            state = joint_call_state(sg, agent)
            print(f"{pname} it={it}: cached rows {state['n_cached_rows']} of {state['n_ho']}, pending mask {state['pending_mask']}, "
                  f"used_pending {state['used_pending']}; {state['plan']}")
            check_call(it, state)
        oouts = oagent.dyn_fg_jacobians(obx, it)
        joint_draw_comparison_block(agent, oagent, p, it, outs, oouts, tag=pname)
        # keep both agents on the SAME hallucinated data for the next iteration
        if follow == "oracle":
            agent.Hallcinated_X_train = oagent.Hallcinated_X_train.to(agent.torch_device)
            agent.Hallcinated_Y_train = oagent.Hallcinated_Y_train.to(agent.torch_device)
        else:
            oagent.Hallcinated_X_train = agent.Hallcinated_X_train.cpu()
            oagent.Hallcinated_Y_train = agent.Hallcinated_Y_train.cpu()


CACHE_HIT_SHAPES = [
    ("params_car_residual", 8, 40, 4),            # 45 + 360 slots at it = 3: 26 tiles, 121 columns = 8 column tiles
    ("params_pendulum1D_samples", 16, 30, 4),     # 36 real slots, 91 columns = 6 column tiles
    ("params_car_residual", 8, 12, 3),            # 37 columns: 3 column tiles, a ragged last slot tile at every iteration
    ("params_car_residual", 4, 40, 5),            # it = 4: 45 + 480 = 525 slots, TOP + BOTTOM behind 360 cached rows
    ("params_pendulum1D_samples", 6, 30, 6),      # it = 4: 36 + 360 = 396 slots, the one-launch limit; it = 5: 486 slots, ragged bottom tile
]


@pytest.mark.parametrize("pending", ["1", "0"])
@pytest.mark.parametrize("pname,Ns,H,iters", CACHE_HIT_SHAPES)
def test_joint_draw_matrix_pipe_cache_hit_against_oracle(sg, pname, Ns, H, iters, pending, monkeypatch):
    """The cached shapes of test_joint_draw_matrix_pipe_against_oracle with the factor cache HIT: the oracle follows the kernel, so the
    HIP Agent's hallucinated-set generation survives and from the third iteration on a draw reuses the cached factor rows
    (``n_cached_rows == (it - 1) H T``).  With pending rows (GPMPC_JOINT_PENDING=1) it only factorises in place the X^T / S block its
    predecessor left behind - joint_chol_mfma_kernel(pend_use), joint_test_mfma_kernel(TEST, pend_write, Sv=cache),
    joint_tail_mfma_kernel(Sv=cache); without them the new rows are joint_test_mfma_kernel(FACTOR) against the cached columns; beyond 416
    slots the test rows are TOP + BOTTOM behind the hit cache.  The launch plan of every call is read with the call's own arguments and
    must contain the steps named here; the comparison is the one of the other joint-draw tests, at its tolerances (the oracle's own
    result moves by at most 8e-10 max|Sigma| under a reversal of its conditioning set at these scattered points)."""
    monkeypatch.setenv("GPMPC_JOINT_PENDING", pending)
    on, T = pending == "1", 3
    seen = set()

    def check_call(it, st):
        plan = st["plan"].split("|")[1].strip()
        assert st["path"] == sg._lib.JOINT_MFMA and st["plan"].startswith("path=2 batches=1 ")
        assert st["n_cached_rows"] == (0 if it <= 1 else (it - 1) * H * T)
        assert st["used_pending"] == (on and it >= 2)
        assert "joint_kernel(" not in plan
        split = "TEST_TOP" in plan
        assert split == (st["n_ho"] + (45 if "car" in pname else 36) > 416)
        if split:
            assert "joint_test_mfma(TEST_TOP) joint_test_mfma(TEST_BOTTOM)" in plan
        if it >= 2:
            assert plan.startswith("joint_chol_mfma(pend_use) " if on else "joint_test_mfma(FACTOR) joint_chol_mfma() ")
        if on and it >= 1 and not split:
            assert "joint_test_mfma(TEST,pend_write,Sv=cache)" in plan and "Sv=cache)" in plan.split("joint_tail_mfma(")[1]
        seen.update(s.split(")")[0] + ")" for s in plan.split(" "))

    lib = sg._lib.load()
    lib.gpmpc_joint_pin_path(sg._lib.JOINT_MFMA)
    try:
        _joint_draw_against_oracle(sg, pname, Ns, H, iters, expect_path=sg._lib.JOINT_MFMA, follow="hip", check_call=check_call)
    finally:
        lib.gpmpc_joint_pin_path(sg._lib.JOINT_AUTO)
    assert ("joint_chol_mfma(pend_use)" if on else "joint_test_mfma(FACTOR)") in seen
    if iters >= 5:
        assert "joint_test_mfma(TEST_TOP)" in seen and "joint_test_mfma(TEST_BOTTOM)" in seen


def test_joint_draw_eigh_fallback_distribution(sg):
    """car_residual ships Dyn_gp_jitter = 1e-20: every retry fails and gpytorch falls back to an eigh root for the
    whole batch.  Eigenvector signs are solver specific, so parity is asserted on what is well defined: mean,
    variance, covariance, and R R^T == max(Sigma, 0) for the root actually used."""
    p = load_params("params_car_residual")
    Ns, H = 4, 20
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["agent"]["true_dyn_as_sample"] = False
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 1
    agent, oagent = make_agents(sg, p)
    g = torch.Generator().manual_seed(9)
    x_h = np.tile(np.array(p["env"]["start"]), (H, Ns)) + 0.01 * torch.randn(H, Ns * 4, generator=g, dtype=F64).numpy()
    u_h = 0.05 * torch.randn(H, Ns, 2, generator=g, dtype=F64).numpy()
    agent.train_hallucinated_dynGP(0)
    oagent.train_hallucinated_dynGP(0)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y = agent.sample_gp(agent.env_model.get_g_xu_hat(agent.get_batch_x_hat_u_diff(x_h, u_h)).contiguous(),
                            base_samples=agent.epistimic_random_vector[0][0])
    yo = oagent.sample_gp(oagent.env_model.get_g_xu_hat(oagent.get_batch_x_hat_u_diff(x_h, u_h)),
                          base_samples=oagent.epistimic_random_vector[0][0])
    assert oagent.model_i_call.root_info.used_eigh, "oracle expected to take the eigh branch at jitter 1e-20"
    bits = int(agent.model_i_call.last_info.max().item())
    assert bits & sg._lib.INFO_ROOT_FAIL
    np.testing.assert_allclose(agent.model_i_call.mean.cpu().numpy(), oagent.model_i_call.mean.numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(agent.model_i_call.variance.cpu().numpy(), oagent.model_i_call.variance.numpy(),
                               rtol=1e-4, atol=1e-12)
    assert torch.isfinite(y).all()
    # both samples live in the same clip band
    mean, var = oagent.model_i_call.mean.numpy(), oagent.model_i_call.variance.numpy()
    band = p["agent"]["Dyn_gp_beta"] * np.sqrt(var)
    assert (np.abs(y.cpu().numpy() - mean) <= band * (1 + 1e-6) + 1e-12).all()


@pytest.mark.parametrize("tag,pname", [("pendulum1D", "params_pendulum1D_samples"), ("car_residual", "params_car_residual")])
def test_dyn_fg_jacobians_plumbing_golden(sg, tag, pname):
    """Padding / B_d / velocity transform / split / dtype / return type against the reference's own dyn_fg_jacobians
    (golden captured with an injected GP sample), plus the device-side p_lin packing against the host loop."""
    d = np.load(os.path.join(GOLDEN, f"agent_plumbing_{tag}.npz"))
    p = load_params(pname)
    Ns, H = int(d["Ns"]), int(d["H"])
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["agent"]["true_dyn_as_sample"] = False
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = int(d["n_mpc"]), int(d["n_itr"])
    agent, _ = make_agents(sg, p, erv=d["epistimic_random_vector"])
    agent.train_hallucinated_dynGP(0)
    y_inj = torch.tensor(d["y_inj"]).cuda()
    agent.get_batch_gp_sensitivities = lambda xu, it: y_inj.clone()
    bxd = agent.get_batch_x_hat_u_diff(d["x_h"], d["u_diff"])
    np.testing.assert_array_equal(bxd.cpu().numpy(), d["batch_x_hat_u_diff"])
    gp_val, y_grad, u_grad = agent.dyn_fg_jacobians(bxd, 0)
    for a, b in [(gp_val, d["gp_val"]), (y_grad, d["y_grad"]), (u_grad, d["u_grad"])]:
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-14)
    # p_lin: reference src/solver.py:98-131 host loop restated literally
    nx, nu = agent.nx, agent.nu
    x_h, u_h = d["x_h"], d["u_h"]
    xg, w = np.ones(H + 1) * 2.0, np.ones(H + 1) * 50.0
    got = agent.pack_p_lin(x_h, u_h, xg, w)
    for stage in range(H):
        p_lin = np.empty(0)
        for i in range(Ns):
            p_lin = np.concatenate([p_lin, y_grad[i, :, stage, :].reshape(-1), u_grad[i, :, stage, :].reshape(-1),
                                    x_h[stage, i * nx: nx * (i + 1)], gp_val[i, :, stage, :].reshape(-1)])
        p_lin = np.hstack([p_lin, u_h[stage], xg[stage], w[stage], agent.tilde_eps_list[stage]])
        np.testing.assert_array_equal(got[stage], p_lin)
    # the fused SQP-iteration call (ABI 8: one upload, gpmpc_build_x_hat, the draw, gpmpc_assemble_jacobians_plin, one download):
    # the same stage vectors, bit for bit, as the reference's literal loop over the reference-run golden arrays - with the
    # per-sample inputs of the feedback form (src/solver.py:86-90, K folded into A_i) and with the shared inputs (:92-94)
    K = np.arange(1, nu * nx + 1, dtype=np.float64).reshape(nu, nx) / 7.0
    for per_sample, Kfb in ((True, None), (True, K), (False, None)):
        u_in = d["u_diff"] if per_sample else u_h
        got2 = agent.sqp_linearisation(x_h, u_in, 0, xg, w, K=Kfb, u_nominal=u_h, train=False)
        gv, yg, ug = (t.cpu().numpy() for t in agent._last_device_jacobians)
        bx = agent.get_batch_x_hat_u_diff(x_h, u_in) if per_sample else agent.get_batch_x_hat(x_h, u_in)
        rv, ry, ru = agent.dyn_fg_jacobians(bx, 0)
        for a, b in ((gv, rv), (yg, ry), (ug, ru)):
            np.testing.assert_array_equal(a, b)
        A = ry + (ru @ Kfb if Kfb is not None else 0.0)
        for stage in range(H):
            ref = np.empty(0)
            for i in range(Ns):
                ref = np.concatenate([ref, A[i, :, stage, :].reshape(-1), ru[i, :, stage, :].reshape(-1),
                                      x_h[stage, i * nx: nx * (i + 1)], rv[i, :, stage, :].reshape(-1)])
            ref = np.hstack([ref, u_h[stage], xg[stage], w[stage], agent.tilde_eps_list[stage]])
            if Kfb is None:
                np.testing.assert_array_equal(got2[stage], ref)
            else:                                                # y_grad + u_grad K: the kernel sums nu products, numpy's matmul may pair them differently
                np.testing.assert_allclose(got2[stage], ref, rtol=1e-15, atol=1e-15)


def test_model_i_surface(sg):
    """Attributes the reference's visualiser / benchmarking scripts read from model_i and model_i(x)."""
    p = load_params("params_pendulum1D_samples")
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = 5, 4
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 1
    agent, oagent = make_agents(sg, p)
    agent.train_hallucinated_dynGP(0)
    oagent.train_hallucinated_dynGP(0)
    m = agent.model_i
    assert m.eval() is m and tuple(m.batch_shape) == (5, 1)
    assert tuple(m.train_inputs[0].shape) == (5, 1, 36, 2) and tuple(m.train_targets.shape) == (5, 1, 36, 3)
    x = torch.rand(5, 1, 4, 2, dtype=F64) * torch.tensor([1.5, 10.0]) + torch.tensor([2.1, -5.0])
    post, opost = m(x.cuda()), oagent.model_i(x)
    np.testing.assert_allclose(post.mean.cpu().numpy(), opost.mean.numpy(), rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(post.variance.cpu().numpy(), opost.variance.numpy(), rtol=1e-5, atol=1e-13)
    lo, hi = post.confidence_region()
    olo, ohi = opost.confidence_region()
    np.testing.assert_allclose(lo.cpu().numpy(), olo.numpy(), rtol=1e-6, atol=1e-9)
    z = torch.randn(5, 1, 4, 3, dtype=F64)
    np.testing.assert_allclose(post.sample(z.cuda()).cpu().numpy(), opost.sample(z).numpy(), rtol=1e-5, atol=1e-8)
    assert tuple(post.sample().shape) == (5, 1, 4, 3)
    with pytest.raises(RuntimeError):
        post.sample(torch.zeros(5, 1, 4, 2, dtype=F64).cuda())


def test_true_reachable_set_rollout_against_oracle(sg):
    """Open-loop, internally drawn base samples, variance-is-zero replacement switched on."""
    from sampling_gpmpc_amd.rollout import true_reachable_set_rollout
    Ns, H = 12, 9
    p = fs_params("params_pendulum1D_samples", Ns, H, feedback=False)
    p["agent"]["Dyn_gp_variance_is_zero"] = 4.0e-6
    agent, _ = make_agents(sg, p)
    u = synthetic_u_ff(1, H)
    z = torch.randn(H, Ns, 1, 3, dtype=F64, generator=torch.Generator().manual_seed(2))
    X, Y = true_reachable_set_rollout(agent, u, z=z, return_samples=True)
    erv = torch.zeros(H, 2, Ns, 1, 1, 3, dtype=F64)
    erv[:, 1, :, :, 0, :] = z
    oagent = ao.OracleAgent(p, ao.make_oracle_env(p), erv)
    Xo, Yo = ao.forward_sampling_rollout(oagent, u, return_samples=True)
    print(f"true-RS rollout rel err {relerr(X, Xo):.2e}")
    np.testing.assert_allclose(X, Xo, rtol=RTOL_TRAJ, atol=1e-9)


def test_sharded_rollout_single_rank_rccl(sg):
    """The N > 1 code path (shard_range + rollout on the slice + all-gather over RCCL) with a world of one rank."""
    import torch.distributed as dist
    from sampling_gpmpc_amd.distributed import sharded_forward_sampling_rollout
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    Ns, H = 64, 8
    p = fs_params("params_pendulum1D_samples", Ns, H)
    agent, _ = make_agents(sg, p)
    u_ff = synthetic_u_ff(1, H)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29531")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        tube = sharded_forward_sampling_rollout(agent, u_ff)
        # the pipelined form bench.py runs for N > 1: rollout r+1 on the launch stream, the all-gather of r on a side
        # stream, alternating buffers - five rollouts with different input sequences, every tube checked afterwards
        from sampling_gpmpc_amd.distributed import OverlappedTubeGather
        from sampling_gpmpc_amd.rollout import RolloutRunner
        erv = agent.epistimic_random_vector.to(agent.torch_device).contiguous()
        per = Ns * 3
        runners = [RolloutRunner(agent, u_ff * (1.0 + 0.1 * r), erv.reshape(-1)[per:], erv.shape[1] * per, H,
                                 sg._lib.MODE_RECONDITIONED, False) for r in range(5)]
        refs = []
        for rn in runners:
            refs.append(rn.launch().clone())
        torch.cuda.synchronize()
        for every in (1, 2, 3):                                  # one collective per rollout / per group of rollouts (last group partial)
            pipe = OverlappedTubeGather(Ns, agent.nx, H, every=every)
            tubes = []
            for r, rn in enumerate(runners):
                pipe.before_rollout(r)
                rn.launch(out=pipe.buffer(r))
                pipe.submit(r)
                if r >= 1:                                       # consume tube r-1 while rollout r / gather r are in flight
                    pipe.wait(r - 1)
                    tubes.append(pipe.tube(r - 1).clone())
            pipe.finish()
            tubes.append(pipe.tube(len(runners) - 1).clone())
            torch.cuda.synchronize()
            for r in range(len(runners)):
                assert torch.equal(tubes[r].reshape(refs[r].shape), refs[r]), (every, r)
    finally:
        dist.destroy_process_group()
    X = forward_sampling_rollout(agent, u_ff)
    np.testing.assert_array_equal(tube.cpu().numpy(), X)


def test_sharded_closed_loop_single_rank_rccl(sg):
    """The sharded closed-loop path (make_sharded_agent + min-distance filter reduced through RCCL + gather_jacobians)
    with a world of one rank equals the plain Agent, two SQP iterations."""
    import copy
    import torch.distributed as dist
    from sampling_gpmpc_amd.distributed import make_sharded_agent, gather_jacobians
    Ns, H = 6, 5
    p = load_params("params_pendulum1D_samples")
    p["common"]["use_cuda"] = True
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 2
    p["agent"]["Dyn_gp_min_data_dist"] = 0.02
    torch.manual_seed(9)
    plain = sg.Agent(copy.deepcopy(p), sg.make_env(p))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = "29537"
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        torch.manual_seed(9)
        sharded = make_sharded_agent(sg.Agent, copy.deepcopy(p), sg.make_env(p))
        assert sharded.dist_group is not None and sharded.shard == (0, Ns)
        assert torch.equal(sharded.epistimic_random_vector, plain.epistimic_random_vector)
        g = torch.Generator().manual_seed(5)
        x0 = np.array(p["env"]["start"], dtype=np.float64)
        for it in range(2):
            x_h = np.tile(x0, (H, Ns)) + 0.05 * torch.randn(H, Ns * plain.nx, generator=g, dtype=F64).numpy()
            u_h = 0.3 * torch.randn(H, Ns, plain.nu, generator=g, dtype=F64).numpy()
            outs = []
            for ag in (plain, sharded):
                ag.train_hallucinated_dynGP(it)
                outs.append(ag.dyn_fg_jacobians(ag.get_batch_x_hat_u_diff(x_h, u_h), it))
            full = gather_jacobians(outs[1], Ns)
            for a, b in zip(outs[0], full):
                np.testing.assert_array_equal(a, b)
            assert torch.equal(plain.Hallcinated_X_train, sharded.Hallcinated_X_train)
            np.testing.assert_array_equal(plain.Hallcinated_Y_train.cpu().numpy(), sharded.Hallcinated_Y_train.cpu().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("pname,Ns,H,nograd", [("params_pendulum1D_samples", 16, 12, False),
                                               ("params_car_residual_fs", 9, 10, False),
                                               ("params_car_residual_fs", 70, 9, True)])
def test_generic_kernels_agree_with_tuned_kernels(sg, pname, Ns, H, nograd, monkeypatch):
    """The generic rollout kernel (any T / n_r / horizon) and the tuned kernels (rollout_fast / rollout_indep) are two
    implementations of the same arithmetic: same inputs, results equal to round-off."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p = fs_params(pname, Ns, H, nograd=nograd, beta=(3.0 if (not nograd and "car" in pname) else None))
    agent, _ = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    lib = sg._lib.load()
    X_fast, Y_fast = forward_sampling_rollout(agent, u_ff, return_samples=True)
    # pendulum1D on the 4 x 9 grid with at most 88 appended rows: the one-chain MFMA kernel (path 4); car: rollout_fast (1)
    assert lib.gpmpc_debug_last_rollout_path() == (2 if nograd else (4 if "pendulum" in pname else 1)), "tuned kernel was not selected"
    monkeypatch.setenv("GPMPC_DISABLE_FAST_ROLLOUT", "1")
    agent2, _ = make_agents(sg, p, erv=agent.epistimic_random_vector.cpu().numpy())
    X_gen, Y_gen = forward_sampling_rollout(agent2, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 0, "generic kernel was not selected"
    po = fs_params(pname, Ns, H, nograd=nograd, beta=(3.0 if (not nograd and "car" in pname) else None))
    oagent = ao.OracleAgent(po, ao.make_oracle_env(po), agent.epistimic_random_vector.cpu())
    X_o = ao.forward_sampling_rollout(oagent, u_ff)
    print(f"{pname} Ns={Ns} H={H} nograd={nograd}: tuned vs generic max abs diff {np.abs(X_fast - X_gen).max():.2e}; "
          f"generic vs oracle rel err {relerr(X_gen, X_o):.2e}; tuned vs oracle {relerr(X_fast, X_o):.2e}")
    assert relerr(X_gen, X_o) < RTOL_TRAJ and relerr(X_fast, X_o) < RTOL_TRAJ
    np.testing.assert_allclose(X_fast, X_gen, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Y_fast, Y_gen, rtol=1e-7, atol=1e-11)


@pytest.mark.parametrize("pname,Ns,H,nograd", [("params_pendulum1D_samples", 12, 25, False),
                                               ("params_car_residual_fs", 5, 24, False),
                                               ("params_car_residual_fs", 150, 40, True),       # mode I, ragged workgroup
                                               ("params_pendulum1D_samples", 70, 20, True)])
def test_tuned_kernel_grid_root_vs_cholesky_root(sg, pname, Ns, H, nograd, monkeypatch):
    """The tuned kernel conditions on the real data through the plan's grid root W = D^-1/2 (Qa (x) Qb)^T (tensor-grid
    real inputs, separable kernel row) or, with GPMPC_DISABLE_GRID_ROOT=1, through L_rr^-1.  Both satisfy
    W^T W = (K_rr + s2 I)^-1, so trajectories and samples agree to round-off, and both match the oracle.  Mode I
    (nograd): rollout_indep_grid_kernel against the triangular rollout_indep_kernel."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    path = 2 if nograd else 1
    p = fs_params(pname, Ns, H, nograd=nograd, beta=(3.0 if (not nograd and "car" in pname) else None))
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    lib = sg._lib.load()
    X_grid, Y_grid = forward_sampling_rollout(agent, u_ff, return_samples=True)
    # (pendulum1D, mode R: the grid-root launch is the one-chain MFMA kernel, the Cholesky-root launch rollout_fast)
    assert lib.gpmpc_debug_last_rollout_path() == (4 if (not nograd and "pendulum" in pname) else path)
    assert agent._plan(use_grad=not nograd).desc.grid_n1 == 9, "the facade did not detect the reference's training grid"
    monkeypatch.setenv("GPMPC_DISABLE_GRID_ROOT", "1")
    agent2, _ = make_agents(sg, p, erv=agent.epistimic_random_vector.cpu().numpy())
    X_chol, Y_chol = forward_sampling_rollout(agent2, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == path
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    print(f"{pname} Ns={Ns} H={H}: grid root vs Cholesky root max abs diff X {np.abs(X_grid - X_chol).max():.2e} "
          f"Y {np.abs(Y_grid - Y_chol).max():.2e}; vs oracle {relerr(X_grid, Xo):.2e} / {relerr(X_chol, Xo):.2e}")
    assert np.abs(X_grid - X_chol).max() > 0.0, "the two roots produced bit-identical results: the knob is not wired"
    assert relerr(X_grid, Xo) < RTOL_TRAJ and relerr(X_chol, Xo) < RTOL_TRAJ
    np.testing.assert_allclose(X_grid, X_chol, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Y_grid, Y_chol, rtol=1e-7, atol=1e-11)
    np.testing.assert_allclose(Y_grid, Yo, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("pname,Ns,H", [
    ("params_pendulum1D_samples", 1, 2),        # a single sample, the shortest horizon that appends (n_h max 3)
    ("params_pendulum1D_samples", 5, 43),       # longest horizon of the tuned kernel (n_h max 126 of 128)
    ("params_pendulum1D_samples", 3, 45),       # beyond it: generic kernel, 4 rows per lane (n_h max 132)
    ("params_car_residual_fs", 2, 3),
    ("params_car_residual_fs", 1025, 2),        # many workgroups, tiny horizon
])
def test_rollout_edge_sizes(sg, pname, Ns, H):
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p = fs_params(pname, Ns, H, nograd=False, beta=(3.0 if "car" in pname else None))
    if Ns > 64:
        p["agent"]["base_sample_generator"] = "vectorized"
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    X, Y = forward_sampling_rollout(agent, u_ff, return_samples=True)
    path = sg._lib.load().gpmpc_debug_last_rollout_path()
    if Ns > 64:                                    # oracle on a subset (it is Ns-tiled and from scratch)
        sel = slice(Ns - 24, Ns)
        po = fs_params(pname, 24, H, nograd=False, beta=(3.0 if "car" in pname else None))
        oagent = ao.OracleAgent(po, ao.make_oracle_env(po), agent.epistimic_random_vector[:, :, sel].cpu())
        X, Y = X[sel], Y[sel]
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    print(f"{pname} Ns={Ns} H={H}: kernel path {path}, rel err X {relerr(X, Xo):.2e} Y {relerr(Y, Yo):.2e}")
    chains = Ns * agent.g_ny
    tiled = chains > (1024 if agent.g_ny == 1 else 768)                  # the one-chain kernel would need a second round of the chip
    one = agent.g_ny == 1 and 3 * (H - 1) <= 88 and Ns <= 2048          # rollout_one_kernel: pendulum1D 4 x 9, H <= 30
    assert path == (0 if H > 43 else (4 if one else (3 if tiled else 1)))
    assert relerr(X, Xo) < RTOL_TRAJ
    np.testing.assert_allclose(Y, Yo, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("pname", ["params_pendulum1D_samples", "params_car_residual"])
def test_derivative_observing_real_data(sg, pname):
    """env.train_data_has_derivatives: True - the real labels observe value AND gradient (n_r = N_r*T slots): plan,
    joint draw and re-conditioned rollout (generic kernel) against the oracle."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    Ns, H = 6, 5
    p = load_params(pname)
    p["env"]["train_data_has_derivatives"] = True
    p["agent"]["true_dyn_as_sample"] = False
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 1
    if "car" in pname:
        p["agent"]["Dyn_gp_jitter"] = 1e-9
    agent, oagent = make_agents(sg, p)
    assert agent._plan(True).real_has_grad and agent._plan(True).n_r == agent.Dyn_gp_X_train.shape[0] * 3
    g = torch.Generator().manual_seed(4)
    x_h = np.tile(np.array(p["env"]["start"]), (H, Ns)) + 0.05 * torch.randn(H, Ns * agent.nx, generator=g, dtype=F64).numpy()
    u_h = 0.2 * torch.randn(H, Ns, agent.nu, generator=g, dtype=F64).numpy()
    agent.train_hallucinated_dynGP(0)
    oagent.train_hallucinated_dynGP(0)
    gp_val, y_grad, u_grad = agent.dyn_fg_jacobians(agent.get_batch_x_hat_u_diff(x_h, u_h), 0)
    ogp_val, oy_grad, ou_grad = oagent.dyn_fg_jacobians(oagent.get_batch_x_hat_u_diff(x_h, u_h), 0)
    np.testing.assert_allclose(agent.model_i_call.mean.cpu().numpy(), oagent.model_i_call.mean.numpy(), rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(agent.model_i_call.variance.cpu().numpy(), oagent.model_i_call.variance.numpy(),
                               rtol=1e-3, atol=1e-13)
    lvl = (agent.model_i_call.last_info.cpu().numpy() >> 1) & 7                     # (Ns, g_ny): per GP task
    ojit = oagent.model_i_call.root_info.jitter_added.numpy()
    same_task = (lvl > 0) == (ojit > 0)
    assert same_task.any()
    # with gradient labels on the grid the posterior is nearly degenerate (variances at the jitter level), so the
    # samples carry O(sqrt(jitter)) branch/round-off noise; mean, variance above are the sharp checks.  Whether a task's
    # Cholesky needs the jitter is decided by round-off, and it comes out differently with the host's BLAS: a state row
    # (f + B_d g) is compared where every task it takes from B_d took the same branch on both sides
    uses = oagent.env_model.B_d.numpy() != 0                                         # (nx, g_ny)
    same = (same_task[:, None, :] | ~uses[None]).all(axis=2)                         # (Ns, nx)
    print(f"{pname}: derivative data, max |gp_val - oracle| = {np.abs(gp_val[same] - ogp_val[same]).max():.2e}")
    np.testing.assert_allclose(gp_val[same], ogp_val[same], rtol=1e-5, atol=2e-4)
    # rollout with the same data (forward-sampling layout)
    pf = fs_params(pname if "pendulum" in pname else "params_car_residual_fs", Ns, 6, nograd=False,
                   beta=(3.0 if "car" in pname else None))
    pf["env"]["train_data_has_derivatives"] = True
    agent, oagent = make_agents(sg, pf)
    u_ff = synthetic_u_ff(agent.nu, 6)
    X = forward_sampling_rollout(agent, u_ff)
    assert sg._lib.load().gpmpc_debug_last_rollout_path() == 0
    Xo = ao.forward_sampling_rollout(oagent, u_ff)
    print(f"{pname} derivative-observing real data: rollout rel err {relerr(X, Xo):.2e}")
    assert relerr(X, Xo) < RTOL_TRAJ


def test_value_only_appended_labels(sg):
    """hall_tasks = 1: the appended points observe task 0 only (reference src/agent.py:402, the forward-sampling data
    of prepare_dynamics_set).  Oracle: the same loop with the gradient labels NaN-ed before the dataset update."""
    from sampling_gpmpc_amd.rollout import rollout_device
    from sampling_gpmpc_amd import _lib
    Ns, H = 7, 8
    p = fs_params("params_pendulum1D_samples", Ns, H)
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(1, H)
    erv = agent.epistimic_random_vector
    per = Ns * 3
    res = rollout_device(agent, u_ff, erv.reshape(-1)[per:], erv.shape[1] * per, H=H, mode=_lib.MODE_RECONDITIONED,
                         use_model_without_derivatives=False, hall_tasks=1)
    assert sg._lib.load().gpmpc_debug_last_rollout_path() == 0
    X = res.X_traj.cpu().numpy()
    try:                                                          # the tiled kernel's dead-row form of the same call
        sg._lib.load().gpmpc_rollout_pin_kernel(_lib.KERNEL_TILES)
        res_t = rollout_device(agent, u_ff, erv.reshape(-1)[per:], erv.shape[1] * per, H=H, mode=_lib.MODE_RECONDITIONED,
                               use_model_without_derivatives=False, hall_tasks=1)
        assert sg._lib.load().gpmpc_debug_last_rollout_path() == 3
    finally:
        sg._lib.load().gpmpc_rollout_pin_kernel(-1)
    assert relerr(res_t.X_traj.cpu().numpy(), X) < 1e-9 and relerr(res_t.Y.cpu().numpy(), res.Y.cpu().numpy()) < 1e-7
    # oracle loop (forward_sampling_rollout of oracle/agent_oracle.py with the label masking inserted)
    K = np.array(p["optimizer"]["terminal_tightening"]["K"])
    x_equi = np.array(p["env"]["goal_state"])
    x_h = np.tile(np.array(p["env"]["start"], dtype=np.float64), (1, Ns))
    Xo = np.empty((Ns, 2, H + 1))
    orig_update = oagent.update_hallucinated_Dyn_dataset
    def masked_update(newX, newY):
        newY = newY.clone()
        newY[..., 1:] = float("nan")
        orig_update(newX, newY)
    oagent.update_hallucinated_Dyn_dataset = masked_update
    for t in range(H):
        oagent.train_hallucinated_dynGP(1)
        oagent.mpc_iteration(t)
        bx = oagent.get_batch_x_hat_u_diff(x_h, -(x_equi - x_h.reshape(1, Ns, -1)) @ K.T + np.tile(u_ff[t].reshape(1, 1, -1), (Ns, 1)))
        gp_val, _, _ = oagent.dyn_fg_jacobians(bx, 1)
        Xo[:, :, t] = bx[:, 0, 0, :2].numpy()
        x_h = gp_val[:, :, 0, 0].reshape(1, -1)
    Xo[:, :, H] = gp_val[:, :, 0, 0]
    print(f"value-only appended labels: rel err {relerr(X, Xo):.2e}")
    assert relerr(X, Xo) < RTOL_TRAJ


def _clamped_base_samples(p, H, seed):
    g = torch.Generator().manual_seed(seed)
    ag = p["agent"]
    T = 1 if p["env"]["use_model_without_derivatives"] else 1 + ag["g_dim"]["nx"] + ag["g_dim"]["nu"]
    return torch.randn(H, 2, ag["num_dyn_samples"], ag["g_dim"]["ny"], 1, T, generator=g, dtype=F64).clamp(-2.0, 2.0)


@pytest.mark.parametrize("pname,nograd", [("params_pendulum1D_samples", False), ("params_car_residual_fs", False),
                                          ("params_car_residual_fs", True)])
def test_stepwise_harness_equals_fused_rollout(sg, pname, nograd):
    """The per-step Agent call sequence (gpmpc_joint_sample + gpmpc_assemble_jacobians per step, the reference's loop
    structure) and the one-launch fused rollout are the same computation."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout, forward_sampling_stepwise
    Ns, H = 16, 8
    p = fs_params(pname, Ns, H, nograd=nograd, beta=(3.0 if (not nograd and "car" in pname) else None))
    erv = _clamped_base_samples(p, H, 11)
    a_fused, _ = make_agents(sg, p, erv=erv)
    a_step, _ = make_agents(sg, p, erv=erv)
    u_ff = synthetic_u_ff(a_fused.nu, H)
    Xf, Yf = forward_sampling_rollout(a_fused, u_ff, return_samples=True)
    Xs, Ys = forward_sampling_stepwise(a_step, u_ff, return_samples=True)
    print(f"{pname} nograd={nograd}: stepwise vs fused max abs diff X {np.abs(Xf - Xs).max():.2e} Y {np.abs(Yf - Ys).max():.2e}")
    np.testing.assert_allclose(Xs, Xf, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(Ys, Yf, rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(a_step.Hallcinated_X_train.cpu().numpy(), a_fused.Hallcinated_X_train.cpu().numpy(),
                               rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("pname,min_dist", [("params_pendulum1D_samples", 0.25), ("params_car_residual_fs", 0.05)])
def test_forward_sampling_with_min_data_dist(sg, pname, min_dist):
    """Dyn_gp_min_data_dist >= 0 (off in the shipped YAMLs): appended points too close to existing data get NaN labels
    per sample, points filtered in all samples are dropped, draws too close to an observed label are overwritten
    (reference src/agent.py:164-202, 666-698).  forward_sampling_rollout routes to the per-step harness for it."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout, fused_rollout_supported
    Ns, H = 12, 8
    p = fs_params(pname, Ns, H, nograd=False, beta=(3.0 if "car" in pname else None))
    p["agent"]["Dyn_gp_min_data_dist"] = min_dist
    agent, oagent = make_agents(sg, p, erv=_clamped_base_samples(p, H, 3))
    assert not fused_rollout_supported(agent)
    u_ff = synthetic_u_ff(agent.nu, H)
    X, Y = forward_sampling_rollout(agent, u_ff, return_samples=True)
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    hy, hyo = agent.Hallcinated_Y_train.cpu().numpy(), oagent.Hallcinated_Y_train.numpy()
    assert hy.shape == hyo.shape and hy.shape[2] < H, "the filter must have dropped points in this case"
    nan, nano = np.isnan(hy), np.isnan(hyo)
    assert nan.any() and (nan == nano).all(), "per-sample NaN-labelled points differ"
    print(f"{pname} min_dist={min_dist}: kept {hy.shape[2]}/{H} points, {nan[..., 0].mean():.0%} NaN-labelled; "
          f"rel err X {relerr(X, Xo):.2e}")
    np.testing.assert_allclose(X, Xo, rtol=RTOL_TRAJ, atol=1e-9)
    np.testing.assert_allclose(Y, Yo, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(hy[~nan], hyo[~nano], rtol=1e-5, atol=1e-9)


@pytest.fixture
def pin_tiles_if(sg):
    """fused == "tiles": the fused launch pinned to the tiled kernel (the size heuristic takes it from 256 chains on)"""
    lib = sg._lib.load()
    def pin(fused):
        if fused == "tiles":
            lib.gpmpc_rollout_pin_kernel(sg._lib.KERNEL_TILES)
    yield pin
    lib.gpmpc_rollout_pin_kernel(-1)


@pytest.mark.parametrize("fused", [True, False, "tiles"])
def test_prepare_dynamics_set_against_oracle(sg, fused, pin_tiles_if):
    """Forward sampling with rejection (reference src/agent.py:331-443): the GP is re-trained on real + forward-sampled
    (value-only labels) + hallucinated data at every step, samples leaving the tube are rejected and their
    hallucinated data replaced by survivors'.  Same base samples and the same RandomState on both sides.
    fused: steps 2.. in ONE gpmpc_rollout_seeded launch (hallucinated points as seeds, value-only draws appended);
    otherwise one gpmpc_joint_sample per step."""
    Ns, H = 10, 6
    p = load_params("params_pendulum1D_samples")
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = Ns, H
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 2
    agent, oagent = make_agents(sg, p)
    nx, nu = agent.nx, agent.nu
    g = torch.Generator().manual_seed(21)
    x0 = np.array(p["env"]["start"], dtype=np.float64)
    # one SQP iteration of joint draws so that both agents carry hallucinated data (copied from the oracle)
    x_h = np.tile(x0, (H, Ns)) + 0.05 * torch.randn(H, Ns * nx, generator=g, dtype=F64).numpy()
    u_h = 0.3 * torch.randn(H, Ns, nu, generator=g, dtype=F64).numpy()
    for ag in (agent, oagent):
        ag.train_hallucinated_dynGP(0)
    oagent.dyn_fg_jacobians(oagent.get_batch_x_hat_u_diff(x_h, u_h), 0)
    agent.Hallcinated_X_train = oagent.Hallcinated_X_train.clone().to(agent.torch_device)
    agent.Hallcinated_Y_train = oagent.Hallcinated_Y_train.clone().to(agent.torch_device)
    for ag in (agent, oagent):
        ag.train_hallucinated_dynGP(1)
    U_soln = 0.5 * torch.randn(H + 1, nu, generator=g, dtype=F64)
    X_kp1 = torch.tensor(x0[:nx]).reshape(nx, 1)
    z = [torch.randn(Ns, 1, 1, 3, generator=g, dtype=F64).clamp(-2, 2) for _ in range(H)]
    X_soln = torch.zeros(H + 1, Ns * nx, dtype=F64)
    X_soln[1] = torch.tensor(x0[:nx]).repeat(Ns)
    for ag in (agent, oagent):
        ag.ci_list = [1e9] * (H + 1)
    # step 1: everything survives (huge tube); now tighten the tube of step 2 around the median sampled state
    pin_tiles_if(fused)
    tiles, fused = fused == "tiles", bool(fused)
    agent.prepare_dynamics_set(X_soln.clone(), U_soln, X_kp1, base_samples=z, rng=np.random.RandomState(5), fused=fused)
    if tiles:
        assert sg._lib.load().gpmpc_debug_last_rollout_path() == 3, "the fused launch did not run the tiled kernel"
    oagent.prepare_dynamics_set(X_soln.clone(), U_soln, X_kp1, base_samples=z, rng=np.random.RandomState(5))
    np.testing.assert_allclose(agent.FS_X_train_batch.cpu().numpy(), oagent.FS_X_train_batch.numpy(), rtol=1e-8, atol=1e-10)
    fy, fyo = agent.FS_Y_train_batch.cpu().numpy(), oagent.FS_Y_train_batch.numpy()
    assert fy.shape == fyo.shape == (Ns, 1, H - 2, 3) and (np.isnan(fy) == np.isnan(fyo)).all() and np.isnan(fy[..., 1:]).all()
    np.testing.assert_allclose(fy[..., 0], fyo[..., 0], rtol=1e-6, atol=1e-9)
    for a_, b_ in zip(agent.rejection_trace, oagent.rejection_trace):
        assert (a_.cpu().numpy() == b_.numpy()).all()
    print(f"prepare_dynamics_set: FS points {fy.shape[2]}, survivors per step {[int(t.sum()) for t in oagent.rejection_trace]}, "
          f"max |dY| {np.nanmax(np.abs(fy - fyo)):.2e}")
    # second call with a tube around the sampled states of step 2: part of the samples is rejected and replaced
    x2 = oagent.FS_X_train_batch[:, 0, 2, 0]                     # theta after two sampled steps (the first differing one)
    med = float(x2.median())
    tol = float((x2 - med).abs().median()) + 1e-12
    X_soln2 = X_soln.clone()
    X_soln2[3] = torch.stack([torch.full((Ns,), med, dtype=F64), torch.zeros(Ns, dtype=F64)], dim=1).reshape(-1)
    for ag, dev in ((agent, agent.torch_device), (oagent, "cpu")):
        ag.ci_list = [1e9] * (H + 1)
        ag.ci_list[2] = torch.tensor([tol, 1e9], dtype=F64, device=dev)      # tube on theta only at that step
        ag.train_hallucinated_dynGP(1)
    hx_before = oagent.Hallcinated_X_train.clone()
    agent.prepare_dynamics_set(X_soln2.clone(), U_soln, X_kp1, base_samples=z, rng=np.random.RandomState(7), fused=fused)
    if tiles:
        assert sg._lib.load().gpmpc_debug_last_rollout_path() == 3
    oagent.prepare_dynamics_set(X_soln2.clone(), U_soln, X_kp1, base_samples=z, rng=np.random.RandomState(7))
    left = oagent.rejection_trace[-1].numpy()
    assert 0 < left.sum() < Ns, f"the tube should split the samples, survivors: {left}"
    assert (agent.rejection_trace[-1].cpu().numpy() == left).all()
    np.testing.assert_allclose(agent.Hallcinated_X_train.cpu().numpy(), oagent.Hallcinated_X_train.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(agent.Hallcinated_Y_train.cpu().numpy(), oagent.Hallcinated_Y_train.numpy(), rtol=1e-9, atol=1e-12)
    assert not np.array_equal(oagent.Hallcinated_X_train.numpy(), hx_before.numpy()), "rejected samples keep their data"


@pytest.mark.gpu
@pytest.mark.parametrize("pname,Ns,H", [("params_car_residual_fs", 200, 40), ("params_pendulum1D_samples", 130, 30)])
def test_mode_i_exp_recurrence_vs_direct_exponentials(sg, pname, Ns, H, monkeypatch):
    """Mode I on the equispaced training grid: the kernel factors come from the recurrence E_0 rho^k G_k (two
    exponentials per axis, constants in the plan's mode-I table) or, with GPMPC_DISABLE_EXP_RECURRENCE=1 (the plan then
    marks the axes "not equispaced"), from one exponential per axis point.  Same arithmetic up to round-off; both match
    the oracle."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p = fs_params(pname, Ns, H, nograd=True)
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    lib = sg._lib.load()
    X_rec, Y_rec = forward_sampling_rollout(agent, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 2
    monkeypatch.setenv("GPMPC_DISABLE_EXP_RECURRENCE", "1")
    agent2, _ = make_agents(sg, p, erv=agent.epistimic_random_vector.cpu().numpy())
    X_dir, Y_dir = forward_sampling_rollout(agent2, u_ff, return_samples=True)
    assert lib.gpmpc_debug_last_rollout_path() == 2
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    print(f"{pname} Ns={Ns} H={H}: recurrence vs direct max abs diff X {np.abs(X_rec - X_dir).max():.2e} "
          f"Y {np.abs(Y_rec - Y_dir).max():.2e}; vs oracle {relerr(X_rec, Xo):.2e} / {relerr(X_dir, Xo):.2e}")
    assert np.abs(Y_rec - Y_dir).max() > 0.0, "bit-identical results: the knob is not wired"
    assert relerr(X_rec, Xo) < RTOL_TRAJ and relerr(X_dir, Xo) < RTOL_TRAJ
    np.testing.assert_allclose(X_rec, X_dir, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(Y_rec, Y_dir, rtol=1e-7, atol=1e-11)
    np.testing.assert_allclose(Y_rec, Yo, rtol=1e-4, atol=1e-8)





def test_joint_row_limit_is_reported_up_front(sg):
    """More label rows per chain than the joint kernels are instantiated for (2048): a clear error before any launch
    (the reference's max_sqp_iter = 150 would need 22 500 rows at the shipped car horizon)."""
    p = load_params("params_pendulum1D_samples")
    p["agent"]["num_dyn_samples"], p["optimizer"]["H"] = 2, 10
    p["common"]["num_MPC_itrs"], p["optimizer"]["SEMPC"]["max_sqp_iter"] = 1, 1
    agent, _ = make_agents(sg, p)
    agent.train_hallucinated_dynGP(0)
    dev = agent.torch_device
    agent.Hallcinated_X_train = torch.rand(2, 1, 700, 2, dtype=F64, device=dev)
    agent.Hallcinated_Y_train = torch.rand(2, 1, 700, 3, dtype=F64, device=dev)
    agent.train_hallucinated_dynGP(1)
    x = torch.rand(2, 1, 10, 2, dtype=F64, device=dev)
    with pytest.raises(sg._lib.GpmpcError, match="2048 rows"):
        agent.model_i(x).mean


def test_second_fused_rollout_conditions_on_existing_points(sg):
    """reference simulate_forward_sampling_car.py:118 calls train_hallucinated_dynGP(1), which never resets: a second
    rollout on the same agent conditions on the first one's points.  The fused call must not silently start from the
    real data only: it is routed through the per-step harness."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    p = fs_params("params_pendulum1D_samples", 5, 6, nograd=False)
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(1, 6)
    X1 = forward_sampling_rollout(agent, u_ff)
    Xo1 = ao.forward_sampling_rollout(oagent, u_ff)
    assert relerr(X1, Xo1) < RTOL_TRAJ
    assert agent.Hallcinated_X_train.shape[2] == 6
    X2 = forward_sampling_rollout(agent, u_ff)                    # conditions on the 6 points of the first rollout
    Xo2 = ao.forward_sampling_rollout(oagent, u_ff)
    print(f"second rollout on the same agent: rel err {relerr(X2, Xo2):.2e}; differs from the first by {relerr(X2, X1):.2e}")
    assert relerr(X2, Xo2) < RTOL_TRAJ
    assert relerr(X2, X1) > 1e-6
    assert agent.Hallcinated_X_train.shape[2] == 12


@pytest.mark.parametrize("pname", ["params_pendulum1D_samples", "params_car_residual_fs"])
def test_seeded_rollout_on_the_tiled_kernel(sg, pname):
    """a seeded call (no kept factor state) runs the tiled FP64-MFMA kernel - the seed points are
    conditioning-only passes of its step body.  Second and third rollout on the same Agent (reference
    simulate_forward_sampling_car.py:118: train_hallucinated_dynGP(1) never resets) against the oracle and against the generic
    kernel, path asserted; the un-pinned dispatcher takes the tiled kernel from 256 chains on."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout
    lib = sg._lib.load()
    H = 7
    p = fs_params(pname, 6, H, nograd=False, beta=(3.0 if "car" in pname else None))
    u_ff = synthetic_u_ff(2 if "car" in pname else 1, H)
    X = {}
    for kern in (sg._lib.KERNEL_TILES, sg._lib.KERNEL_GENERIC):
        agent, oagent = make_agents(sg, p)
        try:
            lib.gpmpc_rollout_pin_kernel(kern)
            runs = []
            for rep in range(3):                                  # 0, 7 and 14 seed points (21 rows per rollout)
                runs.append(forward_sampling_rollout(agent, u_ff))
                assert lib.gpmpc_debug_last_rollout_path() == (3 if kern == sg._lib.KERNEL_TILES else 0), (kern, rep)
        finally:
            lib.gpmpc_rollout_pin_kernel(-1)
        X[kern] = runs
        if kern == sg._lib.KERNEL_TILES:
            for rep in range(3):
                Xo = ao.forward_sampling_rollout(oagent, u_ff)
                print(f"{pname} tiled kernel, rollout {rep} on the same agent ({7 * rep} seed points): rel err {relerr(runs[rep], Xo):.2e}")
                assert relerr(runs[rep], Xo) < RTOL_TRAJ
            assert agent.Hallcinated_X_train.shape[2] == 3 * H
    for rep in range(3):
        assert relerr(X[sg._lib.KERNEL_TILES][rep], X[sg._lib.KERNEL_GENERIC][rep]) < 1e-9
    # the dispatcher by itself: 256 chains and more take the tiled kernel for a seeded call
    plan = agent._plan(use_grad=True)
    Ns_big = 256 if "pendulum" in pname else 96
    pb = fs_params(pname, Ns_big, 5, nograd=False, beta=(3.0 if "car" in pname else None))
    big, _ = make_agents(sg, pb)
    ub = synthetic_u_ff(2 if "car" in pname else 1, 5)
    forward_sampling_rollout(big, ub)
    X2 = forward_sampling_rollout(big, ub)
    assert lib.gpmpc_debug_last_rollout_path() == 3 and np.isfinite(X2).all()


def test_value_only_seeded_rollout_on_the_tiled_kernel(sg):
    """hall_tasks = 1 behind seed points (the fused prepare_dynamics_set's launch, reference src/agent.py:399-405): the tiled
    kernel keeps three row slots per point and leaves the derivative rows of a value-only point dead (identity rows, zero
    right-hand sides).  Same call on the generic kernel (one row per value-only point) must agree to round-off."""
    from sampling_gpmpc_amd.rollout import rollout_device
    from sampling_gpmpc_amd import _lib
    lib = _lib.load()
    Ns, H = 9, 6
    p = fs_params("params_pendulum1D_samples", Ns, H, nograd=False)
    agent, _ = make_agents(sg, p)
    dev = agent.torch_device
    g = torch.Generator().manual_seed(3)
    n0, nv = 5, 2
    Xs = (torch.tensor([0.3, 0.1], dtype=F64) + 0.4 * torch.randn(Ns, 1, n0, 2, generator=g, dtype=F64)).to(dev)
    Ys = (0.2 * torch.randn(Ns, 1, n0, 3, generator=g, dtype=F64)).to(dev)
    Xv = (torch.tensor([0.2, -0.1], dtype=F64) + 0.4 * torch.randn(Ns, 1, nv, 2, generator=g, dtype=F64)).to(dev)
    Yv = (0.2 * torch.randn(Ns, 1, nv, 3, generator=g, dtype=F64)).to(dev)
    z = torch.randn(H, Ns * 3, generator=g, dtype=F64).clamp(-2, 2).to(dev)
    u_ff = synthetic_u_ff(1, H)
    out = {}
    for kern in (_lib.KERNEL_TILES, _lib.KERNEL_GENERIC):
        try:
            lib.gpmpc_rollout_pin_kernel(kern)
            for ht, vs in ((1, (Xv, Yv)), (3, (Xv, Yv)), (1, None)):
                res = rollout_device(agent, u_ff, z.reshape(-1), z.shape[1], H=H, mode=_lib.MODE_RECONDITIONED,
                                     use_model_without_derivatives=False, hall_tasks=ht, seeds=(Xs, Ys), value_seeds=vs)
                assert lib.gpmpc_debug_last_rollout_path() == (3 if kern == _lib.KERNEL_TILES else 0)
                assert int(res.info.max().item()) & ~_lib.INFO_VAR_CLAMPED == 0
                out[(kern, ht, vs is None)] = (res.X_traj.cpu().numpy(), res.Y.cpu().numpy())
        finally:
            lib.gpmpc_rollout_pin_kernel(-1)
    for key in [(1, False), (3, False), (1, True)]:
        Xt, Yt = out[(_lib.KERNEL_TILES,) + key]
        Xg, Yg = out[(_lib.KERNEL_GENERIC,) + key]
        print(f"hall_tasks={key[0]} value seeds={not key[1]}: tiled vs generic rel err X {relerr(Xt, Xg):.2e}, Y {relerr(Yt, Yg):.2e}")
        assert relerr(Xt, Xg) < 1e-9 and relerr(Yt, Yg) < 1e-7
    # value-only conditioning differs from conditioning on all tasks
    assert relerr(out[(_lib.KERNEL_TILES, 1, False)][0], out[(_lib.KERNEL_TILES, 3, False)][0]) > 1e-6
    # a one-step horizon behind the seeds (prepare_dynamics_set with n_last = 2): nothing is appended by the rollout itself
    one = {}
    for kern in (_lib.KERNEL_TILES, _lib.KERNEL_GENERIC):
        try:
            lib.gpmpc_rollout_pin_kernel(kern)
            res = rollout_device(agent, u_ff[:1], z[:1].reshape(-1), z.shape[1], H=1, mode=_lib.MODE_RECONDITIONED,
                                 use_model_without_derivatives=False, hall_tasks=1, seeds=(Xs, Ys), value_seeds=(Xv, Yv))
            assert lib.gpmpc_debug_last_rollout_path() == (3 if kern == _lib.KERNEL_TILES else 0)
            one[kern] = (res.X_traj.cpu().numpy(), res.Y.cpu().numpy())
        finally:
            lib.gpmpc_rollout_pin_kernel(-1)
    assert relerr(one[_lib.KERNEL_TILES][0], one[_lib.KERNEL_GENERIC][0]) < 1e-9
    assert relerr(one[_lib.KERNEL_TILES][1], one[_lib.KERNEL_GENERIC][1]) < 1e-7


def test_seeded_rollout_with_more_than_200_seed_slots(sg):
    """a seeded rollout's factor covers the seed slots too (here 70 points x 3 tasks = 210 + 3 x 11 appended:
    far beyond what stays in LDS), so its workspace comes from gpmpc_rollout_seeded_workspace_bytes - the un-seeded query
    (3 x 11 slots) would be too small and the call would fail with GPMPC_E_WORKSPACE."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout, seeds_fit
    H1, H2 = 70, 12
    p = fs_params("params_pendulum1D_samples", 4, H1, nograd=False)
    agent, oagent = make_agents(sg, p)
    X1 = forward_sampling_rollout(agent, synthetic_u_ff(1, H1))
    Xo1 = ao.forward_sampling_rollout(oagent, synthetic_u_ff(1, H1))
    assert relerr(X1, Xo1) < RTOL_TRAJ and agent.Hallcinated_X_train.shape[2] == H1
    assert seeds_fit(agent, H1, 0, H2, 3, 3)
    lib = sg._lib.load()
    plan = agent._plan(use_grad=True)
    small = lib.gpmpc_rollout_workspace_bytes(plan.desc, sg._lib.MODE_RECONDITIONED, 3, 4, H2)
    need = lib.gpmpc_rollout_seeded_workspace_bytes(plan.desc, sg._lib.MODE_RECONDITIONED, 3, 4, H2, H1, 0)
    assert need > small
    agent._ws_cache.pop("rollout", None)                          # force a fresh, exactly sized workspace
    u2 = synthetic_u_ff(1, H2)
    X2 = forward_sampling_rollout(agent, u2)                      # seeded: conditions on the 70 points of the first rollout
    assert lib.gpmpc_debug_last_rollout_path() == 0
    Xo2 = ao.forward_sampling_rollout(oagent, u2)
    print(f"seeded rollout on 210 seed slots: rel err {relerr(X2, Xo2):.2e}")
    assert relerr(X2, Xo2) < RTOL_TRAJ and agent.Hallcinated_X_train.shape[2] == H1 + H2


@pytest.mark.parametrize("pname", ["params_pendulum1D_samples", "params_car_residual_fs"])
def test_rollout_factor_state_export_and_resume(sg, pname):
    """SURVEY.md 8b "final factor state": a rollout keeps its chains' factor (gpmpc_rollout_seeded, state), a second call
    resumes from it - the two tubes together equal ONE rollout over the whole horizon (oracle), nothing is re-factorised."""
    from sampling_gpmpc_amd.rollout import RolloutState, rollout_device
    Ns, H1, H2 = 5, 6, 4
    H = H1 + H2
    p = fs_params(pname, Ns, H, nograd=False, beta=(3.0 if "car" in pname else None))
    agent, oagent = make_agents(sg, p)
    u_ff = synthetic_u_ff(agent.nu, H)
    Xo, Yo = ao.forward_sampling_rollout(oagent, u_ff, return_samples=True)
    erv = agent.epistimic_random_vector.to(agent.torch_device).contiguous()
    T = 3
    per = Ns * agent.g_ny * T
    z = erv.reshape(-1)[per:]
    stride = erv.shape[1] * per
    state = RolloutState(agent, slots=T * H, points=H)
    r1 = rollout_device(agent, u_ff[:H1], z, stride, H=H1, mode=sg._lib.MODE_RECONDITIONED,
                        use_model_without_derivatives=False, state=state)
    assert state.counts() == (0, H1)                               # the last draw is in the factor too
    x_mid = r1.X_traj[:, :, H1].contiguous()
    r2 = rollout_device(agent, u_ff[H1:], z[H1 * stride:], stride, H=H2, mode=sg._lib.MODE_RECONDITIONED,
                        use_model_without_derivatives=False, x0=x_mid, state=state, resume=True)
    assert state.counts() == (0, H)
    X = torch.cat([r1.X_traj, r2.X_traj[:, :, 1:]], dim=2).cpu().numpy()
    Y = torch.cat([r1.Y, r2.Y], dim=2).cpu().numpy()
    print(f"{pname}: resumed rollout vs one {H}-step rollout: rel err X {relerr(X, Xo):.2e}, Y {relerr(Y, Yo):.2e}")
    assert relerr(X, Xo) < RTOL_TRAJ
    np.testing.assert_allclose(Y, Yo, rtol=1e-4, atol=1e-8)
    assert not int(r2.info.max().item()) & sg._lib.INFO_STATE_FULL
    # a third call has no room left: the draw is still produced, the info bit says the factor was not extended
    r3 = rollout_device(agent, u_ff[:1], z, stride, H=1, mode=sg._lib.MODE_RECONDITIONED,
                        use_model_without_derivatives=False, x0=x_mid, state=state, resume=True)
    assert int(r3.info.max().item()) & sg._lib.INFO_STATE_FULL and torch.isfinite(r3.X_traj).all()


@pytest.mark.parametrize("fused", [True, False, "tiles"])
def test_prepare_dynamics_set_against_reference_run(sg, fused, pin_tiles_if):
    """The HIP Agent against the reference's REAL ``Agent.prepare_dynamics_set`` (src/agent.py:331-443; golden captured by
    make_goldens.py under the gpytorch stub): forward-sampled points, value-only labels, the rejection trace (survivor
    counts), survivor replacement of the hallucinated tensors, for a tube nobody leaves and one that splits the samples."""
    from tests.test_oracle_golden import _pds_params, replay_prepare_dynamics_set
    d = np.load(os.path.join(GOLDEN, "agent_e2e_prepare_dynamics_set_pendulum1D.npz"))
    p = _pds_params(d)
    agent, _ = make_agents(sg, p, erv=d["epistimic_random_vector"])
    pin_tiles_if(fused)
    replay_prepare_dynamics_set(agent, d, to_dev=lambda t: t.to(agent.torch_device), joint_draw_exact=False, fused=bool(fused))
    if fused == "tiles":
        assert sg._lib.load().gpmpc_debug_last_rollout_path() == 3, "the fused launch did not run the tiled kernel"


def test_pinned_sample_branches_against_reference_run(sg):
    """true_dyn_as_sample / mean_as_dyn_sample and their Ns = 1 / Ns = 2 short-circuits (src/agent.py:582-624) on the HIP
    Agent against the reference-run golden: value / Jacobian arrays, the hallucinated tensors, the posterior mean."""
    from tests.test_oracle_golden import pinned_cases, replay_pinned
    d = np.load(os.path.join(GOLDEN, "agent_e2e_pinned_samples.npz"))
    for tag, p, c in pinned_cases(d):
        agent, _ = make_agents(sg, p, erv=c["epistimic_random_vector"])
        replay_pinned(agent, c, to_dev=lambda t: t.to(agent.torch_device), drawn_exact=False)
        print(f"pinned-sample case {tag}: ok")


@pytest.mark.parametrize("mode", ["block", "poll"])
def test_to_host_waits_for_its_copy_in_both_wait_modes(sg, mode, monkeypatch):
    """_lib.to_host: the pinned D2H copy is asynchronous and nothing blocking follows it - it must be complete when the array
    is handed out, also under GPMPC_HOST_WAIT=block where host_wait() returns at once."""
    monkeypatch.setenv("GPMPC_HOST_WAIT", mode)
    dev = torch.device("cuda")
    for rep in range(20):
        a_ = torch.full((4096, 257), float(rep), dtype=F64, device=dev)
        b_ = (a_ * 2.0 + 1.0).cumsum(0)                    # some queued work in front of the copy
        h = sg._lib.to_host(b_)
        np.testing.assert_array_equal(h, b_.cpu().numpy())


def test_pinned_kernel_makes_shard_launches_bit_equal_to_the_full_launch(sg):
    """The dispatcher picks the kernel by launch size and the kernels sum in different orders: a 512-sample shard of a
    4096-sample pendulum launch runs rollout_one_kernel where the full launch runs rollout_tiles_kernel - equal to round-off,
    not bit for bit.  gpmpc_rollout_pin_kernel (rollout.pin_rollout_kernel_like) gives the shard the full launch's kernel:
    bit-equal again."""
    from sampling_gpmpc_amd.rollout import forward_sampling_rollout, rollout_device, pin_rollout_kernel_like
    from sampling_gpmpc_amd import _lib
    Ns, H = 4096, 30
    p = fs_params("params_pendulum1D_samples", Ns, H)
    p["agent"]["base_sample_generator"] = "vectorized"
    torch.manual_seed(11)
    pg = {**p, "common": {**p["common"], "use_cuda": True}}
    agent = sg.Agent(pg, sg.make_env(pg))
    u_ff = synthetic_u_ff(1, H)
    lib = _lib.load()
    try:
        X = forward_sampling_rollout(agent, u_ff)
        assert lib.gpmpc_rollout_last_kernel() == 3
        erv = agent.epistimic_random_vector
        per_slab = Ns * 3
        z = erv.reshape(-1)[per_slab:]
        kw = dict(H=H, mode=_lib.MODE_RECONDITIONED, use_model_without_derivatives=False, sample_slice=(1024, 1536))
        sub = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, **kw).X_traj.cpu().numpy()
        assert lib.gpmpc_rollout_last_kernel() == 4
        assert not np.array_equal(sub, X[1024:1536])
        np.testing.assert_allclose(sub, X[1024:1536], rtol=1e-9, atol=1e-11)
        assert pin_rollout_kernel_like(agent, H=H, Ns_launch=Ns) == 3
        sub = rollout_device(agent, u_ff, z, erv.shape[1] * per_slab, **kw).X_traj.cpu().numpy()
        assert lib.gpmpc_rollout_last_kernel() == 3
        np.testing.assert_array_equal(sub, X[1024:1536])
    finally:
        lib.gpmpc_rollout_pin_kernel(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("Ns,g_ny,H,T,beta", [(1024, 1, 30, 3, 2.5), (4096, 3, 40, 3, 3.0), (32768, 3, 40, 1, 30.0)])
def test_base_samples_kernel_against_the_torch_form(sg, Ns, g_ny, H, T, beta):
    """gpmpc_base_samples (one launch, one wave per vector, the whole-vector rejection loop of reference src/agent.py:84-100 inside
    the wave) against the same counter stream evaluated with torch ops on the same device: bit-identical, at two global-sample
    offsets (a shard of a larger run is the slice of the whole run); inside the bounds; attempts counted."""
    from sampling_gpmpc_amd.agent import counter_base_samples
    n_mpc, n_itrs = 2, 3
    for offset in (0, 777):
        z = counter_base_samples(n_mpc, n_itrs, Ns, g_ny, H, T, beta, seed=4242, offset=offset, device="cuda")
        zt = counter_base_samples(n_mpc, n_itrs, Ns, g_ny, H, T, beta, seed=4242, offset=offset, device="cuda", _force_torch=True)
        assert z.shape == (n_mpc, n_itrs, Ns, g_ny, H, T) and z.is_cuda
        assert torch.equal(z, zt), f"max |diff| {float((z - zt).abs().max()):.3e}"
        assert float(z.abs().max()) <= beta
    whole = counter_base_samples(n_mpc, n_itrs, Ns + 777, g_ny, H, T, beta, seed=4242, offset=0, device="cuda")
    assert torch.equal(whole[:, :, 777:], z)
    # the attempts the kernel reports are those of the rule: every earlier attempt has an entry outside the bounds
    lib = sg._lib.load()
    V = g_ny * H * T
    out = torch.empty(n_mpc, n_itrs, 64, V, dtype=F64, device="cuda")
    att = torch.zeros(n_mpc, n_itrs, 64, dtype=torch.int32, device="cuda")
    sg._lib.check(lib.gpmpc_base_samples(4242, n_mpc, n_itrs, 0, 64, V, beta, sg._lib.dptr(out), sg._lib.dptr(att),
                                         sg._lib.current_stream_ptr()), "gpmpc_base_samples")
    torch.cuda.synchronize()
    assert torch.equal(out.reshape(n_mpc, n_itrs, 64, g_ny, H, T), whole[:, :, :64])
    if beta < 10:
        assert int(att.max()) >= 1, "with these bounds some vector needs a second attempt"
    print(f"Ns={Ns} V={V} beta={beta}: mean attempts {float(att.float().mean()) + 1:.2f}")

