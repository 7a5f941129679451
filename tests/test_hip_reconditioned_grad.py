"""``gpmpc_rollout_vjp`` / ``reconditioned_rollout(differentiable=True)`` / ``plan_inputs_reconditioned`` on the device against the CPU
reference A of tests/reconditioned_grad_reference.py (every step a from-scratch dense Cholesky of [real; own draws], gradients by
autograd through the whole rollout, no analytic derivative) and against central differences of ``gpmpc_rollout`` itself.  The
kernel is never compared with itself.

Tolerances are measured, not chosen (the rule of tests/test_hip_moments.py): ``WORST_AB`` records, per case and quantity, the deviation
between the CPU references A and B (B: the append-row factor and the reverse sweep written out by hand), with and without ``g_Y``
and under 1, 2, 4 and 8 host threads and the package's default (the figures move with the BLAS's blocking), the largest figure -
``X`` per state dimension, ``Y`` per output and task, each gradient per sample relative to the largest magnitude in that sample's block (``reconditioned_grad_reference.deviations``).  The kernel's gradients get 8 x that, never less than 16 * 2^-52;
tests/test_reconditioned_grad_host.py re-measures A against B against this table without a GPU, and ``python -m
tests.reconditioned_grad_reference`` prints it.  ``FD_ERR`` is the error of a central difference of form A (beta = 30, the fixed
direction ``fd_direction``, h = ``FD_H``) against form A's own autograd; the device's finite differences get 8 x that.
"""
import pytest
import torch

from sampling_gpmpc_amd import _lib
from tests import reconditioned_grad_reference as ref
from tests import rollout_variants as rv

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
FAIL_BITS = _lib.INFO_ROOT_FAIL | _lib.INFO_NEG_1x1 | _lib.INFO_TRAIN_CHOL_FAIL | _lib.INFO_STATE_FULL | _lib.INFO_NONFINITE

WORST_AB = {
    "pend_fb@H1": {"X": 1.5e-15, "Y": 9.6e-13, "x0": 3.7e-13, "U": 2.8e-13},
    "pend_fb@H2": {"X": 2.1e-15, "Y": 5.5e-13, "x0": 1.2e-12, "U": 7.9e-13},
    "pend_fb@H4": {"X": 5.6e-15, "Y": 2.7e-12, "x0": 1.3e-12, "U": 5.0e-13},
    "pend_nofb@H23": {"X": 3.3e-14, "Y": 6.8e-13, "x0": 1.1e-12, "U": 2.2e-12},
    "car@H5": {"X": 5.1e-12, "Y": 2.6e-11, "x0": 8.5e-11, "U": 5.4e-11},
    "car@H15": {"X": 6.7e-12, "Y": 7.3e-11, "x0": 1.7e-10, "U": 2.7e-11},
    "pend_clip": {"X": 2.5e-15, "Y": 1.9e-12, "x0": 2.2e-13, "U": 2.0e-13},
    "pend_zero": {"X": 1.9e-16, "Y": 6.9e-14, "x0": 2.5e-14, "U": 1.4e-14},
    "raw_floor": {"X": 1.9e-15, "Y": 1.3e-12, "x0": 4.7e-12, "U": 3.3e-13},
}
FD_ERR = {"pend_fb@H4": 4.2e-08, "car@H5": 5.2e-08}


@pytest.fixture(scope="module")
def sg():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: -m gpu tests must run on the MI355X box")
    import sampling_gpmpc_amd as pkg
    pkg._lib.load()
    return pkg


_AGENTS = {}


def agent_of(sg, name):
    """The product agent of ``rollout_variants.make_pair`` on the case's training set, one per (env, Ns, H, feedback)."""
    c = ref.CASES[name]
    key = (c.env, c.Ns, c.H, c.feedback)
    if key not in _AGENTS:
        _AGENTS[key] = rv.make_pair(sg, c.rv_case())[0]
    return _AGENTS[key]


def descriptors(sg, name):
    """(plan, GP descriptor with the case's variance floor, env descriptor) for the raw C-ABI calls"""
    m = ref.model(name)
    ag = agent_of(sg, name)
    plan = ag._plan(use_grad=True)
    desc = _lib.GpDesc.from_buffer_copy(plan.desc)
    desc.var_floor = m.var_floor
    return plan, desc, ag.env_desc(m.use_fb)


def raw_forward(sg, name, x0, U, z, beta=None):
    """``gpmpc_rollout`` at the C-ABI: x0 (Ns, nx), U (H, nu), z (H, Ns, g_ny, T) on the device -> (X, Y, Xi, info)."""
    m = ref.model(name, beta)
    lib = _lib.load()
    plan, desc, env = descriptors(sg, name)
    H, Ns = int(z.shape[0]), int(z.shape[1])
    X = torch.empty(Ns, m.nx, H + 1, dtype=F64, device=DEV)
    Y = torch.empty(Ns, m.g_ny, H, 3, dtype=F64, device=DEV)
    Xi = torch.empty(Ns, H, 2, dtype=F64, device=DEV)
    info = torch.zeros(Ns, dtype=torch.int32, device=DEV)
    nbytes = lib.gpmpc_rollout_workspace_bytes(desc, _lib.MODE_RECONDITIONED, 3, Ns, H)
    ws = _lib.workspace(nbytes, DEV)
    _lib.check(lib.gpmpc_rollout(desc, env, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), _lib.MODE_RECONDITIONED, 3, m.var_zero_thr, m.beta, Ns,
                                 H, _lib.dptr(x0), 1, _lib.dptr(U), _lib.dptr(z), Ns * m.g_ny * 3, _lib.dptr(X), _lib.dptr(Y), _lib.dptr(Xi),
                                 _lib.dptr(info), _lib.dptr(ws), ws.numel(), _lib.current_stream_ptr()), "gpmpc_rollout")
    return X, Y, Xi, info


def raw_vjp(sg, name, x0, U, z, fwd, g_X, g_Y, beta=None):
    """``gpmpc_rollout_vjp`` at the C-ABI -> per-sample (g_x0 (Ns, nx), g_U (Ns, H, nu), info (Ns))"""
    m = ref.model(name, beta)
    lib = _lib.load()
    plan, desc, env = descriptors(sg, name)
    H, Ns = int(z.shape[0]), int(z.shape[1])
    X, Y, Xi, info_f = fwd
    g_x0 = torch.empty(Ns, m.nx, dtype=F64, device=DEV)
    g_U = torch.empty(Ns, H, m.nu, dtype=F64, device=DEV)
    info = torch.zeros(Ns, dtype=torch.int32, device=DEV)
    nbytes = lib.gpmpc_rollout_vjp_workspace_bytes(desc, Ns, H)
    assert nbytes > 0
    ws = _lib.workspace(nbytes, DEV)
    _lib.check(lib.gpmpc_rollout_vjp(desc, env, _lib.dptr(plan.buf), _lib.dptr(plan.X_r), m.var_zero_thr, m.beta, Ns, H, _lib.dptr(x0), 1,
                                     _lib.dptr(U), _lib.dptr(z), Ns * m.g_ny * 3, _lib.dptr(X), _lib.dptr(Y), _lib.dptr(Xi), _lib.dptr(info_f),
                                     _lib.dptr(g_X), _lib.dptr(g_Y), _lib.dptr(g_x0), _lib.dptr(g_U), _lib.dptr(info), _lib.dptr(ws),
                                     ws.numel(), _lib.current_stream_ptr()), "gpmpc_rollout_vjp")
    return g_x0, g_U, info


def device_inputs(name, beta=None):
    m = ref.model(name, beta)
    gX, gY = ref.cotangents(name)
    return (m.x0.expand(m.Ns, m.nx).contiguous().to(DEV), m.U.contiguous().to(DEV), m.z.contiguous().to(DEV), gX.contiguous().to(DEV),
            gY.contiguous().to(DEV))


_RUNS = {}


def device_run(sg, name):
    """forward once per case, shared and left unchanged"""
    if name not in _RUNS:
        x0, U, z, _, _ = device_inputs(name)
        _RUNS[name] = raw_forward(sg, name, x0, U, z)
    return _RUNS[name]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the kernel against form A
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gy", [True, False], ids=["g_Y", "no_g_Y"])
@pytest.mark.parametrize("name", ref.NAMED)
def test_kernel_against_form_a(sg, name, with_gy):
    """Two launches, both held to 8 x WORST_AB: the VJP at form A's own forward (X_traj, Y, Xi uploaded), where both differentiate at the
    same point and the figure is the kernel's alone, and the shipped path, the device's own forward followed by the VJP.  The device's
    X_traj and Y are held to the same table.  ``car@H15`` runs the instance that keeps factor and adjoint in the workspace."""
    x0, U, z, gX, gY = device_inputs(name)
    fwd = device_run(sg, name)
    fa = ref.forward_A(name)
    at_a = (fa["X"].contiguous().to(DEV), fa["Y"].contiguous().to(DEV), ref.gp_inputs_A(name).contiguous().to(DEV), torch.zeros_like(fwd[3]))
    g_x0, g_U, info = raw_vjp(sg, name, x0, U, z, at_a, gX, gY if with_gy else None)
    d_x0, d_U, d_info = raw_vjp(sg, name, x0, U, z, fwd, gX, gY if with_gy else None)
    torch.cuda.synchronize()
    want = ref.results_A(name, with_gy)
    dev = ref.deviations(name, want, {"X": fwd[0].cpu(), "Y": fwd[1].cpu(), "x0": g_x0.cpu(), "U": g_U.cpu()})
    dev_d = ref.deviations(name, want, {"x0": d_x0.cpu(), "U": d_U.cpu()})
    tol = ref.tolerances(WORST_AB[name])
    print(name, with_gy, {q: f"{v:.2e} / {tol[q]:.2e}" for q, v in dev.items()}, "on the device's forward", {q: f"{v:.2e}" for q, v in dev_d.items()},
          "info", fwd[3].tolist(), info.tolist())
    assert sorted(dev) == sorted(ref.QUANTITIES) and max(tol.values()) <= 1e-2
    for q in ref.QUANTITIES:
        assert dev[q] <= tol[q], (name, with_gy, q, dev[q], tol[q])
    for q in ref.GRADIENTS:
        assert dev_d[q] <= tol[q], (name, with_gy, "on the device's forward", q, dev_d[q], tol[q])
    allowed = _lib.INFO_VAR_CLAMPED if name == "raw_floor" else 0
    for i in (info, d_info):
        assert not bool((i.cpu() & ~allowed).any()) and torch.equal(i.cpu() & allowed, fwd[3].cpu() & allowed)


def test_the_long_car_case_keeps_its_factor_in_the_workspace(sg):
    """car@H15: three chains' factors and adjoints are 169 KB, above the 160 KiB - 256 B of LDS, so every launch of the case above, of the
    bit-equality, containment and wrapper tests below runs ``rollout_vjp_kernel<false>``; every other case stays in LDS."""
    lib = _lib.load()
    for name in ref.NAMED:
        m = ref.model(name)
        nbytes = lib.gpmpc_rollout_vjp_workspace_bytes(descriptors(sg, name)[1], m.Ns, m.H)
        n_r, nh = m.X_r.shape[0], 3 * m.H
        per_chain = 2 * (n_r * nh + nh * (nh + 1) // 2) * 8
        assert nbytes == ((m.Ns * m.g_ny * per_chain + 255) // 256 * 256 + 256 if name == "car@H15" else 256), name


# ---------------------------------------------------------------------------------------------------------------------
# 2. finite differences of the shipped forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pin", ["generic", "auto"])
@pytest.mark.parametrize("name", ref.FD_CASES)
def test_vjp_against_central_differences_of_the_forward(sg, name, pin):
    """beta = 30: no slot is clipped; info == 0 is asserted for every sample and every launch, so nothing is left out."""
    lib = _lib.load()
    x0, U, z, gX, gY = device_inputs(name, ref.FD_BETA)
    d_x0, d_U = (t.to(DEV) for t in ref.fd_direction(name))
    infos = []
    prev = lib.gpmpc_rollout_pin_kernel(_lib.KERNEL_GENERIC if pin == "generic" else _lib.KERNEL_AUTO)
    try:
        def loss(x0_, U_):
            X, Y, _, info = raw_forward(sg, name, x0_.contiguous(), U_.contiguous(), z, ref.FD_BETA)
            infos.append(info)
            return (gX * X).sum(dim=(1, 2)) + (gY * Y).sum(dim=(1, 2, 3))

        fd = ref.central_difference(loss, x0, U, d_x0, d_U)
        fwd = raw_forward(sg, name, x0, U, z, ref.FD_BETA)
        kernel = lib.gpmpc_rollout_last_kernel()
    finally:
        lib.gpmpc_rollout_pin_kernel(prev)
    g_x0, g_U, info = raw_vjp(sg, name, x0, U, z, fwd, gX, gY, ref.FD_BETA)
    torch.cuda.synchronize()
    an = ref.directional(g_x0, g_U, d_x0, d_U)
    err = ref.fd_relative_error(fd.cpu(), an.cpu())
    print(name, pin, "kernel", kernel, f"{err:.2e} / {8.0 * FD_ERR[name]:.2e}", fd.tolist(), an.tolist())
    assert pin != "generic" or kernel == _lib.KERNEL_GENERIC
    for i in infos + [fwd[3], info]:
        assert not bool(i.cpu().any())
    assert err <= 8.0 * FD_ERR[name]


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. bit-equality, NULL cotangents, edge sizes and containment
# ---------------------------------------------------------------------------------------------------------------------
def _subset(t, idx, dim=0):
    return t.index_select(dim, idx).contiguous()


@pytest.mark.parametrize("name", ["pend_nofb@H23", "car@H5", "car@H15"])
def test_a_samples_gradient_bits_do_not_depend_on_the_launch(sg, name):
    """alone, inside the batch, at another position: the same forward outputs, sliced"""
    x0, U, z, gX, gY = device_inputs(name)
    fwd = device_run(sg, name)
    full = raw_vjp(sg, name, x0, U, z, fwd, gX, gY)
    Ns = x0.shape[0]
    j = Ns - 1
    for order in ([j], [j] + list(range(Ns - 1)), list(range(Ns)) + [j, 0]):
        idx = torch.tensor(order, device=DEV)
        sub = raw_vjp(sg, name, _subset(x0, idx), U, _subset(z, idx, 1), tuple(_subset(t, idx) for t in fwd), _subset(gX, idx),
                      _subset(gY, idx))
        torch.cuda.synchronize()
        for got, want in zip(sub, full):
            assert torch.equal(got.cpu(), want.cpu()[order])


@pytest.mark.parametrize("name", ["pend_fb@H4", "car@H5"])
def test_null_cotangents(sg, name):
    x0, U, z, gX, gY = device_inputs(name)
    fwd = device_run(sg, name)
    g_x0, g_U, info = raw_vjp(sg, name, x0, U, z, fwd, None, None)
    torch.cuda.synchronize()
    assert not bool(g_x0.any()) and not bool(g_U.any()) and not bool(info.any())
    both = raw_vjp(sg, name, x0, U, z, fwd, gX, gY)
    only_x = raw_vjp(sg, name, x0, U, z, fwd, gX, None)
    only_y = raw_vjp(sg, name, x0, U, z, fwd, None, gY)
    torch.cuda.synchronize()
    for b, a, c in zip(both[:2], only_x[:2], only_y[:2]):                   # the VJP is linear in the cotangents
        assert bool(torch.isfinite(b).all()) and float(a.abs().max()) > 0 and float(c.abs().max()) > 0
        torch.testing.assert_close(a + c, b, rtol=1e-9, atol=1e-9 * float(b.abs().max()))


def test_empty_batch_and_empty_horizon(sg):
    from sampling_gpmpc_amd.reconditioned import reconditioned_rollout, reconditioned_rollout_vjp
    name = "car@H5"
    ag = agent_of(sg, name)
    x0, U, z, gX, gY = device_inputs(name)
    # H = 0: the tube is x0, g_x0 = g_X[:, :, 0]
    U0, z0 = torch.zeros(0, 2, dtype=F64, device=DEV), torch.zeros(0, 2, 3, 3, dtype=F64, device=DEV)
    res = reconditioned_rollout(ag, x0, U0, z0)
    g = gX[:, :, :1].contiguous()
    g_x0, g_U, info = reconditioned_rollout_vjp(ag, res, x0, U0, z0, g)
    torch.cuda.synchronize()
    assert res.X_traj.shape == (2, 4, 1) and torch.equal(res.X_traj[:, :, 0], x0) and res.Y.shape == (2, 3, 0, 3)
    assert torch.equal(g_x0, g[:, :, 0]) and g_U.shape == (0, 2) and not bool(info.any())
    # Ns = 0
    ze = torch.zeros(5, 0, 3, 3, dtype=F64, device=DEV)
    xe = torch.zeros(0, 4, dtype=F64, device=DEV)
    res = reconditioned_rollout(ag, xe, U, ze)
    g_x0, g_U, info = reconditioned_rollout_vjp(ag, res, xe, U, ze, None)
    assert res.X_traj.shape == (0, 4, 6) and g_x0.shape == (0, 4) and g_U.shape == (5, 2) and info.shape == (0,) and not bool(g_U.any())


@pytest.mark.parametrize("name", ["pend_fb@H4", "car@H5", "car@H15"])
def test_a_bad_sample_stays_with_itself(sg, name):
    """a non-finite x0, a non-finite cotangent or a flagged forward info of one sample: NaN and the bit for that sample, every other
    sample's bits unchanged"""
    x0, U, z, gX, gY = device_inputs(name)
    fwd = device_run(sg, name)
    clean = [t.cpu() for t in raw_vjp(sg, name, x0, U, z, fwd, gX, gY)]
    bad = 1
    others = [i for i in range(x0.shape[0]) if i != bad]
    xb, gb, ib = x0.clone(), gX.clone(), fwd[3].clone()
    xb[bad, 1] = float("nan")
    gb[bad, 0, 1] = float("inf")
    ib[bad] = _lib.INFO_ROOT_FAIL
    for x_, g_, i_, bit in ((xb, gX, fwd[3], _lib.INFO_NONFINITE), (x0, gb, fwd[3], _lib.INFO_NONFINITE), (x0, gX, ib, _lib.INFO_ROOT_FAIL)):
        got = [t.cpu() for t in raw_vjp(sg, name, x_, U, z, (fwd[0], fwd[1], fwd[2], i_), g_, gY)]
        assert bool(torch.isnan(got[0][bad]).all()) and bool(torch.isnan(got[1][bad]).all()) and int(got[2][bad]) == bit
        for g, c in zip(got, clean):
            assert torch.equal(g[others], c[others])
    assert not bool(clean[2].any())


# ---------------------------------------------------------------------------------------------------------------------
# 6. the autograd wrapper, 7. the planner
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pend_fb@H4", "car@H5", "car@H15"])
def test_differentiable_reconditioned_rollout(sg, name):
    from sampling_gpmpc_amd.reconditioned import reconditioned_rollout, reconditioned_rollout_vjp
    from sampling_gpmpc_amd.rollout import rollout_device
    m = ref.model(name)
    ag = agent_of(sg, name)
    x0, U, z, gX, gY = device_inputs(name)
    plain = reconditioned_rollout(ag, x0, U, z)
    exist = rollout_device(ag, U, z.reshape(-1), m.Ns * m.g_ny * 3, H=m.H, mode=_lib.MODE_RECONDITIONED, use_model_without_derivatives=False,
                           x0=x0, want_samples=True)
    xs, Us = x0.clone().requires_grad_(True), U.clone().requires_grad_(True)
    res = reconditioned_rollout(ag, xs, Us, z, differentiable=True)
    for k in ("X_traj", "Y", "Xi", "info"):
        assert torch.equal(getattr(plain, k), getattr(exist, k)) and torch.equal(getattr(res, k), getattr(plain, k)), k
    assert plain.X_traj.grad_fn is None and res.X_traj.grad_fn is not None and res.Y.grad_fn is not None
    assert not res.Xi.requires_grad and not res.info.requires_grad
    g1 = torch.autograd.grad((gX * res.X_traj).sum() + (gY * res.Y).sum(), (xs, Us))
    w1 = reconditioned_rollout_vjp(ag, plain, x0, U, z, gX, gY)
    per = reconditioned_rollout_vjp(ag, plain, x0, U, z, gX, gY, per_sample=True)
    torch.cuda.synchronize()
    assert torch.equal(g1[0], w1[0]) and torch.equal(g1[1], w1[1]) and g1[1].shape == U.shape and g1[0].shape == x0.shape
    assert torch.equal(per[1].sum(0), w1[1]) and torch.equal(per[0], w1[0])
    # X_traj alone (g_Y = NULL), a shared x0 (its gradient is the sum over the samples), U without a gradient
    x1 = m.x0.to(DEV).clone().requires_grad_(True)
    r2 = reconditioned_rollout(ag, x1, U, z, differentiable=True)
    assert torch.equal(r2.X_traj, plain.X_traj)
    g2, = torch.autograd.grad((gX * r2.X_traj).sum(), (x1,))
    w2 = reconditioned_rollout_vjp(ag, plain, m.x0.to(DEV), U, z, gX)
    assert g2.shape == (m.nx,) and torch.equal(g2, w2[0])
    want = ref.gradients_A(name, False)
    assert ref.deviations(name, {"x0": want["x0"].sum(0, keepdim=True)}, {"x0": g2.cpu()[None]})["x0"] <= 8.0 * max(ref.tolerances(WORST_AB[name]).values())


def test_plan_inputs_reconditioned_follows_the_loop_driven_by_form_a(sg):
    """pend_fb@H4, 5 steps of Adam on the shared U: the same loop on the CPU, its gradient from autograd through form A, gives the cost
    history within 8 x the case's largest tolerance (relative to the cost) at every iteration."""
    from sampling_gpmpc_amd.reconditioned import plan_inputs_reconditioned
    from sampling_gpmpc_amd.pathwise import sampled_tube_penalty                          # noqa: F401  (works on the tube unchanged)
    name, steps, lr = "pend_fb@H4", 5, 0.05
    m = ref.model(name)
    ag = agent_of(sg, name)
    _, want = ref.plan_reference(name, steps, lr)
    cost = ref.planner_cost(m.x_goal.to(DEV))
    U, got = plan_inputs_reconditioned(ag, m.x0.to(DEV), m.U.to(DEV), m.z.to(DEV), cost, steps, lr)
    torch.cuda.synchronize()
    got = got.cpu()
    tol = 8.0 * max(ref.tolerances(WORST_AB[name]).values())
    dev = (got - want).abs() / want.abs()
    print(name, [f"{float(d):.2e}" for d in dev], f"/ {tol:.2e}", got.tolist())
    assert got.shape == (steps + 1,) and U.shape == m.U.shape
    assert float(dev.max()) <= tol
    assert float(got[-1]) < float(got[0])
    U_, hist = plan_inputs_reconditioned(ag, m.x0.to(DEV), m.U.to(DEV), m.z.to(DEV), cost, 0, lr)
    assert torch.equal(U_.cpu(), m.U) and hist.shape == (1,)
