"""``gpmpc_pairwise_lipschitz`` / ``pairwise_lipschitz`` on the device against the reference's own formula on the CPU
(``robust_tube_based_GPMPC_koller.py:34-44``, ``robust_tube_reference.lipschitz_formula``).

Tolerance: a ratio is two sums of at most 8 squares, two square roots, one addition and one division - each correctly rounded, the
sums' relative error at most 8 * 2^-53 under a square root - far inside ``rtol = 64 * 2^-52``; the CPU formula rounds the same
quantities in another order, within the same bound."""
import pytest
import torch

from sampling_gpmpc_amd import _lib
from sampling_gpmpc_amd.robust_tube import pairwise_lipschitz
from tests import robust_tube_reference as ref

pytestmark = pytest.mark.gpu
F64 = torch.float64
DEV = "cuda"
RTOL = 64 * 2.0 ** -52
SHAPES = [(2, 1, 1), (4, 4, 6), (8, 8, 8)]                 # (dx, G, df); the last one takes the 32-row tile, the others the 64-row one


def problem(N, dx, G, df, seed=0):
    g = torch.Generator().manual_seed(1000 * N + 100 * dx + 10 * G + df + seed)
    X = torch.randn(N, dx, dtype=F64, generator=g)
    Wm = torch.randn(G, df, dx, dtype=F64, generator=g)
    F = torch.sin(torch.einsum("gfd,nd->ngf", Wm, X)) + 0.1 * torch.randn(N, G, df, dtype=F64, generator=g)
    return X, F


def device_result(X, F, eps=1e-6, max_blocks=0):
    mx, pair, skipped = pairwise_lipschitz(X.to(DEV), F.to(DEV), eps, max_blocks)
    torch.cuda.synchronize()
    return mx.cpu(), pair.cpu(), int(skipped)


def ratio_of(X, F, pair, g, eps):
    i, j = int(pair[g, 0]), int(pair[g, 1])
    return float(torch.norm(F[i, g] - F[j, g]) / (torch.norm(X[i] - X[j]) + eps))


@pytest.mark.parametrize("dx,G,df", SHAPES)
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 257, 1025])
def test_maximum_and_pair_against_the_cpu_formula(N, dx, G, df):
    X, F = problem(N, dx, G, df)
    eps = 1e-6
    mx, pair, skipped = device_result(X, F, eps)
    want, want_pair, _ = ref.lipschitz_cpu(X, F, eps)
    assert mx.shape == (G,) and pair.shape == (G, 2) and pair.dtype == torch.int64 and skipped == 0
    if N < 2:
        assert not bool(mx.any()) and bool((pair == -1).all())
        return
    torch.testing.assert_close(mx, want, rtol=RTOL, atol=0)
    assert bool((pair[:, 0] >= 0).all()) and bool((pair[:, 0] < pair[:, 1]).all()) and bool((pair[:, 1] < N).all())
    for g in range(G):
        r = ratio_of(X, F, pair, g, eps)
        assert abs(r - float(mx[g])) <= RTOL * float(mx[g]), (g, r, float(mx[g]))


def test_ungrouped_f_and_the_reference_formula_itself():
    X, F = problem(257, 4, 1, 6)
    mx, pair, skipped = pairwise_lipschitz(X.to(DEV), F[:, 0].to(DEV))
    torch.cuda.synchronize()
    assert mx.dim() == 0 and pair.shape == (2,) and skipped.dim() == 0
    want = float(ref.lipschitz_formula(X, F[:, 0]).max())                   # torch.max(ratio), diagonal (0) and lower triangle included
    assert abs(float(mx) - want) <= RTOL * want


@pytest.mark.parametrize("eps", [0.0, 0.5])
def test_a_planted_exact_tie_returns_the_lowest_pair(eps):
    """Integer points on a line, F zero but for two spikes of the same height: the pairs (69, 70), (70, 71), (199, 200) and
    (200, 201) - in different tiles, so in different workgroups - have the same operands, hence the same ratio bit for bit."""
    N = 257
    X = torch.zeros(N, 2, dtype=F64)
    X[:, 0] = torch.arange(N, dtype=F64)
    F = torch.zeros(N, 2, 3, dtype=F64)
    F[70, 0, 1] = F[200, 0, 1] = 8.0
    F[:, 1, 0] = 2.0 * X[:, 0]                                               # group 1: with eps = 0 every pair has ratio 2
    for max_blocks in (0, 1, 3):
        mx, pair, skipped = device_result(X, F, eps, max_blocks)
        assert float(mx[0]) == 8.0 / (1.0 + eps) and pair[0].tolist() == [69, 70]
        if eps == 0.0:
            assert float(mx[1]) == 2.0 and pair[1].tolist() == [0, 1]
        else:
            assert pair[1].tolist() == [0, N - 1]                            # 2 d / (d + eps) grows with the distance
        assert skipped == 0


@pytest.mark.parametrize("dx,G,df", SHAPES)
def test_rows_with_a_non_finite_entry_are_skipped_and_counted(dx, G, df):
    N = 257
    X, F = problem(N, dx, G, df, seed=5)
    clean = ref.lipschitz_cpu(X, F)
    i0, j0 = (int(v) for v in clean[1][0])                                   # spoil the rows that attain group 0's maximum
    X[i0, dx - 1] = float("nan")
    F[j0, G - 1, df - 1] = float("inf")
    F[200, 0, 0] = float("-inf")
    mx, pair, skipped = device_result(X, F)
    want, want_pair, want_skipped = ref.lipschitz_cpu(X, F)
    assert skipped == want_skipped == len({i0, j0, 200})
    torch.testing.assert_close(mx, want, rtol=RTOL, atol=0)
    assert bool(torch.isfinite(mx).all()) and float(mx[0]) < float(clean[0][0])
    bad = torch.tensor(sorted({i0, j0, 200}))
    assert not bool(torch.isin(pair, bad).any())
    assert torch.equal(pair, want_pair)                                      # random data: no ties, the pair is the CPU's
    Xn = torch.full((5, dx), float("nan"), dtype=F64)
    mx, pair, skipped = device_result(Xn, torch.zeros(5, G, df, dtype=F64))
    assert not bool(mx.any()) and bool((pair == -1).all()) and skipped == 5


@pytest.mark.parametrize("dx,G,df", SHAPES)
def test_the_result_does_not_depend_on_the_grid(dx, G, df):
    X, F = problem(1025, dx, G, df, seed=9)
    X[17, 0] = float("nan")
    base = device_result(X, F)
    for max_blocks in (1, 7, 64):
        other = device_result(X, F, max_blocks=max_blocks)
        assert torch.equal(base[0], other[0]) and torch.equal(base[1], other[1]) and base[2] == other[2] == 1, max_blocks


def test_sizes_outside_the_kernel_are_errors():
    for shape_x, shape_f in (((4, 9), (4, 1, 1)), ((4, 2), (4, 9, 1)), ((4, 2), (4, 1, 9))):
        with pytest.raises(_lib.GpmpcError, match="dx <= 8"):
            pairwise_lipschitz(torch.zeros(shape_x, dtype=F64, device=DEV), torch.zeros(shape_f, dtype=F64, device=DEV))
    with pytest.raises(_lib.GpmpcError):
        pairwise_lipschitz(torch.zeros(4, 2, dtype=F64, device=DEV), torch.zeros(5, 1, 1, dtype=F64, device=DEV))
    with pytest.raises(_lib.GpmpcError, match="eps"):
        pairwise_lipschitz(torch.zeros(4, 2, dtype=F64, device=DEV), torch.zeros(4, 1, 1, dtype=F64, device=DEV), eps=-1.0)
