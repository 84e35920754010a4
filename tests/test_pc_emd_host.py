"""CPU-side checks of the 3-D variant's earth mover's evaluation (csrc/pc_emd.hip, sivae_hip.pointcloud.emd_matrix,
soft_intro_vae_3d/metrics/evaluation_metrics.py::emd_matrix): the argument validation of sivae_emd_matrix (every call
returns before any launch), the Python surface, and the numpy oracle tests/pc3d_emd_oracle.py against ground truth: exact
optimal matchings by brute force (and by scipy's assignment solver where it is installed), the plan's marginals, and the
invariance under a permutation of either cloud's points."""
import ctypes
import inspect
import itertools
import math

import numpy as np
import pytest
import torch

import pc3d_emd_oracle as MO
from sivae_hip import lib


def test_pc_emd_entry_points_validate_arguments():
    """null pointers, non-positive sizes, empty / out-of-range row ranges, S R >= 2^31 - 1, clouds beyond 4096 points, a
    flag outside {0, 1}, a null workspace: the documented codes, in the manner of test_pc_eval_host.py.  No size uses a
    workspace (both clouds are held in LDS), so the size function returns 0 throughout and no workspace can be short."""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    f = L.sivae_emd_matrix
    ok = dict(sample=one, ss=30, sn=3, sc=1, ref=one, rs=30, rn=3, rc=1, D=one, S=4, R=5, M=10, N=10, s0=0, s1=4, norm=1,
              ws=one, ws_bytes=0, stream=null)

    def em(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("sample", "ref", "D"):
        assert em(**{k: null}) == -1, k
    for k in ("S", "R", "M", "N"):
        assert em(**{k: 0}) == -2 and em(**{k: -3}) == -2, k
    assert em(s0=2, s1=2) == -2 and em(s0=3, s1=2) == -2 and em(s0=-1) == -2 and em(s1=5) == -2  # row range
    assert em(S=1 << 16, R=1 << 15, s1=1) == -5
    assert em(S=0x7fffffff, R=1, s1=1) == -5            # (the bound itself is refused)
    assert em(M=4097) == -5 and em(N=4097) == -5 and em(M=4097, N=4097) == -5
    assert em(norm=2) == -6 and em(norm=-1) == -6
    assert em(ws=null) == -4                             # (a null workspace is refused although none is used)
    assert em(M=4096, N=4096, ws=null) == -4
    wb = L.sivae_emd_matrix_workspace_bytes
    for args in ((4, 5, 10, 10), (4, 5, 2049, 1025), (3000, 800, 4096, 4096), (1, 1, 1, 1), (0, 5, 10, 10),
                 (4, 5, 4097, 10)):
        assert wb(*args) == 0, args
    assert L.sivae_abi_version() == 1


def test_pointcloud_surface():
    from sivae_hip import pointcloud as PC
    x = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.emd_matrix(x, x)
    for bad in (torch.zeros(5, 3), torch.zeros(2, 3, 5), torch.zeros(2, 5, 3, 1)):
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            PC.emd_matrix(bad, x)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            PC.emd_matrix(x, bad)
    # the point limit is checked before any launch (test_more_than_4096_points_raise_before_any_launch runs it)
    src = inspect.getsource(PC.emd_matrix)
    assert src.index("EMD_MAX_POINTS") < src.index("_lib.call(") and PC.EMD_MAX_POINTS == 4096
    # the module's idiom: checks, allocation through the module's torch / workspace (what tests/support/guard.py patches)
    assert "_require_clouds(" in src and "workspace(" in src and "torch.empty(" in src and "timer_end(" in src
    assert "EMD_POINT_PAIRS_PER_LAUNCH" in src and PC.EMD_POINT_PAIRS_PER_LAUNCH > 0
    assert "emd_matrix(sample [S, M, 3], ref [R, N, 3]" in PC.__doc__


@pytest.mark.parametrize("side", ["sample", "ref"])
def test_more_than_4096_points_raise_before_any_launch(monkeypatch, side):
    """the device check is stood in for (there is no device here); the library must not be reached"""
    from sivae_hip import pointcloud as PC
    small, large = torch.zeros(1, 5, 3), torch.zeros(1, 4097, 3)
    monkeypatch.setattr(PC, "_require_clouds", lambda pcs, who: (pcs.shape[0], pcs.shape[1], pcs.stride()))
    monkeypatch.setattr(PC._lib, "call", lambda *a: pytest.fail("the library was called"))
    monkeypatch.setattr(PC._lib, "load", lambda: pytest.fail("the library was asked for a workspace size"))
    with pytest.raises(ValueError, match="4096"):
        PC.emd_matrix(*((large, small) if side == "sample" else (small, large)))


def test_drop_in_module_surface():
    import soft_intro_vae_3d.metrics.evaluation_metrics as E
    assert "emd_matrix" in E.__all__ and callable(E.emd_matrix)
    assert list(inspect.signature(E.emd_matrix).parameters) == ["sample_pcs", "ref_pcs", "normalize"]
    assert inspect.signature(E.emd_matrix).parameters["normalize"].default is True
    assert "dist=emd_matrix(x_g, x)" in E.__doc__
    x = np.zeros((2, 5, 3), dtype=np.float32)
    for f in (E.minimum_mathing_distance, E.coverage):
        with pytest.raises(NotImplementedError, match=r"emd_matrix.*dist=|dist=.*emd_matrix"):
            f(x, x, use_EMD=True)
    for bad in (np.zeros((5, 3), dtype=np.float32), torch.zeros(2, 3, 5)):
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            E.emd_matrix(bad, x)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            E.emd_matrix(x, bad)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E.emd_matrix(x, x)
    src = inspect.getsource(E)
    for banned in ("tensorflow", "scipy", "sklearn"):
        assert "import " + banned not in src and "from " + banned not in src


# ------------------------------------------------------------------------------------------------ the oracle
def _cloud(rng, n):
    return rng.random((n, 3)) - 0.5


def _exact_by_permutations(A, B):
    """the optimal transport cost between A (mass big / n a point) and B (mass big / m a point), big = max(n, m): every
    point is repeated until all carry the same mass big / L, L = lcm(n, m) <= 6, and the L! assignments are tried (an
    optimal transport between equal integer masses is an assignment)"""
    n, m = len(A), len(B)
    L = n * m // math.gcd(n, m)
    assert L <= 6
    A, B = np.repeat(A, L // n, axis=0), np.repeat(B, L // m, axis=0)
    dist = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2))
    perms = np.array(list(itertools.permutations(range(L))))
    return float(dist[np.arange(L)[None, :], perms].sum(axis=1).min()) * max(n, m) / L


def test_one_point_against_one_is_their_distance():
    A, B = np.array([[0.25, -0.5, 1.0]]), np.array([[-0.75, 0.5, 0.0]])
    for normalize in (True, False):
        assert abs(MO.emd(A, B, normalize) - math.sqrt(3.0)) <= 1e-8
    assert MO.emd(A, A) == 0.0
    D = MO.emd_matrix(B[None], A[None])
    assert D.shape == (1, 1) and abs(D[0, 0] - math.sqrt(3.0)) <= 1e-8


@pytest.mark.parametrize("n,m", [(5, 5), (64, 64), (7, 12), (12, 7), (40, 100), (1, 9), (9, 1)])
def test_plan_marginals_are_the_masses(n, m):
    rng = np.random.default_rng(100 * n + m)
    A, B = _cloud(rng, n), _cloud(rng, m)
    value, plan = MO.emd(A, B, normalize=False, return_plan=True)
    big = max(n, m)
    assert plan.shape == (n, m) and (plan >= 0).all()
    assert np.abs(plan.sum(axis=1) - big / n).max() <= 1e-6
    assert np.abs(plan.sum(axis=0) - big / m).max() <= 1e-6
    dist = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2))
    assert abs(value - float((plan * dist).sum())) <= 1e-12 * value      # (the cost is the plan's)
    assert abs(MO.emd(A, B, normalize=True) - value / big) <= 1e-15 * value


def test_never_below_the_exact_optimum_small_clouds():
    """feasibility of the plan implies approx >= exact up to the 1e-9 terms of the definition"""
    rng = np.random.default_rng(7)
    sizes = [(k, k) for k in range(1, 7)] * 8 + [(1, 4), (4, 1), (2, 4), (4, 2), (2, 6), (6, 3), (3, 2), (2, 3), (1, 6)] * 4
    worst_lo, worst_hi = np.inf, 0.0
    for n, m in sizes:
        A, B = _cloud(rng, n), _cloud(rng, m)
        exact = _exact_by_permutations(A, B)
        approx = MO.emd(A, B, normalize=False)
        assert approx >= exact * (1 - 1e-8), (n, m, approx, exact)
        worst_lo, worst_hi = min(worst_lo, approx / exact), max(worst_hi, approx / exact)
    print("approx / exact over %d small cloud pairs: %.12f ... %.4f" % (len(sizes), worst_lo, worst_hi))
    assert worst_hi <= 2.0                                                # (an approximation, not a wild guess)


@pytest.mark.parametrize("n", [64, 300])
def test_never_below_the_exact_optimum_scipy(n):
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(n)
    A, B = _cloud(rng, n), _cloud(rng, n)
    dist = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2))
    rows, cols = opt.linear_sum_assignment(dist)
    exact = float(dist[rows, cols].sum())
    approx = MO.emd(A, B, normalize=False)
    print("n = %d: approx / exact = %.4f" % (n, approx / exact))
    assert approx >= exact * (1 - 1e-8)


def test_jittered_permutation_of_itself_is_within_one_percent_of_exact():
    rng = np.random.default_rng(64)
    A = _cloud(rng, 64)
    perm = rng.permutation(64)
    B = A[perm] + 1e-3 * rng.standard_normal((64, 3))
    dist = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(axis=2))
    # every point's nearest neighbour is its own jittered copy and the map is one to one: the sum of the nearest-neighbour
    # distances, a lower bound of any matching's cost, is then the cost of a matching, hence the exact optimum
    nearest = dist.argmin(axis=1)
    assert np.array_equal(np.sort(nearest), np.arange(64)) and np.array_equal(perm[nearest], np.arange(64))
    exact = float(dist.min(axis=1).sum())
    approx = MO.emd(A, B, normalize=False)
    print("jittered permutation: approx / exact = %.6f" % (approx / exact))
    assert exact * (1 - 1e-8) <= approx <= 1.01 * exact


@pytest.mark.parametrize("n,m", [(33, 33), (20, 45)])
def test_point_order_does_not_matter(n, m):
    rng = np.random.default_rng(n + m)
    A, B = _cloud(rng, n), _cloud(rng, m)
    base = MO.emd(A, B)
    assert abs(MO.emd(A[rng.permutation(n)], B) - base) < 1e-12 * base
    assert abs(MO.emd(A, B[rng.permutation(m)]) - base) < 1e-12 * base


def test_matrix_convention_and_non_finite_clouds():
    rng = np.random.default_rng(3)
    sample = rng.random((2, 6, 3)).astype(np.float32) - 0.5
    ref = rng.random((3, 9, 3)).astype(np.float32) - 0.5
    D = MO.emd_matrix(sample, ref)
    assert D.shape == (2, 3) and D.dtype == np.float64
    assert D[1, 2] == MO.emd(ref[2], sample[1]) and D[1, 2] != MO.emd(sample[1], ref[2])   # left = ref: not symmetric
    assert np.allclose(MO.emd_matrix(sample, ref, normalize=False), D * 9, rtol=1e-14, atol=0)   # (big = max(6, 9))
    D32 = MO.emd_matrix(sample, ref, dtype=np.float32)
    assert D32.dtype == np.float64 and 0 < np.abs(D32 - D).max() <= 1e-5 * D.max()
    bad_s, bad_r = sample.copy(), ref.copy()
    bad_s[0, 3, 1] = np.nan
    bad_r[1, 0, 2] = -np.inf
    Db = MO.emd_matrix(bad_s, bad_r)
    want = np.zeros((2, 3), dtype=bool)
    want[0, :] = True
    want[:, 1] = True
    assert np.array_equal(np.isnan(Db), want) and np.array_equal(Db[~want], D[~want])
