"""GPU checks of the 3-D variant's 1-nearest-neighbour accuracy: sivae_chamfer_matrix_self / sivae_nn1_loo
(csrc/pc_eval.hip), sivae_hip.pointcloud.chamfer_matrix_self / nn1_loo and one_nn_accuracy of the drop-in
soft_intro_vae_3d/metrics/evaluation_metrics.py.

No new tolerance: the self matrix is held BIT FOR BIT to the existing chamfer_matrix(x, x) (which tests/test_pc_eval_gpu.py
holds to the float64 oracle at 1e-5), nn1_loo to exact indices against tests/pc3d_nna_oracle.py on the same float32
matrices, and the metric to exact indices and scores against the float64 oracles wherever the oracle's own gap between the
best and the second-best candidate is at least MIN_GAP = 1e-4 (asserted per case; the matrices agree to 1e-5).

Self-matrix shapes (S, M) and what each covers (a block takes one cloud pair; the pairs i <= j are walked by folded rows
of S + 1 columns, at most 2048 blocks; a lane keeps 8 points, a block 2048; 1024 points are staged in LDS at a time)
  S = 1 .. 9, M = 4     odd and even fold, the middle row of an odd S, S = 1 and 2 (one folded row)
  (5, 33)               ragged lanes, fewer pairs than blocks
  (4, 256)              one full pair of queries per lane
  (3, 1030)             two staged chunks
  (2, 2053), (3, 2048)  the workspace spill (two chunks on both sides); the largest size without it
  (70, 8)               35 folded rows of 71: 2485 units on 2048 blocks, blocks walk one or two
"""
import functools

import numpy as np
import pytest
import torch

import pc3d_emd_oracle as MO
import pc3d_eval_oracle as EO
import pc3d_nna_oracle as NO
from support.pc import DEV, _PC, put

pytestmark = pytest.mark.gpu
SELF_CASES = [(S, 4) for S in range(1, 10)] + [(5, 33), (4, 256), (3, 1030), (2, 2053), (3, 2048)]
FLAGS = [(True, False), (True, True), (False, False), (False, True)]  # (normalize, use_sqrt)
# (seed, S, R, M, N) of the metric checks, the reference set scaled by 1.15: each asserts its own gap
METRIC_CASES = [(3024, 7, 5, 40, 55), (3025, 5, 8, 55, 40), (3026, 12, 12, 33, 33), (3027, 1, 6, 20, 20), (3028, 6, 1, 20, 20)]
MIN_GAP = 1e-4          # tests/test_pc_eval_gpu.py's, against its matrix tolerance of 1e-5
EMD_CASE = (4024, 5, 4, 16)  # (seed, S, R, N)
INF, NAN = float("inf"), float("nan")


def _E():
    import soft_intro_vae_3d.metrics.evaluation_metrics as E
    return E


@functools.lru_cache(maxsize=None)
def _set(S, M, seed=None):
    """float32 numpy clouds [S, M, 3] (never modified by a test): PCG64, uniform in the cube of side 1 about the origin"""
    x = (np.random.default_rng(S * 1000003 + M * 101 if seed is None else seed).random((S, M, 3)) - 0.5).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _two_sets(seed, S, R, M, N):
    """sample [S, M, 3] and ref [R, N, 3], the latter scaled by 1.15 (so that the sets differ a little)"""
    rng = np.random.default_rng(seed)
    sample = (rng.random((S, M, 3)) - 0.5).astype(np.float32)
    ref = ((rng.random((R, N, 3)) - 0.5) * 1.15).astype(np.float32)
    sample.setflags(write=False)
    ref.setflags(write=False)
    return sample, ref


@functools.lru_cache(maxsize=None)
def _metric_case(seed, S, R, M, N, normalize=True, use_sqrt=False):
    """-> (sample, ref, the oracle's result on its float64 Chamfer matrices); asserts the oracle's own gap"""
    sample, ref = _two_sets(seed, S, R, M, N)
    mats = [EO.chamfer_matrix(a, b, normalize, use_sqrt) for a, b in ((sample, sample), (sample, ref), (ref, ref))]
    gap = NO.smallest_gap(*mats)
    print("1-NNA case %s: smallest gap %.2e" % ((seed, S, R, M, N, normalize, use_sqrt), gap))
    assert gap >= MIN_GAP, "case %s: gap %.2e — float32 cannot be asked for the float64 neighbour" % ((seed, S, R, M, N), gap)
    return sample, ref, NO.one_nn_accuracy(*mats)


def _same(got, want):
    """a result dict of one_nn_accuracy against the oracle's: scores and indices exactly"""
    assert isinstance(got["acc"], float) and isinstance(got["acc_sample"], float) and isinstance(got["acc_ref"], float)
    assert got["nn"].dtype == np.int64 and got["nn_dist"].dtype == np.float32 and got["nn"].shape == got["nn_dist"].shape
    assert np.array_equal(got["nn"], want["nn"])
    assert (got["acc"], got["acc_sample"], got["acc_ref"]) == (want["acc"], want["acc_sample"], want["acc_ref"])


# ------------------------------------------------------------------------------------------------ the self matrix
@pytest.mark.parametrize("S,M", SELF_CASES)
def test_self_matrix_is_the_existing_op_bit_for_bit(S, M):
    PC = _PC()
    x = put(_set(S, M))
    upper = torch.ones(S, S, dtype=torch.bool, device=DEV).triu()
    for normalize, use_sqrt in FLAGS:
        J = PC.chamfer_matrix_self(x, normalize=normalize, use_sqrt=use_sqrt)
        assert J.shape == (S, S) and J.dtype == torch.float32 and J.is_contiguous()
        D = PC.chamfer_matrix(x, x, normalize=normalize, use_sqrt=use_sqrt)
        assert torch.equal(J[upper], D[upper])
        assert torch.equal(J, J.T)
        assert torch.equal(J.diagonal(), torch.zeros(S, device=DEV))
        whole = torch.equal(J, D)
        print("chamfer_matrix_self (%d, %d) normalize=%s use_sqrt=%s: the whole matrix equals chamfer_matrix(x, x): %s"
              % (S, M, normalize, use_sqrt, whole))
        assert whole  # (for M = N the pair's arithmetic is symmetric in its two clouds)


@pytest.mark.parametrize("normalize,use_sqrt", FLAGS)
def test_slabs_change_no_bit(monkeypatch, normalize, use_sqrt):
    """(7, 33): four folded rows, one per launch"""
    PC = _PC()
    S, M = 7, 33
    x = put(_set(S, M))
    whole = PC.chamfer_matrix_self(x, normalize=normalize, use_sqrt=use_sqrt)
    calls = []
    real = PC._lib.call
    monkeypatch.setattr(PC._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(PC, "MATRIX_POINT_PAIRS_PER_LAUNCH", (S + 1) * M * M)
    slabs = PC.chamfer_matrix_self(x, normalize=normalize, use_sqrt=use_sqrt)
    assert calls.count("sivae_chamfer_matrix_self") == 4
    assert torch.equal(slabs, whole)


@pytest.mark.parametrize("S,M", [(5, 33), (2, 2053)])
def test_layouts_change_no_bit(S, M):
    """the [S, M, 3] view of [S, 3, M] storage (a decoder output's transpose(1, 2)), read in place"""
    PC = _PC()
    x = put(_set(S, M))
    v = x.permute(0, 2, 1).contiguous().transpose(1, 2)
    assert not v.is_contiguous() and v.stride(2) == M
    assert torch.equal(PC.chamfer_matrix_self(v), PC.chamfer_matrix_self(x))
    assert torch.equal(PC.chamfer_matrix_self(put(_set(S, M), misaligned=True)), PC.chamfer_matrix_self(x))


@pytest.mark.parametrize("S,M", [(70, 8), (2, 2053)])
def test_two_runs_are_bit_identical(S, M):
    PC = _PC()
    x = put(_set(S, M))
    for normalize, use_sqrt in FLAGS:
        J = PC.chamfer_matrix_self(x, normalize, use_sqrt)
        assert torch.equal(J, PC.chamfer_matrix_self(x, normalize, use_sqrt))
        assert torch.equal(J, PC.chamfer_matrix(x, x, normalize, use_sqrt))  # (blocks that walk more than one unit)


@pytest.mark.parametrize("normalize,use_sqrt", FLAGS)
def test_a_non_finite_coordinate_stays_in_its_row_and_column(normalize, use_sqrt):
    PC, E = _PC(), _E()
    S, M = 5, 33
    x = np.array(_set(S, M))
    clean = PC.chamfer_matrix_self(put(x), normalize, use_sqrt)
    x[2, 17, 1] = np.nan
    J = PC.chamfer_matrix_self(put(x), normalize, use_sqrt)
    bad = torch.zeros(S, S, dtype=torch.bool, device=DEV)
    bad[2, :] = True
    bad[:, 2] = True
    assert torch.equal(~torch.isfinite(J), bad)
    assert torch.equal(J[~bad], clean[~bad])
    with pytest.raises(ValueError, match="non-finite"):
        E.one_nn_accuracy(x, np.array(_set(S, M)), normalize=normalize, use_sqrt=use_sqrt)
    with pytest.raises(ValueError, match="non-finite"):
        E.one_nn_accuracy(None, None, dist=clean, dist_ss=clean, dist_rr=J)


# ------------------------------------------------------------------------------------------------ nn1_loo
def _sym(rng, n):
    A = (rng.random((n, n)) + 0.01).astype(np.float32)
    return np.triu(A) + np.triu(A, 1).T


@pytest.mark.parametrize("S,R", [(1, 1), (1, 6), (6, 1), (7, 5), (64, 63), (130, 70)])
def test_nn1_loo_against_the_oracle(S, R):
    """random positive float32 matrices, Dss and Drr symmetric; whatever the diagonals hold changes nothing"""
    PC = _PC()
    rng = np.random.default_rng(S * 1009 + R)
    Dss, Dsr, Drr = _sym(rng, S), (rng.random((S, R)) + 0.01).astype(np.float32), _sym(rng, R)
    val64, arg64 = NO.nn1_loo(Dss, Dsr, Drr)
    joint = np.block([[Dss, Dsr], [Dsr.T, Drr]])
    first = None
    for d in (None, 0.0, -1.0, NAN):
        A, B = Dss.copy(), Drr.copy()
        if d is not None:
            np.fill_diagonal(A, d)
            np.fill_diagonal(B, d)
        val, arg = PC.nn1_loo(put(A), put(Dsr), put(B))
        assert val.shape == (S + R,) and val.dtype == torch.float32 and arg.shape == (S + R,) and arg.dtype == torch.int32
        arg, val = arg.cpu().numpy(), val.cpu().numpy()
        assert np.array_equal(arg, arg64), d
        assert np.array_equal(val, joint[np.arange(S + R), arg]), d       # (bit-equal to the chosen entry)
        first = (val, arg) if first is None else first
        assert np.array_equal(val, first[0]) and np.array_equal(arg, first[1])
    assert np.array_equal(val.astype(np.float64), val64)


def test_nn1_loo_special_cases():
    PC = _PC()

    def run(Dss, Dsr, Drr):
        mats = [np.array(D, dtype=np.float32) for D in (Dss, Dsr, Drr)]
        val, arg = PC.nn1_loo(*(put(D) for D in mats))
        val64, arg64 = NO.nn1_loo(*mats)
        assert np.array_equal(arg.cpu().numpy(), arg64) and np.array_equal(val.cpu().numpy().astype(np.float64), val64)
        return arg.tolist(), val.tolist()

    # the matrices of tests/test_pc_nna_host.py::test_oracle_against_hand_computed_matrices, in its order: plain;
    # ties between a candidate of each set (the lowest joint index); +inf / NaN that never win and an item with no
    # candidate left; a non-symmetric Dss (item t reads ROW t)
    assert run([[0, 5], [5, 0]], [[2, 7], [9, 1]], [[0, 4], [4, 0]]) == ([2, 3, 0, 1], [2.0, 1.0, 2.0, 1.0])
    assert run([[0, 3], [3, 0]], [[3, 8], [9, 6]], [[0, 6], [6, 0]]) == ([1, 0, 0, 1], [3.0, 3.0, 3.0, 6.0])
    assert run([[0, INF], [INF, 0]], [[4, NAN], [NAN, INF]], [[0, 5], [5, 0]]) == ([2, -1, 0, 2], [4.0, INF, 4.0, 5.0])
    assert run([[0, 1], [8, 0]], [[5], [2]], [[0]]) == ([1, 2, 1], [1.0, 2.0, 2.0])
    # a tie INSIDE a set: items 3, 67 (the same lane's second step) and 70 (another lane) of 80 samples at one distance
    S, R = 80, 3
    Dss = np.full((S, S), 9.0, dtype=np.float32)
    Dss[0, 70] = Dss[0, 67] = Dss[0, 3] = 2.0
    Dsr = np.full((S, R), 9.0, dtype=np.float32)
    Dsr[0, 1] = 2.0                                     # (and the same distance again in the other set: item 81)
    Drr = np.full((R, R), 9.0, dtype=np.float32)
    arg, val = run(Dss, Dsr, Drr)
    assert arg[0] == 3 and val[0] == 2.0 and arg[1] == 0 and arg[S + 1] == 0 and val[S + 1] == 2.0
    # every candidate non-finite: (+inf, -1) for every item
    arg, val = run(np.full((3, 3), NAN), np.full((3, 2), INF), np.full((2, 2), NAN))
    assert arg == [-1] * 5 and val == [INF] * 5
    # S = R = 1: each item has the other only; with a NaN between them, none
    assert run([[0]], [[7]], [[0]]) == ([1, 0], [7.0, 7.0])
    assert run([[0]], [[NAN]], [[0]]) == ([-1, -1], [INF, INF])
    # larger than a wave and a block on either side, many equal entries: ties between lanes
    g = np.random.default_rng(11)
    S, R = 333, 200
    A = g.integers(1, 40, size=(S, S)).astype(np.float32)
    B = g.integers(1, 40, size=(R, R)).astype(np.float32)
    C = g.integers(1, 40, size=(S, R)).astype(np.float32)
    arg, val = run(A, C, B)                             # (not symmetric: the row rule)
    r2 = PC.nn1_loo(put(A), put(C), put(B))
    assert r2[1].tolist() == arg and r2[0].tolist() == val


# ------------------------------------------------------------------------------------------------ the metric
@pytest.mark.parametrize("seed,S,R,M,N", METRIC_CASES)
def test_one_nn_accuracy_against_the_oracle(seed, S, R, M, N):
    E = _E()
    sample, ref, want = _metric_case(seed, S, R, M, N)
    got = E.one_nn_accuracy(put(sample), put(ref))
    print("1-NNA %s: acc %.4f acc_sample %.4f acc_ref %.4f" % ((seed, S, R, M, N), got["acc"], got["acc_sample"], got["acc_ref"]))
    _same(got, want)
    assert np.all(np.abs(got["nn_dist"] - want["nn_dist"]) <= 1e-5 * want["nn_dist"])


def test_precomputed_matrices_and_host_inputs_give_the_same():
    E, PC = _E(), _PC()
    seed, S, R, M, N = METRIC_CASES[0]
    sample, ref, want = _metric_case(seed, S, R, M, N)
    sd, rd = put(sample), put(ref)
    base = E.one_nn_accuracy(sd, rd)
    _same(base, want)
    Dss, Dsr, Drr = E.chamfer_matrix_self(sd), E.chamfer_matrix(sd, rd), E.chamfer_matrix_self(np.array(ref))
    assert torch.equal(Dss, PC.chamfer_matrix(sd, sd)) and torch.equal(Drr, PC.chamfer_matrix(rd, rd))
    for args, kw in (((None, None), dict(dist=Dsr, dist_ss=Dss, dist_rr=Drr)),
                     ((None, None), dict(dist=Dsr.cpu().numpy(), dist_ss=Dss.cpu().numpy(), dist_rr=Drr.cpu())),
                     ((sd, rd), dict(dist=Dsr)),                      # (the matrix MMD and COV were given)
                     ((np.array(sample), np.array(ref)), {}),
                     ((torch.from_numpy(np.array(sample)), rd), {})):
        r = E.one_nn_accuracy(*args, **kw)
        _same(r, base)
        assert np.array_equal(r["nn_dist"], base["nn_dist"])
    mmd, _ = E.minimum_mathing_distance(sd, rd, dist=Dsr)             # one cross matrix serves all three figures
    assert mmd == E.minimum_mathing_distance(sd, rd)[0]
    # the flags reach the matrices
    for normalize, use_sqrt in FLAGS[1:]:
        _, _, want = _metric_case(seed, S, R, M, N, normalize, use_sqrt)
        _same(E.one_nn_accuracy(sd, rd, normalize=normalize, use_sqrt=use_sqrt), want)
    with pytest.raises(ValueError, match=r"dist_ss \[S, S\]"):
        E.one_nn_accuracy(sd, rd, dist_ss=Drr)


def test_exact_figures():
    """a set against itself: every cloud's twin in the other set is at distance 0 and nothing else is -> exactly 0;
    against itself moved by 10: exactly 1"""
    E = _E()
    x = put(_set(6, 40))
    r = E.one_nn_accuracy(x, x)
    assert (r["acc"], r["acc_sample"], r["acc_ref"]) == (0.0, 0.0, 0.0) and not r["nn_dist"].any()
    assert np.array_equal(r["nn"], np.concatenate([np.arange(6, 12), np.arange(6)]))
    r = E.one_nn_accuracy(x, x + 10)
    assert (r["acc"], r["acc_sample"], r["acc_ref"]) == (1.0, 1.0, 1.0)


def test_emd_metric_against_the_oracle():
    """metric="emd": three whole emd_matrix calls (the approximate matching is not symmetric; item t reads its row)"""
    from test_pc_emd_gpu import _gate                  # (the gap tests/test_pc_emd_gpu.py asks of its own argmin checks)
    E = _E()
    seed, S, R, N = EMD_CASE
    sample, ref = _two_sets(seed, S, R, N, N)
    mats = [MO.emd_matrix(a, b) for a, b in ((sample, sample), (sample, ref), (ref, ref))]
    gap = NO.smallest_gap(*mats)
    print("1-NNA (emd) case %s: smallest gap %.2e, required %.2e" % (EMD_CASE, gap, 100 * _gate()))
    assert gap >= 100 * _gate(), "gap %.2e: float32 cannot be asked for the float64 neighbour" % gap
    want = NO.one_nn_accuracy(*mats)
    got = E.one_nn_accuracy(put(sample), put(ref), metric="emd")
    _same(got, want)
    assert np.all(np.abs(got["nn_dist"] - want["nn_dist"]) <= _gate() * want["nn_dist"])
    sd, rd = put(sample), put(ref)
    again = E.one_nn_accuracy(None, None, metric="emd", dist=E.emd_matrix(sd, rd), dist_ss=E.emd_matrix(sd, sd),
                              dist_rr=E.emd_matrix(rd, rd))
    _same(again, got)
    assert np.array_equal(again["nn_dist"], got["nn_dist"])


# ------------------------------------------------------------------------------------------------ guarded
def test_guarded():
    """on guarded, poisoned outputs and exact workspaces: nothing written outside a tensor, no element left at the poison
    value (0xFF bytes: NaN as float32, -1 as int32), the unguarded results"""
    from sivae_hip import ops, pointcloud
    from support.guard import describe, guarded
    sets = [put(_set(5, 33)), put(_set(2, 2053))]
    J0 = [pointcloud.chamfer_matrix_self(x) for x in sets]
    rng = np.random.default_rng(5)
    mats = [put(_sym(rng, 7)), put((rng.random((7, 5)) + 0.01).astype(np.float32)), put(_sym(rng, 5))]
    n0 = pointcloud.nn1_loo(*mats)
    for modules in ((pointcloud,), (pointcloud, ops)):  # (`workspace` is ops' name: with ops it has exactly its stated size)
        with guarded(*modules) as g:
            J1 = [pointcloud.chamfer_matrix_self(x) for x in sets]
            n1 = pointcloud.nn1_loo(*mats)
            damage = g.verify()
            assert not damage, "guard damage:\n%s" % describe(damage)
        for a, b in zip(J1, J0):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        assert bool(torch.isfinite(n1[0]).all()) and int(n1[1].min()) >= 0 and int(n1[1].max()) < 12
        assert torch.equal(n1[0], n0[0]) and torch.equal(n1[1], n0[1])
