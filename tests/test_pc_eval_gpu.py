"""GPU checks of the 3-D variant's set-to-set evaluation: sivae_chamfer_matrix / sivae_match_min (csrc/pc_eval.hip),
sivae_hip.pointcloud.chamfer_matrix / match_min and the drop-in soft_intro_vae_3d/metrics/evaluation_metrics.py, against
the float64 restatement tests/pc3d_eval_oracle.py on the same float32 inputs.

Matrix gate: |D - D64| <= 1e-5 |D64| element-wise, the bound tests/test_pointcloud_gpu.py holds chamfer_fwd to (the
worst figure of every case is printed; DESIGN.md "Point clouds" lists what was measured).

Shapes (S, R, M, N) and what each covers (a lane keeps 8 query points, a block 2048; 1024 reference points are staged)
  (3, 5, 33, 70)      ragged everything: one pair of queries per lane, most lanes empty, a tail of 2 reference points
  (1, 1, 1, 1)        one point against one
  (2, 3, 2053, 300)   sample cloud beyond one register set: a second query chunk of 5 points, column minima kept in LDS
  (3, 2, 300, 2053)   reference cloud beyond one LDS chunk: three chunks, row minima kept in registers across them
  (1, 2, 2053, 1030)  both: the column minima rest in the workspace between the query chunks
  (70, 130, 8, 8)     9100 pairs on 2048 blocks: blocks walk 4 or 5 pairs, rows and columns of D cross block strides
  (300, 300, 4, 4)    90 000 pairs, past any 65 535 grid limit
  (2, 2, 700, 64), (2, 2, 1300, 64)   two and three pairs of queries per lane (the other instances of the scan)
"""
import functools

import numpy as np
import pytest
import torch

import pc3d_eval_oracle as EO
from support.pc import DEV, _PC, put

pytestmark = pytest.mark.gpu
TOL = 1e-5
CASES = [(3, 5, 33, 70), (1, 1, 1, 1), (2, 3, 2053, 300), (3, 2, 300, 2053), (1, 2, 2053, 1030), (70, 130, 8, 8),
         (300, 300, 4, 4), (2, 2, 700, 64), (2, 2, 1300, 64)]
FLAGS = [(True, False), (True, True), (False, False), (False, True)]  # (normalize, use_sqrt)
# (seed, S, R, M, N) of the metric checks: the generator asserts the argmin gap of each
METRIC_CASES = [(2024, 6, 9, 40, 55), (2025, 9, 6, 55, 40), (2026, 12, 5, 33, 70)]
MIN_GAP = 1e-4


def _E():
    import soft_intro_vae_3d.metrics.evaluation_metrics as E
    return E


@functools.lru_cache(maxsize=None)
def _clouds(S, R, M, N, seed=None):
    """float32 numpy inputs (never modified by a test): PCG64, uniform in the cube of side 1 about the origin"""
    rng = np.random.default_rng(S * 1000003 + R * 10007 + M * 101 + N if seed is None else seed)
    sample = (rng.random((S, M, 3)) - 0.5).astype(np.float32)
    ref = (rng.random((R, N, 3)) - 0.5).astype(np.float32)
    sample.setflags(write=False)
    ref.setflags(write=False)
    return sample, ref


@functools.lru_cache(maxsize=None)
def _ref(S, R, M, N, normalize, use_sqrt, seed=None):
    D = EO.chamfer_matrix(*_clouds(S, R, M, N, seed), normalize=normalize, use_sqrt=use_sqrt)
    D.setflags(write=False)
    return D


def _worst(D, D64):
    """largest |D - D64| / |D64| (0 / 0 counts as 0: an exact zero must be met exactly)"""
    D = D.double().cpu().numpy()
    assert np.isfinite(D).all()
    err = np.abs(D - D64)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(err == 0, 0.0, err / np.abs(D64))
    return float(rel.max())


@pytest.mark.parametrize("normalize,use_sqrt", FLAGS)
@pytest.mark.parametrize("S,R,M,N", CASES)
def test_matrix_parity(S, R, M, N, normalize, use_sqrt):
    PC = _PC()
    sample, ref = _clouds(S, R, M, N)
    D = PC.chamfer_matrix(put(sample), put(ref), normalize=normalize, use_sqrt=use_sqrt)
    assert D.shape == (S, R) and D.dtype == torch.float32 and D.is_contiguous()
    w = _worst(D, _ref(S, R, M, N, normalize, use_sqrt))
    print("chamfer_matrix (%d, %d, %d, %d) normalize=%s use_sqrt=%s: worst relative error %.3e"
          % (S, R, M, N, normalize, use_sqrt, w))
    assert w <= TOL


@pytest.mark.parametrize("normalize,use_sqrt", FLAGS)
def test_slabs_change_no_bit(monkeypatch, normalize, use_sqrt):
    """(3, 5, 33, 70) in three launches of one row each"""
    PC = _PC()
    S, R, M, N = 3, 5, 33, 70
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    whole = PC.chamfer_matrix(sample, ref, normalize=normalize, use_sqrt=use_sqrt)
    calls = []
    real = PC._lib.call
    monkeypatch.setattr(PC._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    monkeypatch.setattr(PC, "MATRIX_POINT_PAIRS_PER_LAUNCH", R * M * N)
    slabs = PC.chamfer_matrix(sample, ref, normalize=normalize, use_sqrt=use_sqrt)
    assert calls.count("sivae_chamfer_matrix") == 3
    assert torch.equal(slabs, whole)


def test_same_set_on_both_sides_has_an_exact_zero_diagonal():
    PC = _PC()
    x = put(_clouds(4, 4, 256, 256)[0])
    for normalize, use_sqrt in FLAGS:
        D = PC.chamfer_matrix(x, x, normalize=normalize, use_sqrt=use_sqrt)
        assert torch.equal(D.diagonal(), torch.zeros(4, device=DEV))
        off = D[~torch.eye(4, dtype=torch.bool, device=DEV)]
        assert bool((off > 0).all())
        assert _worst(D, EO.chamfer_matrix(x.cpu().numpy(), x.cpu().numpy(), normalize, use_sqrt)) <= TOL


@pytest.mark.parametrize("B,M,N", [(4, 300, 260), (2, 2053, 1030)])
def test_diagonal_agrees_with_the_training_kernel(B, M, N):
    """D[b, b] without normalisation is chamfer_fwd's loss[b]: other summation order, so 1e-5 and no bit equality"""
    PC = _PC()
    sample, ref = (put(a) for a in _clouds(B, B, M, N))
    D = PC.chamfer_matrix(sample, ref, normalize=False)
    loss = PC.chamfer_fwd(sample, ref)[0]
    rel = ((D.diagonal().double() - loss.double()).abs() / loss.double()).max()
    print("chamfer_matrix diagonal vs chamfer_fwd [%d, %d, %d]: worst relative difference %.3e" % (B, M, N, float(rel)))
    assert float(rel) <= TOL


def _transposed_view(a):
    """the [S, N, 3] view of [S, 3, N] storage: what evaluation/generate_data_for_metrics.py's transpose_(1, 2) yields"""
    v = put(a).permute(0, 2, 1).contiguous().transpose(1, 2)
    assert not v.is_contiguous() and v.stride(2) == a.shape[1]
    return v


@pytest.mark.parametrize("S,R,M,N", [(3, 5, 33, 70), (2, 3, 2053, 300)])
def test_layouts_change_no_bit(S, R, M, N):
    PC = _PC()
    sample, ref = _clouds(S, R, M, N)
    base = PC.chamfer_matrix(put(sample), put(ref))
    for name, s, r in (("sample transposed", _transposed_view(sample), put(ref)),
                       ("ref transposed", put(sample), _transposed_view(ref)),
                       ("both transposed", _transposed_view(sample), _transposed_view(ref)),
                       ("sample misaligned", put(sample, misaligned=True), put(ref)),
                       ("ref misaligned", put(sample), put(ref, misaligned=True))):
        assert torch.equal(PC.chamfer_matrix(s, r), base), name


@pytest.mark.parametrize("S,R,M,N", [(3, 5, 33, 70), (1, 2, 2053, 1030), (70, 130, 8, 8)])
def test_two_runs_are_bit_identical(S, R, M, N):
    PC = _PC()
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    for normalize, use_sqrt in FLAGS:
        assert torch.equal(PC.chamfer_matrix(sample, ref, normalize, use_sqrt),
                           PC.chamfer_matrix(sample, ref, normalize, use_sqrt))


@pytest.mark.parametrize("normalize,use_sqrt", FLAGS)
def test_non_finite_coordinates_stay_in_their_row_and_column(normalize, use_sqrt):
    PC, E = _PC(), _E()
    S, R, M, N = 3, 5, 33, 70
    sample, ref = (np.array(a) for a in _clouds(S, R, M, N))
    clean = PC.chamfer_matrix(put(sample), put(ref), normalize, use_sqrt)
    sample[1, 17, 2] = np.nan
    ref[3, 69, 0] = np.inf
    D = PC.chamfer_matrix(put(sample), put(ref), normalize, use_sqrt)
    bad = torch.zeros(S, R, dtype=torch.bool, device=DEV)
    bad[1, :] = True
    bad[:, 3] = True
    assert torch.equal(~torch.isfinite(D), bad)
    assert torch.equal(D[~bad], clean[~bad])
    want = np.isnan(EO.chamfer_matrix(sample, ref, normalize, use_sqrt))
    assert np.array_equal(want, bad.cpu().numpy())
    for f in (E.minimum_mathing_distance, E.coverage):
        with pytest.raises(ValueError, match="non-finite"):
            f(sample, ref, normalize=normalize, use_sqrt=use_sqrt)
        with pytest.raises(ValueError, match="non-finite"):
            f(None, None, dist=D)


def test_match_min():
    PC = _PC()
    inf = float("inf")
    # planted equal minima: rows 0 and 2 hold theirs twice, columns 1 and 2 too
    D = torch.tensor([[3.0, 1.0, 1.0, 7.0],
                      [2.0, 5.0, 2.5, 2.0],
                      [9.0, 1.0, 1.0, 8.0]], device=DEV)
    rm, ra, cm, ca = PC.match_min(D)
    assert ra.dtype == torch.int32 and ca.dtype == torch.int32
    assert rm.tolist() == [1.0, 2.0, 1.0] and ra.tolist() == [1, 0, 1]
    assert cm.tolist() == [2.0, 1.0, 1.0, 2.0] and ca.tolist() == [1, 0, 0, 1]
    # a row of +inf (and with it +inf in every column), a NaN that must not win
    D = torch.tensor([[inf, inf, inf], [4.0, float("nan"), 6.0], [inf, inf, inf]], device=DEV)
    rm, ra, cm, ca = PC.match_min(D)
    assert rm.tolist() == [inf, 4.0, inf] and ra.tolist() == [0, 0, 0]
    assert cm.tolist() == [4.0, inf, 6.0] and ca.tolist() == [1, 0, 1]
    # S = 1 and R = 1
    rm, ra, cm, ca = PC.match_min(torch.tensor([[5.0, 2.0, 2.0, 9.0]], device=DEV))
    assert (rm.tolist(), ra.tolist(), cm.tolist(), ca.tolist()) == ([2.0], [1], [5.0, 2.0, 2.0, 9.0], [0, 0, 0, 0])
    rm, ra, cm, ca = PC.match_min(torch.tensor([[5.0], [2.0], [2.0]], device=DEV))
    assert (rm.tolist(), ra.tolist(), cm.tolist(), ca.tolist()) == ([5.0, 2.0, 2.0], [0, 0, 0], [2.0], [1])
    # larger than one wave / one block on either side, ties between lanes and between waves: numpy's argmin
    g = np.random.default_rng(7)
    A = g.integers(0, 50, size=(333, 517)).astype(np.float32)   # (many equal entries)
    rm, ra, cm, ca = PC.match_min(put(A))
    assert np.array_equal(ra.cpu().numpy(), A.argmin(axis=1)) and np.array_equal(rm.cpu().numpy(), A.min(axis=1))
    assert np.array_equal(ca.cpu().numpy(), A.argmin(axis=0)) and np.array_equal(cm.cpu().numpy(), A.min(axis=0))
    r2 = PC.match_min(put(A))
    assert all(torch.equal(x, y) for x, y in zip((rm, ra, cm, ca), r2))


@functools.lru_cache(maxsize=None)
def _metric_case(seed, S, R, M, N, normalize, use_sqrt=False):
    """-> (sample, ref, D64); asserts in float64 that every row and column of D64 tells its best from its second best"""
    sample, ref = _clouds(S, R, M, N, seed)
    D64 = _ref(S, R, M, N, normalize, use_sqrt, seed)
    gap = EO.smallest_gap(D64)
    assert gap >= MIN_GAP, "case %s: argmin gap %.2e — float32 cannot be asked for the float64 argmin" % (
        (seed, S, R, M, N, normalize), gap)
    return sample, ref, D64


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("seed,S,R,M,N", METRIC_CASES)
def test_mmd_and_cov_against_the_oracle(seed, S, R, M, N, normalize):
    E = _E()
    sample, ref, D64 = _metric_case(seed, S, R, M, N, normalize)
    mmd64, matched64, arg64 = EO.minimum_matching_distance(D64)
    cov64, ref64, dist64 = EO.coverage(D64)
    sd, rd = put(sample), put(ref)
    mmd, matched = E.minimum_mathing_distance(sd, rd, normalize=normalize)
    cov, matched_ref, matched_dist = E.coverage(sd, rd, normalize=normalize, ret_dist=True)
    assert isinstance(mmd, float) and isinstance(cov, float)
    assert isinstance(matched, np.ndarray) and matched.shape == (R,) and matched.dtype == np.float32
    assert isinstance(matched_ref, np.ndarray) and matched_ref.shape == (S,) and matched_ref.dtype.kind == "i"
    assert abs(mmd - mmd64) <= TOL * mmd64
    assert np.all(np.abs(matched - matched64) <= TOL * matched64)
    assert np.all(np.abs(matched_dist - dist64) <= TOL * dist64)
    assert np.array_equal(matched_ref, ref64)
    assert cov == cov64
    D = E.chamfer_matrix(sd, rd, normalize=normalize)
    assert np.array_equal(_PC().match_min(D)[3].cpu().numpy(), arg64)  # (the sample behind each matched distance)
    assert len(E.coverage(sd, rd, normalize=normalize)) == 2
    assert E.minimum_matching_distance(sd, rd, normalize=normalize)[0] == mmd
    # a precomputed matrix, numpy arrays, CPU tensors, a mixed pair: the same results
    for kw in (dict(dist=D), dict(dist=D.cpu().numpy())):
        m2, d2 = E.minimum_mathing_distance(sd, rd, **kw)
        c2, r2 = E.coverage(sd, rd, **kw)
        assert m2 == mmd and np.array_equal(d2, matched) and c2 == cov and np.array_equal(r2, matched_ref)
    for a, b in ((np.array(sample), np.array(ref)), (torch.from_numpy(np.array(sample)), torch.from_numpy(np.array(ref))),
                 (sd, np.array(ref))):
        m2, d2 = E.minimum_mathing_distance(a, b, normalize=normalize, batch_size=100, sess=object(), verbose=True)
        c2, r2 = E.coverage(a, b, normalize=normalize, batch_size=100, sess=None, verbose=True)
        assert m2 == mmd and np.array_equal(d2, matched) and c2 == cov and np.array_equal(r2, matched_ref)


def test_identical_sets():
    E = _E()
    x = put(_clouds(6, 9, 40, 55, 2024)[0])
    mmd, matched = E.minimum_mathing_distance(x, x)
    cov, matched_ref = E.coverage(x, x)
    assert mmd == 0.0 and not matched.any()
    assert cov == 1.0 and np.array_equal(matched_ref, np.arange(6))
    with pytest.raises(NotImplementedError):
        E.coverage(x, x, use_EMD=True)


@pytest.mark.parametrize("S,R,M,N", [(3, 5, 33, 70), (2, 3, 2053, 300), (1, 2, 2053, 1030)])
def test_guarded(S, R, M, N):
    """on guarded, poisoned outputs and exact workspaces: nothing written outside a tensor, no element left at the poison
    value (0xFF bytes: NaN as float32, -1 as int32), the unguarded results"""
    from sivae_hip import ops, pointcloud
    from support.guard import describe, guarded
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    D0 = pointcloud.chamfer_matrix(sample, ref)
    m0 = pointcloud.match_min(D0)
    with guarded(pointcloud) as g:  # (pointcloud's names only: its torch; `workspace` is ops' and needs ops in the list)
        D1 = pointcloud.chamfer_matrix(sample, ref)
        m1 = pointcloud.match_min(D1)
        damage = g.verify()
        assert not damage, "guard damage:\n%s" % describe(damage)
    with guarded(pointcloud, ops) as g:  # (and with the workspace at exactly its stated size)
        D2 = pointcloud.chamfer_matrix(sample, ref)
        m2 = pointcloud.match_min(D2)
        damage = g.verify()
        assert not damage, "guard damage:\n%s" % describe(damage)
    for D, m in ((D1, m1), (D2, m2)):
        assert bool(torch.isfinite(D).all()) and torch.equal(D, D0)
        assert bool(torch.isfinite(m[0]).all()) and bool(torch.isfinite(m[2]).all())
        assert int(m[1].min()) >= 0 and int(m[1].max()) < R and int(m[3].min()) >= 0 and int(m[3].max()) < S
        assert all(torch.equal(x, y) for x, y in zip(m, m0))
