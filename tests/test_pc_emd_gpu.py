"""GPU checks of the 3-D variant's earth mover's evaluation: sivae_emd_matrix (csrc/pc_emd.hip),
sivae_hip.pointcloud.emd_matrix and the drop-in soft_intro_vae_3d/metrics/evaluation_metrics.py::emd_matrix, against the
float64 restatement tests/pc3d_emd_oracle.py on the same float32 inputs.  Clouds are seeded PCG64, uniform in the cube of
side 1 about the origin, except where said.

Gate: |D - D64| <= GATE |D64| per entry, GATE = 16 x the worst such error of the FLOAT32 ORACLE over the value cases below,
computed here (the yardstick is the restatement, never the kernel; the factor covers the hardware exp2 and sqrt, flushed
denormals and another summation shape).  DESIGN.md "Point clouds" lists what was measured.

Value cases (M sample points, N reference points, S, R) and what each covers (512 threads own up to 8 points of either
cloud each, in 1 .. 4 register pairs; both clouds are staged whole in LDS, (M + N) 16 bytes of it):
  (1, 1)  (1, 9)  (5, 7)  (64, 64)     one point; fewer points than lanes of a wave; one wave
  (255, 257)  (257, 300)               most of the block idle, ragged on both sides
  (1025, 2049)  (2049, 1025)           two and three register pairs on either side, a ragged last one
  (4096, 3)  (3, 3073)                 the fourth register pair on either side; just past 64 KB of LDS
  (5, 7) and (257, 300) again without normalisation
"""
import functools

import numpy as np
import pytest
import torch

import pc3d_emd_oracle as MO
import pc3d_eval_oracle as EO
from support.pc import DEV, _PC, put

pytestmark = pytest.mark.gpu
# (M, N, S, R, normalize)
VALUE_CASES = [(1, 1, 2, 3, True), (1, 9, 2, 3, True), (5, 7, 2, 3, True), (64, 64, 2, 3, True), (255, 257, 2, 3, True),
               (257, 300, 2, 3, True), (1025, 2049, 1, 1, True), (2049, 1025, 1, 1, True), (4096, 3, 2, 3, True),
               (3, 3073, 1, 1, True), (5, 7, 2, 3, False), (257, 300, 2, 3, False)]


def _E():
    import soft_intro_vae_3d.metrics.evaluation_metrics as E
    return E


@functools.lru_cache(maxsize=None)
def _clouds(S, R, M, N, seed=None):
    """float32 numpy inputs (never modified by a test)"""
    rng = np.random.default_rng(S * 1000003 + R * 10007 + M * 101 + N if seed is None else seed)
    sample = (rng.random((S, M, 3)) - 0.5).astype(np.float32)
    ref = (rng.random((R, N, 3)) - 0.5).astype(np.float32)
    sample.setflags(write=False)
    ref.setflags(write=False)
    return sample, ref


@functools.lru_cache(maxsize=None)
def _ref(S, R, M, N, normalize, seed=None, dtype=np.float64):
    D = MO.emd_matrix(*_clouds(S, R, M, N, seed), normalize=normalize, dtype=dtype)
    D.setflags(write=False)
    return D


def _rel(D, D64):
    return float((np.abs(np.asarray(D, dtype=np.float64) - D64) / D64).max())


@functools.lru_cache(maxsize=None)
def _gate():
    """16 x the worst relative error of the float32 oracle against the float64 oracle over VALUE_CASES"""
    worst = max(_rel(_ref(S, R, M, N, nz, None, np.float32), _ref(S, R, M, N, nz)) for M, N, S, R, nz in VALUE_CASES)
    assert 0 < worst < 1e-5, worst
    print("float32 oracle against float64 oracle, worst relative error %.3e -> gate %.3e" % (worst, 16 * worst))
    return 16 * worst


def _host(D):
    D = D.double().cpu().numpy()
    assert np.isfinite(D).all()
    return D


@pytest.mark.parametrize("M,N,S,R,normalize", VALUE_CASES)
def test_values_against_the_float64_oracle(M, N, S, R, normalize):
    PC = _PC()
    sample, ref = _clouds(S, R, M, N)
    D = PC.emd_matrix(put(sample), put(ref), normalize=normalize)
    assert D.shape == (S, R) and D.dtype == torch.float32 and D.is_contiguous()
    w = _rel(_host(D), _ref(S, R, M, N, normalize))
    print("emd_matrix M=%d N=%d S=%d R=%d normalize=%s: worst relative error %.3e (gate %.3e)"
          % (M, N, S, R, normalize, w, _gate()))
    assert w <= _gate()


def _diameter(x):
    """largest distance between two points of x [n, 3] (float64)"""
    x = np.asarray(x, dtype=np.float64)
    best = 0.0
    for i in range(0, len(x), 512):
        d = x[i:i + 512, None, :] - x[None, :, :]
        best = max(best, float((d * d).sum(axis=2).max()))
    return float(np.sqrt(best))


RESOLVED_GAP = 0.03     # sqrt(20 ln 2 / 16384): two points that far apart weigh 2^-20 at the first level


def _closest_pair(x):
    """smallest distance between two different points of x [n, 3] (float64)"""
    x = np.asarray(x, dtype=np.float64)
    best = np.inf
    for i in range(0, len(x), 512):
        d = x[i:i + 512, None, :] - x[None, :, :]
        d2 = (d * d).sum(axis=2)
        d2[np.arange(d2.shape[0]), i + np.arange(d2.shape[0])] = np.inf
        best = min(best, float(d2.min()))
    return float(np.sqrt(best))


@pytest.mark.parametrize("how", ["identical", "permuted"])
@pytest.mark.parametrize("n,side", [(64, 1.0), (64, 16.0), (2048, 16.0)])
def test_a_cloud_against_itself(n, side, how):
    """normalised D <= 1e-5 x the cloud's diameter, for a cloud against itself and against a permutation of itself.

    The bound rests on ten levels each misplacing at most about 2^-20 of a point's mass, no farther than a diameter away.
    That presupposes that the FIRST level tells the cloud's points apart: its weight exp(-16384 d2) between two different
    points must itself be about 2^-20 or less, i.e. the closest pair at least sqrt(20 ln 2 / 16384) = 0.03 apart (asserted
    below from the inputs alone).  64 points uniform in the unit cube are that far apart (0.046).  2048 points in the unit
    cube are not (closest pair 0.002, weight 0.94): neighbours share mass BY THE DEFINITION, the float64 oracle itself
    gives 3.248e-5 against a bound of 1.61e-5 (1.77e-5 against 1.59e-5 at 1024 points), and no implementation of the
    definition can meet the bound there.  The bound is therefore asked of 2048 points in the cube of side 16 (closest pair
    0.063), and the dense 2048-point unit-cube cloud is held to the float64 oracle in
    test_a_dense_cloud_against_itself_matches_the_oracle."""
    PC = _PC()
    x = np.float32(side) * _clouds(1, 1, n, n, 9000 + n)[0]
    gap = _closest_pair(x[0])
    assert gap >= RESOLVED_GAP, "closest pair %.4f: the first level does not resolve this cloud" % gap
    y = x[:, np.random.default_rng(n).permutation(n)] if how == "permuted" else x
    D = float(PC.emd_matrix(put(x), put(y), normalize=True)[0, 0])
    diam = _diameter(x[0])
    print("emd_matrix of a %d-point cloud (cube of side %g) against %s: %.3e (closest pair %.3f, diameter %.3f, bound %.3e)"
          % (n, side, "itself" if how == "identical" else "a permutation of itself", D, gap, diam, 1e-5 * diam))
    assert 0 <= D <= 1e-5 * diam


@functools.lru_cache(maxsize=None)
def _dense_self(n):
    """-> (cloud [1, n, 3] uniform in the UNIT cube, float64 oracle of it against itself, the float32 oracle's value)"""
    x = _clouds(1, 1, n, n, 9000 + n)[0]
    return x, MO.emd(x[0], x[0]), MO.emd(x[0], x[0], dtype=np.float32)


@pytest.mark.parametrize("how", ["identical", "permuted"])
@pytest.mark.parametrize("n", [1024, 2048])
def test_a_dense_cloud_against_itself_matches_the_oracle(n, how):
    """1024 and 2048 points (the model's cloud size) in the UNIT cube against themselves and against a permutation of
    themselves, where neighbours share mass at the first level and the definition leaves 1.8e-5 and 3.2e-5 (see above):
    the float64 oracle's value (the same for both forms; the host tests hold its invariance under a permutation to 1e-12)
    within 16 x the float32 oracle's error ON THIS CASE (3.6e-7 at 2048 points: a gate of 5.8e-6).  The value is a sum of
    small leftovers of nearly cancelling masses, so the case has a yardstick of its own, by the rule of the gate."""
    PC = _PC()
    x, D64, D32 = _dense_self(n)
    gate = 16 * abs(D32 - D64) / D64
    assert 0 < gate < 1e-4, gate
    y = x[:, np.random.default_rng(n).permutation(n)] if how == "permuted" else x
    D = float(PC.emd_matrix(put(x), put(y))[0, 0])
    print("%d-point unit-cube cloud against %s: %.6e, float64 oracle %.6e, relative error %.3e (float32 oracle %.3e, gate "
          "%.3e)" % (n, "itself" if how == "identical" else "a permutation of itself", D, D64, abs(D - D64) / D64,
                     abs(D32 - D64) / D64, gate))
    assert abs(D - D64) <= gate * D64


def test_full_size_clouds():
    """4096 x 4096 points, all 128 KB of LDS and every register pair on both sides: finite, the same bits twice, and the
    same value within twice the gate when the points of both clouds are permuted (each value is within the gate of the
    one float64 value)"""
    PC = _PC()
    sample, ref = _clouds(1, 2, 4096, 4096)
    rng = np.random.default_rng(4096)
    D = PC.emd_matrix(put(sample), put(ref))
    assert torch.equal(D, PC.emd_matrix(put(sample), put(ref)))
    Dp = PC.emd_matrix(put(sample[:, rng.permutation(4096)]), put(ref[:, rng.permutation(4096)]))
    D, Dp = _host(D), _host(Dp)
    assert (D > 0.01).all() and (D < 1.0).all()      # (unrelated uniform clouds: a fraction of the cube's side)
    print("4096-point clouds %s, their points permuted %s" % (D.tolist(), Dp.tolist()))
    assert _rel(Dp, D) <= 2 * _gate()


# ------------------------------------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("S,R,M,N", [(3, 5, 33, 70), (1, 2, 2049, 1025), (50, 50, 16, 16)])
def test_two_runs_are_bit_identical(S, R, M, N):
    PC = _PC()
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    for normalize in (True, False):
        assert torch.equal(PC.emd_matrix(sample, ref, normalize), PC.emd_matrix(sample, ref, normalize))


def _transposed_view(a):
    """the [S, N, 3] view of [S, 3, N] storage: what evaluation/generate_data_for_metrics.py's transpose_(1, 2) yields"""
    v = put(a).permute(0, 2, 1).contiguous().transpose(1, 2)
    assert not v.is_contiguous() and v.stride(2) == a.shape[1]
    return v


@pytest.mark.parametrize("S,R,M,N", [(3, 5, 33, 70), (2, 3, 1030, 300)])
def test_layouts_change_no_bit(S, R, M, N):
    PC = _PC()
    sample, ref = _clouds(S, R, M, N)
    base = PC.emd_matrix(put(sample), put(ref))
    for name, s, r in (("sample transposed", _transposed_view(sample), put(ref)),
                       ("ref transposed", put(sample), _transposed_view(ref)),
                       ("both transposed", _transposed_view(sample), _transposed_view(ref))):
        assert torch.equal(PC.emd_matrix(s, r), base), name


def _count_launches(monkeypatch, PC):
    calls = []
    real = PC._lib.call
    monkeypatch.setattr(PC._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


@pytest.mark.parametrize("normalize", [True, False])
def test_slabs_change_no_bit(monkeypatch, normalize):
    """(3, 5, 33, 70) in one launch and in three launches of one row each"""
    PC = _PC()
    S, R, M, N = 3, 5, 33, 70
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    calls = _count_launches(monkeypatch, PC)
    whole = PC.emd_matrix(sample, ref, normalize=normalize)
    assert calls.count("sivae_emd_matrix") == 1
    monkeypatch.setattr(PC, "EMD_POINT_PAIRS_PER_LAUNCH", R * M * N)
    slabs = PC.emd_matrix(sample, ref, normalize=normalize)
    assert calls.count("sivae_emd_matrix") == 1 + S
    assert torch.equal(slabs, whole)


def test_a_true_row_slab_of_the_entry_point():
    """sivae_emd_matrix itself with 0 < s0 < s1 < S (pointcloud.emd_matrix always hands it whole matrices of sub-views): the
    rows s0 .. s1 - 1 bit for bit, every other element of D untouched"""
    PC = _PC()
    S, R, M, N = 5, 4, 33, 70
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    whole = PC.emd_matrix(sample, ref)
    D = torch.full((S, R), -7.0, dtype=torch.float32, device=DEV)
    ws = PC.workspace(PC._lib.load().sivae_emd_matrix_workspace_bytes(2, R, M, N), sample.device)
    sa, sb = sample.stride(), ref.stride()
    PC._lib.call("sivae_emd_matrix", PC._p(sample), sa[0], sa[1], sa[2], PC._p(ref), sb[0], sb[1], sb[2], PC._p(D), S, R, M, N,
                 2, 4, 1, PC._p(ws), ws.numel(), PC._s(sample))
    assert torch.equal(D[2:4], whole[2:4])
    assert bool((D[:2] == -7.0).all()) and bool((D[4:] == -7.0).all())


def test_long_rows_go_in_column_blocks(monkeypatch):
    """(3, 5, 33, 70) with two cloud pairs to a launch: every row in blocks of 2, 2 and 1 columns"""
    PC = _PC()
    S, R, M, N = 3, 5, 33, 70
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    whole = PC.emd_matrix(sample, ref)
    calls = _count_launches(monkeypatch, PC)
    monkeypatch.setattr(PC, "EMD_POINT_PAIRS_PER_LAUNCH", 2 * M * N)
    blocks = PC.emd_matrix(sample, ref)
    assert calls.count("sivae_emd_matrix") == 9
    assert torch.equal(blocks, whole)
    assert torch.equal(PC.emd_matrix(_transposed_view(sample.cpu().numpy()), _transposed_view(ref.cpu().numpy())), whole)


def test_more_pairs_than_blocks_against_row_slabs(monkeypatch):
    """50 x 50 clouds of 16 points: 2500 pairs on a grid capped at 1024 blocks (a block walks 2 or 3 pairs) against the
    same matrix in slabs of 7 rows (350 pairs: one pair a block).  Against the float64 oracle these sparse clouds have a
    yardstick of their own, by the rule of the gate: where a point's weights sum to about the 1e-9 of step 1, float32
    decides the split differently, and the float32 ORACLE is off by 6.8e-5 on its worst entry of this matrix."""
    PC = _PC()
    S, R, M, N = 50, 50, 16, 16
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    calls = _count_launches(monkeypatch, PC)
    whole = PC.emd_matrix(sample, ref)
    assert calls.count("sivae_emd_matrix") == 1
    monkeypatch.setattr(PC, "EMD_POINT_PAIRS_PER_LAUNCH", 7 * R * M * N)
    slabs = PC.emd_matrix(sample, ref)
    assert calls.count("sivae_emd_matrix") == 1 + 8
    assert torch.equal(slabs, whole)
    D64 = _ref(S, R, M, N, True)
    yard = _rel(_ref(S, R, M, N, True, None, np.float32), D64)
    w = _rel(_host(whole), D64)
    print("emd_matrix 50 x 50 clouds of 16 points: worst relative error %.3e (float32 oracle %.3e, gate %.3e)" % (w, yard, 16 * yard))
    assert w <= 16 * yard


# ------------------------------------------------------------------------------------------------ convention, NaN
@functools.lru_cache(maxsize=None)
def _asymmetric():
    """40-point uniform sample clouds, 70-point reference clouds in a Gaussian blob with five points set apart"""
    rng = np.random.default_rng(1)
    sample = (rng.random((2, 40, 3)) - 0.5).astype(np.float32)
    ref = (0.15 * rng.standard_normal((3, 70, 3))).astype(np.float32)
    ref[:, :5] += 0.4
    return sample, ref


def test_order_convention():
    """D[s, r] = EMD(left = ref_r, right = sample_s); the swapped call computes EMD(left = sample_s, right = ref_r), which
    the oracle tells apart by at least 100 gates on these clouds"""
    PC = _PC()
    sample, ref = _asymmetric()
    want = np.array([[MO.emd(ref[r], sample[s]) for r in range(3)] for s in range(2)])
    other = np.array([[MO.emd(sample[s], ref[r]) for r in range(3)] for s in range(2)])
    apart = float((np.abs(want - other) / want).min())
    assert apart >= 100 * _gate(), apart
    D = _host(PC.emd_matrix(put(sample), put(ref)))
    Dsw = _host(PC.emd_matrix(put(ref), put(sample))).T
    print("order convention: oracle's two orders differ by %.3e at least; kernel against the oracle %.3e, swapped call "
          "against the other order %.3e" % (apart, _rel(D, want), _rel(Dsw, other)))
    assert _rel(D, want) <= _gate() and _rel(Dsw, other) <= _gate()
    assert float((np.abs(D - Dsw) / want).min()) > _gate()


@pytest.mark.parametrize("normalize", [True, False])
def test_non_finite_coordinates_stay_in_their_row_and_column(normalize):
    PC = _PC()
    S, R, M, N = 3, 5, 33, 70
    sample, ref = (np.array(a) for a in _clouds(S, R, M, N))
    clean = PC.emd_matrix(put(sample), put(ref), normalize)
    assert bool(torch.isfinite(clean).all())
    sample[1, 17, 2] = np.nan
    ref[3, 69, 0] = np.inf
    D = PC.emd_matrix(put(sample), put(ref), normalize)
    bad = torch.zeros(S, R, dtype=torch.bool, device=DEV)
    bad[1, :] = True
    bad[:, 3] = True
    assert torch.equal(torch.isnan(D), bad)
    assert torch.equal(D[~bad], clean[~bad])
    assert np.array_equal(np.isnan(MO.emd_matrix(sample, ref, normalize)), bad.cpu().numpy())
    E = _E()
    for f in (E.minimum_mathing_distance, E.coverage):
        with pytest.raises(ValueError, match="non-finite"):
            f(None, None, dist=D)


# ------------------------------------------------------------------------------------------------ the drop-in module
def test_drop_in_mmd_and_cov():
    PC, E = _PC(), _E()
    seed, S, R, M, N = 2024, 6, 9, 40, 55
    sample, ref = _clouds(S, R, M, N, seed)
    D64 = _ref(S, R, M, N, True, seed)
    gap = EO.smallest_gap(D64)
    assert gap >= 100 * _gate(), "argmin gap %.2e: float32 cannot be asked for the float64 argmin" % gap
    D = PC.emd_matrix(put(sample), put(ref))
    assert _rel(_host(D), D64) <= _gate()
    De = E.emd_matrix(np.array(sample), np.array(ref))
    assert De.is_cuda and torch.equal(De, D)
    assert torch.equal(E.emd_matrix(torch.from_numpy(np.array(sample)), put(ref)), D)
    assert torch.equal(E.emd_matrix(np.array(sample), np.array(ref), normalize=False),
                       PC.emd_matrix(put(sample), put(ref), normalize=False))
    mmd64, matched64, _ = EO.minimum_matching_distance(D64)
    cov64, ref64, dist64 = EO.coverage(D64)
    for x_g, x, dist in ((np.array(sample), np.array(ref), D), (None, None, D.cpu().numpy())):
        mmd, matched = E.minimum_mathing_distance(x_g, x, dist=dist)
        cov, matched_ref, matched_dist = E.coverage(x_g, x, dist=dist, ret_dist=True)
        assert abs(mmd - mmd64) <= _gate() * mmd64
        assert np.all(np.abs(matched - matched64) <= _gate() * matched64)
        assert np.all(np.abs(matched_dist - dist64) <= _gate() * dist64)
        assert np.array_equal(matched_ref, ref64) and cov == cov64
    with pytest.raises(NotImplementedError):
        E.coverage(put(sample), put(ref), use_EMD=True)


# ------------------------------------------------------------------------------------------------ guarded
@pytest.mark.parametrize("S,R,M,N", [(2, 3, 257, 300), (1, 2, 2049, 1025)])
def test_guarded(S, R, M, N):
    """on a guarded, poisoned output and an exact workspace (no size uses one: a one-byte view of the guard): nothing
    written outside a tensor, no element left at the poison value, the unguarded results"""
    from sivae_hip import ops, pointcloud
    from support.guard import describe, guarded
    sample, ref = (put(a) for a in _clouds(S, R, M, N))
    D0 = pointcloud.emd_matrix(sample, ref)
    with guarded(pointcloud) as g:  # (pointcloud's names only: its torch; `workspace` is ops' and needs ops in the list)
        D1 = pointcloud.emd_matrix(sample, ref)
        damage = g.verify()
        assert not damage, "guard damage:\n%s" % describe(damage)
    with guarded(pointcloud, ops) as g:  # (and with the workspace at exactly its stated size)
        D2 = pointcloud.emd_matrix(sample, ref)
        damage = g.verify()
        assert not damage, "guard damage:\n%s" % describe(damage)
    for D in (D1, D2):
        assert bool(torch.isfinite(D).all()) and torch.equal(D, D0)
