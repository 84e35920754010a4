"""CPU-side checks of the pairwise figures on the FID features (csrc/feat_pairs.hip, sivae_hip/fidelity.py): the numpy
oracle tests/feat_metrics_oracle.py on cases worked by hand, the column-slab planner, KID's index draw, the header
against the wrappers, and the argument validation of the entry points (every call returns before any launch)."""
import ctypes
import inspect
import re

import numpy as np
import pytest
import torch

import feat_metrics_oracle as MO
from sivae_hip import fidelity as FD
from sivae_hip import lib, ops

LINE = np.array([[0.0], [1.0], [3.0], [6.0], [10.0]], dtype=np.float32)


# ------------------------------------------------------------------------------------------------ oracle by hand
def test_oracle_points_on_a_line():
    """0, 1, 3, 6, 10: gaps 1, 2, 3, 4"""
    d2 = MO.sqdist(LINE, LINE)
    assert d2[0].tolist() == [0, 1, 9, 36, 100] and np.array_equal(d2, d2.T)
    assert MO.knn(LINE, None, 1)[:, 0].tolist() == [1, 1, 4, 9, 16]               # a row is not its own neighbour
    assert MO.knn(LINE, None, 2).tolist() == [[1, 9], [1, 4], [4, 9], [9, 16], [16, 49]]
    assert MO.knn(LINE, LINE, 1)[:, 0].tolist() == [0, 0, 0, 0, 0]                # cross: it is
    assert MO.knn_gap(LINE, None, 1) == 3.0 and MO.knn_gap(LINE, None, 2) == 0.0      # (3: the neighbours 0 and 6 tie)
    assert MO.knn_gap(LINE, None, 4) == np.inf
    radii = MO.knn(LINE, None, 1)[:, 0]
    q = np.array([[2.0], [8.0], [-1.0], [20.0]], dtype=np.float32)
    # 2: inside the balls of 1 (1 <= 1, the boundary counts) and 3 (1 <= 4); 8: of 6 (4 <= 9) and 10 (4 <= 16);
    # -1: of 0 (1 <= 1); 20: of none
    assert MO.count_within(q, LINE, radii).tolist() == [2, 2, 1, 0]
    assert MO.membership_gap(q, LINE, radii) == 0.0                                # (the boundary cases above)
    assert MO.count_within(q, LINE, np.full(5, np.inf)).tolist() == [5] * 4
    assert MO.count_within(q, LINE, np.full(5, -1.0)).tolist() == [0] * 4


def test_oracle_prdc_by_hand():
    """real 0, 1, 3, 6, 10 with k = 1 (radii 1, 1, 4, 9, 16) against fake 2, 8, 20 (radii 36, 36, 144)"""
    fake = np.array([[2.0], [8.0], [20.0]], dtype=np.float32)
    p = MO.prdc(LINE, fake, 1)
    assert p["radii_real"].tolist() == [1, 1, 4, 9, 16] and p["radii_fake"].tolist() == [36, 36, 144]
    assert p["precision"] == 2 / 3 and p["density"] == 4 / 3            # 2 and 8 lie in two real balls each
    # every real row lies in a fake ball; nearest fake of 0, 1, 3, 6, 10: 4, 1, 1, 4, 4 against radii 1, 1, 4, 9, 16
    assert p["recall"] == 1.0 and p["coverage"] == 4 / 5
    assert p["gap"] == 0.0


def test_oracle_distance_bound_covers_the_expanded_form():
    """the gate, on the construction of the GPU tests: numpy's own expanded form stays inside it"""
    for shape in ((130, 97, 67, 1), (40, 30, 2048, 3)):
        real, fake = MO.construction(*shape)
        x, y = real.astype(np.float64), fake.astype(np.float64)
        expanded = np.maximum(0.0, (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T)
        err = np.abs(expanded - MO.sqdist(real, fake)).max()
        print("%s: expanded vs direct %.3e, gate %.3e" % (shape, err, MO.sqdist_bound(real, fake)))
        assert err <= MO.sqdist_bound(real, fake)


def test_oracle_poly_sums_and_kid_by_hand():
    x = np.array([[1.0, 0.0], [0.0, 2.0]], dtype=np.float32)
    y = np.array([[1.0, 1.0], [2.0, 0.0], [0.0, 0.0]], dtype=np.float32)
    # gamma 0.5, coef0 1, degree 2: x.y = [[1, 2, 0], [2, 0, 0]] -> (0.5 t + 1)^2 = [[2.25, 4, 1], [4, 1, 1]]
    assert MO.poly_sum(x, y, 0.5, 1.0, 2) == (13.25, 13.25, 6)
    assert MO.poly_sum(x, y, 0.5, 1.0, 2, skip_diag=True) == (13.25 - 2.25 - 1.0, 10.0, 4)
    assert MO.poly_sum(x, y, -1.0, 0.0, 1)[0:2] == (-5.0, 5.0)
    # KID of a set against itself with the same subsets: sxx = syy, sxy = sxx + the diagonal
    g = np.random.default_rng(3)
    a = g.standard_normal((12, 5)).astype(np.float32)
    idx = np.stack([g.permutation(12)[:6] for _ in range(4)])
    mean, std, bound = MO.kid(a, a, idx, idx)
    for s in range(4):
        sub = a[idx[s]].astype(np.float64)
        k = (sub @ sub.T / 5 + 1.0) ** 3
        off, diag = k.sum() - np.trace(k), np.trace(k)
        want = 2 * off / 30 - 2 * (off + diag) / 36
        got = MO.kid(a, a, idx[s:s + 1], idx[s:s + 1])[0]
        assert abs(got - want) <= 1e-12 * abs(k).sum()
    assert std >= 0 and 0 < bound < 1e-10


def test_oracle_construction_is_seeded_and_mixed():
    real, fake = MO.construction(130, 97, 67, 1)
    again = MO.construction(130, 97, 67, 1)
    assert np.array_equal(real, again[0]) and np.array_equal(fake, again[1])
    assert real.dtype == np.float32 and real.shape == (130, 67) and fake.shape == (97, 67)
    p = MO.prdc(real, fake, 3)
    for name in ("precision", "recall", "density", "coverage"):
        assert 0.0 < p[name] < 1.0, (name, p[name])
    assert p["gap"] > 1e6 * MO.sqdist_bound(real, fake)


# ------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("nrows,ncols,d,macs", [(50000, 50000, 2048, None), (130, 200, 67, 130 * 67 * 64),
                                                (130, 200, 67, 1), (9, 9, 16, None), (200, 193, 2048, 200 * 2048 * 128),
                                                (64, 64, 1, 64 * 64), (10000, 50000, 2048, 2 ** 38)])
def test_slab_planner(nrows, ncols, d, macs):
    slabs = FD.plan_slabs(nrows, ncols, d, macs)
    budget = FD.FEAT_MACS_PER_LAUNCH if macs is None else macs
    assert slabs[0][0] == 0 and slabs[-1][1] == ncols
    assert all(a[1] == b[0] for a, b in zip(slabs, slabs[1:]))                 # [0, ncols) once, in order
    assert all(c0 % 64 == 0 and c0 < c1 for c0, c1 in slabs)                   # whole tiles
    assert all((c1 - c0) % 64 == 0 for c0, c1 in slabs[:-1])
    for c0, c1 in slabs:
        assert nrows * (c1 - c0) * d <= budget or c1 - c0 <= 64               # within the budget, or the one-tile minimum
    widths = {c1 - c0 for c0, c1 in slabs[:-1]}
    assert len(widths) <= 1
    if widths:                                                                 # ... and no narrower than it has to be
        assert nrows * (widths.pop() + 64) * d > budget
    assert FD.plan_slabs(nrows, ncols, d, macs) == slabs                       # a pure function


def test_slab_planner_at_the_full_size():
    slabs = FD.plan_slabs(50000, 50000, 2048)
    assert FD.FEAT_MACS_PER_LAUNCH == 49 * 64 * 50000 * 2048      # 49 column tiles a launch at this size
    assert len(slabs) == 16 and slabs[0] == (0, 3136) and slabs[-1] == (47040, 50000)
    with pytest.raises(ValueError):
        FD.plan_slabs(0, 5, 5)


# ------------------------------------------------------------------------------------------------ KID's draw
def test_kid_index_draw():
    ri, fi = FD.kid_indices(130, 97, subsets=7, subset_size=50, seed=4)
    assert ri.shape == fi.shape == (7, 50) and ri.dtype == fi.dtype == torch.int64 and not ri.is_cuda
    for rows, n in ((ri, 130), (fi, 97)):
        assert int(rows.min()) >= 0 and int(rows.max()) < n
        assert all(len(set(r.tolist())) == 50 for r in rows)                   # without replacement
    again = FD.kid_indices(130, 97, subsets=7, subset_size=50, seed=4)
    assert torch.equal(ri, again[0]) and torch.equal(fi, again[1])             # seeded
    other = FD.kid_indices(130, 97, subsets=7, subset_size=50, seed=5)
    assert not torch.equal(ri, other[0])
    assert len({tuple(r.tolist()) for r in ri}) == 7                           # the subsets differ
    state = torch.random.get_rng_state()
    FD.kid_indices(130, 97, subsets=2, subset_size=5, seed=0)
    assert torch.equal(state, torch.random.get_rng_state())                    # its own generator
    full = FD.kid_indices(20, 20, subsets=1, subset_size=20, seed=0)
    assert sorted(full[0][0].tolist()) == list(range(20))
    for bad in (dict(subset_size=98), dict(subset_size=1), dict(subsets=0)):
        with pytest.raises(ValueError):
            FD.kid_indices(130, 97, **dict(dict(subsets=3, subset_size=10), **bad))


# ------------------------------------------------------------------------------------------------ header and surface
ENTRIES = ("sivae_feat_row_sqnorm", "sivae_feat_sqdist", "sivae_feat_knn_update", "sivae_feat_within_update",
           "sivae_feat_poly_sums", "sivae_feat_poly_workspace_bytes")


def test_header_declares_every_entry_the_wrappers_call():
    protos = lib.parse_header()
    called = set(re.findall(r"\bsivae_feat_\w+", inspect.getsource(ops)))
    assert called == set(ENTRIES)
    L = lib.load()
    for name in called:
        assert name in protos and hasattr(L, name), name
    assert L.sivae_abi_version() == 1
    assert protos["sivae_feat_poly_workspace_bytes"][0] is ctypes.c_size_t
    assert len(protos["sivae_feat_knn_update"][1]) == 15 and len(protos["sivae_feat_within_update"][1]) == 14
    assert len(protos["sivae_feat_sqdist"][1]) == 12 and len(protos["sivae_feat_poly_sums"][1]) == 18


def test_entry_points_validate_arguments():
    L = lib.load()
    null, one, odd = None, ctypes.c_void_p(16), ctypes.c_void_p(20)
    assert L.sivae_feat_row_sqnorm(null, 8, 4, 8, one, null) == -1
    assert L.sivae_feat_row_sqnorm(one, 8, 4, 8, null, null) == -1
    assert L.sivae_feat_row_sqnorm(one, 7, 4, 8, one, null) == -2              # row stride below d
    assert L.sivae_feat_row_sqnorm(one, 8, 0, 8, one, null) == -2
    assert L.sivae_feat_row_sqnorm(one, 8192, 4, 8193, one, null) == -2         # d <= 8192
    assert L.sivae_feat_row_sqnorm(ctypes.c_void_p(18), 8, 4, 8, one, null) == -2
    assert L.sivae_feat_row_sqnorm(one, 8, 4, 8, odd, null) == -2               # fp64 output: 8-byte aligned
    sq = L.sivae_feat_sqdist
    assert sq(one, 8, 4, null, one, 8, 4, one, 8, one, 4, null) == -1
    assert sq(one, 8, 4, one, one, 8, 4, one, 8, one, 3, null) == -2           # ldd below ny
    assert sq(one, 8, 4, one, one, 4, 4, one, 8, one, 4, null) == -2
    kn = L.sivae_feat_knn_update
    args = (one, 8, 4, one, one, 8, 6, one)
    assert kn(*args, 0, 6, 8, 3, 0, null, null) == -1
    assert kn(*args, 0, 6, 8, 0, 0, one, null) == -2 and kn(*args, 0, 6, 8, 9, 0, one, null) == -2   # 1 <= k <= 8
    assert kn(*args, 0, 7, 8, 3, 0, one, null) == -2 and kn(*args, 5, 4, 8, 3, 0, one, null) == -2   # [c0, c1) in [0, ny]
    assert kn(*args, -1, 4, 8, 3, 0, one, null) == -2
    assert kn(*args, 0, 6, 8, 3, 2, one, null) == -6
    assert kn(*args, 3, 3, 8, 3, 1, one, null) == 0                             # an empty range launches nothing
    wi = L.sivae_feat_within_update
    assert wi(*args, null, 0, 6, 8, one, null) == -1 and wi(*args, one, 0, 6, 8, null, null) == -1
    assert wi(*args, one, 0, 7, 8, one, null) == -2 and wi(*args, one, 0, 6, 8, ctypes.c_void_p(18), null) == -2
    assert wi(*args, one, 6, 6, 8, one, null) == 0
    assert L.sivae_feat_poly_workspace_bytes(3, 130) == 3 * 3 * 8 and L.sivae_feat_poly_workspace_bytes(1, 64) == 8
    assert L.sivae_feat_poly_workspace_bytes(0, 64) == 0
    po = L.sivae_feat_poly_sums
    sets = (one, 64, 8, one, 64, 8, 2, 5, 6, 8)
    assert po(*sets, 0.5, 1.0, 3, 0, null, one, 1 << 10, null) == -1
    assert po(*sets, 0.5, 1.0, 3, 0, one, null, 1 << 10, null) == -1
    assert po(*sets, 0.5, 1.0, 0, 0, one, one, 1 << 10, null) == -6 and po(*sets, 0.5, 1.0, 5, 0, one, one, 1 << 10, null) == -6
    assert po(*sets, 0.5, 1.0, 3, 2, one, one, 1 << 10, null) == -6
    assert po(*sets, 0.5, 1.0, 3, 0, one, one, 8, null) == -4                   # two subsets of one strip: 16 bytes
    assert po(one, 64, 8, one, 64, 8, 0, 5, 6, 8, 0.5, 1.0, 3, 0, one, one, 1 << 10, null) == -2


def test_python_surface():
    want = {"sqdist_matrix": ["x", "y"], "knn_sqdist": ["x", "y", "k"], "count_within": ["q", "x", "radii"],
            "prdc": ["real", "fake", "k"],
            "kid": ["real", "fake", "subsets", "subset_size", "degree", "gamma", "coef0", "seed", "indices"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(FD, name)).parameters) == params, name
    sig = inspect.signature(FD.calculate_fidelity_given_dataset)
    assert list(sig.parameters)[:11] == ["dataloader", "model_s", "batch_size", "cuda", "dims", "device", "num_images",
                                         "inception", "k", "kid_subsets", "kid_subset_size"]
    assert (sig.parameters["k"].default, sig.parameters["kid_subsets"].default,
            sig.parameters["kid_subset_size"].default) == (3, 100, 1000)
    assert inspect.signature(FD.kid).parameters["gamma"].default is None
    assert list(inspect.signature(FD.FeatureBank.__init__).parameters) == ["self", "dims", "device", "capacity"]


def test_cpu_tensors_and_bad_k_are_refused():
    x = torch.zeros(9, 4)
    for call in (lambda: FD.sqdist_matrix(x), lambda: FD.knn_sqdist(x), lambda: FD.count_within(x, x, torch.zeros(9)),
                 lambda: FD.prdc(x, x), lambda: FD.kid(x, x, subsets=1, subset_size=4),
                 lambda: ops.feat_row_sqnorm(x), lambda: ops.feat_poly_sums(x[None], x[None], 0.25),
                 lambda: FD.FeatureBank(4, "cpu", 8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for k in (0, 9):
        with pytest.raises(ValueError, match="1 .. 8"):
            ops.feat_knn_state(4, k, "cpu")
