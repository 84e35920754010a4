"""The pairwise figures on the FID features (csrc/feat_pairs.hip, sivae_hip/fidelity.py) on an MI355X against the numpy
oracle tests/feat_metrics_oracle.py (float64, direct-form distances).

Gates, derived, not measured.  DISTANCE: the kernel evaluates |x|^2 + |y|^2 - 2 x.y with three length-d fp64 accumulations
of exact products, so |got - ref| <= 2 (d + 3) 2^-53 (max|x| + max|y|)^2 (MO.sqdist_bound).  MEMBERSHIP and the
fractions built on it are compared EXACTLY: each test first asserts that its inputs keep every compared pair
(distance, radius) farther apart than the distance gate (twice the gate where the radius comes from the device too).
KERNEL SUMS: 2 (d + 3 + number of addends) 2^-53 sum |k_ij| (MO.poly_sum_bound), on the sums, not on MMD^2, which
cancels."""
import functools
import math
import re

import numpy as np
import pytest
import torch

import feat_metrics_oracle as MO
from support import fid_features as FX
from support.guard import describe, guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RECORDED = (130, 97, 67, 1)      # real rows, fake rows, d, seed: precision 0.4948, recall 0.9462, density 0.5773, coverage 0.8154
WIDE = (200, 130, 2048, 2)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def _sets(n_real, n_fake, d, seed):
    return MO.construction(n_real, n_fake, d, seed)


@functools.lru_cache(maxsize=None)
def _prdc_ref(case):
    real, fake = _sets(*case)
    bound = max(MO.sqdist_bound(real, fake), MO.sqdist_bound(real, real), MO.sqdist_bound(fake, fake))
    return MO.prdc(real, fake, 3), bound


@functools.lru_cache(maxsize=None)
def _asym(nx, ny, d):
    """two sets of different scale and offset; one row of x planted at +100 (a wrong result map cannot hide)"""
    g = np.random.default_rng(7919 * nx + 31 * ny + d)
    x = (0.7 * g.standard_normal((nx, d)) + 0.3).astype(np.float32)
    y = (1.3 * g.standard_normal((ny, d)) - 0.2).astype(np.float32)
    x[(2 * nx) // 3] += np.float32(100.0)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _strided(a):
    """the same rows with row stride d + 3, the first element 4 bytes behind a 16-byte boundary: the scalar loads"""
    n, d = a.shape
    flat = torch.zeros(n * (d + 3) + 1, dtype=torch.float32, device=DEV)
    view = flat[1:].view(n, d + 3)[:, :d]
    view.copy_(_dev(a))
    assert view.stride() == (d + 3, 1) and view.data_ptr() % 16 == 4
    return view


def _padded(a):
    """the same rows with a row stride that is a multiple of 4 behind a 16-byte aligned base: 16-byte loads, and where
    d % 4 != 0 a last k-quad that is cut (its elements come one by one)"""
    n, d = a.shape
    ld = (d + 3) // 4 * 4 + 4
    view = torch.zeros((n, ld), dtype=torch.float32, device=DEV)[:, :d]
    view.copy_(_dev(a))
    assert view.stride() == (ld, 1) and view.data_ptr() % 16 == 0
    return view


def _lower_budget(monkeypatch, nrows, d):
    """one 64-column tile per launch"""
    from sivae_hip import fidelity as FD
    monkeypatch.setattr(FD, "FEAT_MACS_PER_LAUNCH", nrows * d * 64)


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("nx,ny,d", [(5, 3, 7), (65, 130, 67), (64, 64, 16), (130, 65, 1), (70, 100, 2048)])
def test_sqdist_matrix_against_the_oracle(nx, ny, d):
    """one MFMA tile, partial tiles in both directions, exactly one tile, d = 1 (a k tail of 15), 128 staged chunks;
    contiguous rows (16-byte loads only where d % 4 == 0), then the scalar loads, then 16-byte loads with a cut last quad"""
    from sivae_hip import fidelity as FD
    x, y = _asym(nx, ny, d)
    ref, bound = MO.sqdist(x, y), MO.sqdist_bound(x, y)
    for tag, xs, ys in (("contiguous", _dev(x), _dev(y)), ("scalar loads", _strided(x), _strided(y)),
                        ("16-byte loads, padded rows", _padded(x), _padded(y))):
        got = FD.sqdist_matrix(xs, ys)
        assert got.dtype == torch.float64 and tuple(got.shape) == (nx, ny)
        err = np.abs(got.cpu().numpy() - ref).max()
        print("sqdist %s %s: worst error %.3e, gate %.3e" % ((nx, ny, d), tag, err, bound))
        assert err <= bound, tag
    # the planted row is where it belongs, and the other rows are not near it
    far = ref[(2 * nx) // 3].min()
    assert far > 10 * np.delete(ref, (2 * nx) // 3, axis=0).max() or nx == 1
    self_d = FD.sqdist_matrix(_dev(x)).cpu().numpy()
    assert np.abs(self_d - MO.sqdist(x, x)).max() <= MO.sqdist_bound(x, x)
    assert (np.diag(self_d) <= MO.sqdist_bound(x, x)).all() and (self_d >= 0).all()


# ------------------------------------------------------------------------------------------------ nearest neighbours
@pytest.mark.parametrize("n", [9, 130, 200])
def test_knn_sqdist(n, monkeypatch):
    from sivae_hip import fidelity as FD
    real, fake = _sets(n, 70, 67, 10 + n)
    x, q = _dev(real), _dev(fake)
    bound = max(MO.sqdist_bound(real, real), MO.sqdist_bound(fake, real))
    for k in (1, 3, 8):
        self_k, cross_k = FD.knn_sqdist(x, k=k), FD.knn_sqdist(q, x, k=k)
        assert tuple(self_k.shape) == (n, k) and tuple(cross_k.shape) == (70, k) and self_k.dtype == torch.float64
        for tag, got, ref in (("self", self_k, MO.knn(real, None, k)), ("cross", cross_k, MO.knn(fake, real, k))):
            err = np.abs(got.cpu().numpy() - ref).max()
            print("knn n %d k %d %s: worst error %.3e, gate %.3e" % (n, k, tag, err, bound))
            assert err <= bound, (tag, k)                      # (order statistics move by at most the entries' error)
            assert bool((got[:, 1:] >= got[:, :-1]).all())     # ascending
        assert torch.equal(self_k, FD.knn_sqdist(x, k=k)) and torch.equal(cross_k, FD.knn_sqdist(q, x, k=k))  # two runs
    # a row is never its own neighbour: the nearest OTHER row is far (these are independent normal rows)
    assert float(FD.knn_sqdist(x, k=1).min()) > 1.0
    if n == 200:  # the columns cut into four launches, three of them with c0 > 0
        whole = FD.knn_sqdist(x, k=8), FD.knn_sqdist(q, x, k=8)
        _lower_budget(monkeypatch, 200, 67)
        slabs = FD.plan_slabs(200, 200, 67)
        assert len(slabs) == 4 and sum(c0 > 0 for c0, _ in slabs) == 3
        assert torch.equal(whole[0], FD.knn_sqdist(x, k=8))
        _lower_budget(monkeypatch, 70, 67)
        assert len(FD.plan_slabs(70, 200, 67)) == 4
        assert torch.equal(whole[1], FD.knn_sqdist(q, x, k=8))


def test_knn_sqdist_wide_and_strided():
    """d = 2048 through both load paths"""
    from sivae_hip import fidelity as FD
    real, _ = _sets(*WIDE)
    real = real[:130]
    ref, bound = MO.knn(real, None, 3), MO.sqdist_bound(real, real)
    a, b = FD.knn_sqdist(_dev(real), k=3), FD.knn_sqdist(_strided(real), k=3)
    assert np.abs(a.cpu().numpy() - ref).max() <= bound and np.abs(b.cpu().numpy() - ref).max() <= bound
    assert torch.equal(a, b)     # (the loads differ, the arithmetic does not)


def test_knn_duplicate_rows():
    """two identical rows i != j: each is the other's nearest neighbour at a distance within the gate of 0, not
    necessarily 0; the pair (i, i) is left out by index, so no other row sees a 0"""
    from sivae_hip import fidelity as FD
    real, _ = _sets(130, 70, 67, 140)
    x = np.array(real)
    x[77] = x[5]
    bound = MO.sqdist_bound(x, x)
    best = FD.knn_sqdist(_dev(x), k=1)[:, 0].cpu().numpy()
    assert 0 <= best[5] <= bound and 0 <= best[77] <= bound
    others = np.delete(best, [5, 77])
    assert np.abs(others - np.delete(MO.knn(x, None, 1)[:, 0], [5, 77])).max() <= bound and others.min() > 1.0


# ------------------------------------------------------------------------------------------------ ball counts
def test_count_within(monkeypatch):
    from sivae_hip import fidelity as FD
    real, fake = _sets(*RECORDED)
    radii = MO.knn(real, None, 3)[:, 2]
    bound = MO.sqdist_bound(fake, real)
    gap = MO.membership_gap(fake, real, radii)
    print("count_within: smallest |sqdist - radius| %.3e = %.2e x the gate" % (gap, gap / bound))
    assert gap > bound
    ref = MO.count_within(fake, real, radii)
    assert 0 < (ref > 0).sum() < len(ref)
    q, x, r = _dev(fake), _dev(real), _dev(radii)
    got = FD.count_within(q, x, r)
    assert got.dtype == torch.int32 and tuple(got.shape) == (97,)
    assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(FD.count_within(_strided(fake), _strided(real), r).cpu().numpy(), ref)
    inf, neg = torch.full_like(r, float("inf")), torch.full_like(r, -1.0)
    assert FD.count_within(q, x, inf).tolist() == [130] * 97 and FD.count_within(q, x, neg).tolist() == [0] * 97
    _lower_budget(monkeypatch, 97, 67)
    assert len(FD.plan_slabs(97, 130, 67)) == 3
    assert torch.equal(got, FD.count_within(q, x, r)) and FD.count_within(q, x, inf).tolist() == [130] * 97


# ------------------------------------------------------------------------------------------------ the four figures
@pytest.mark.parametrize("case", [RECORDED, WIDE])
def test_prdc(case):
    from sivae_hip import fidelity as FD
    real, fake = _sets(*case)
    ref, bound = _prdc_ref(case)
    print("prdc %s: oracle %s, smallest gap %.2e x the gate"
          % (case, {n: round(ref[n], 4) for n in ("precision", "recall", "density", "coverage")}, ref["gap"] / bound))
    assert ref["gap"] > 2 * bound                          # (the device's radius and its distance may both move)
    got = FD.prdc(_dev(real), _dev(fake), k=3)
    for name in ("precision", "recall", "density", "coverage"):
        assert isinstance(got[name], float) and ref[name] not in (0.0, 1.0)
        assert got[name] == ref[name], name
    for name in ("radii_real", "radii_fake"):
        assert got[name].dtype == torch.float64 and got[name].is_cuda
        assert np.abs(got[name].cpu().numpy() - ref[name]).max() <= bound


# ------------------------------------------------------------------------------------------------ kernel sums and KID
def _subsets(S, m, n, d, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((S, m, d)) + 0.25).astype(np.float32)
    y = (1.2 * g.standard_normal((S, n, d)) - 0.1).astype(np.float32)
    return x, y


@pytest.mark.parametrize("S,m,n,d", [(3, 130, 97, 67), (1, 70, 70, 2048)])
def test_poly_sums(S, m, n, d):
    from sivae_hip import ops
    x, y = _subsets(S, m, n, d, 5 * d + S)
    xd, yd = _dev(x), _dev(y)
    gamma = 1.0 / d
    calls = (("xx", xd, xd, x, x, True), ("yy", yd, yd, y, y, True), ("xy", xd, yd, x, y, False))
    for tag, a, b, an, bn, skip in calls:
        got = ops.feat_poly_sums(a, b, gamma, 1.0, 3, skip_diag=skip)
        assert got.dtype == torch.float64 and tuple(got.shape) == (S,)
        for s in range(S):
            ref, sum_abs, addends = MO.poly_sum(an[s], bn[s], gamma, 1.0, 3, skip)
            bound = MO.poly_sum_bound(d, addends, sum_abs)
            print("poly %s subset %d of %s: error %.3e, bound %.3e" % (tag, s, (S, m, n, d), abs(float(got[s]) - ref), bound))
            assert abs(float(got[s]) - ref) <= bound, (tag, s)
        assert torch.equal(got, ops.feat_poly_sums(a, b, gamma, 1.0, 3, skip_diag=skip))          # two runs
        if S > 1:  # a subset's sum does not depend on the subsets it is launched with
            parts = torch.cat([ops.feat_poly_sums(a[:1], b[:1], gamma, 1.0, 3, skip_diag=skip),
                               ops.feat_poly_sums(a[1:], b[1:], gamma, 1.0, 3, skip_diag=skip)])
            assert torch.equal(got, parts)
    # skip_diag really skips: the difference is the diagonal
    full, skipped = ops.feat_poly_sums(xd, xd, gamma, 1.0, 3), ops.feat_poly_sums(xd, xd, gamma, 1.0, 3, skip_diag=True)
    for s in range(S):
        k = MO.poly_kernel(x[s], x[s], gamma, 1.0, 3)
        diag = float(np.trace(k))
        assert diag > 1e3 * MO.poly_sum_bound(d, m * m, np.abs(k).sum())
        assert abs(float(full[s] - skipped[s]) - diag) <= 2 * MO.poly_sum_bound(d, m * m, np.abs(k).sum())


def test_poly_sums_degrees_and_coefficients():
    from sivae_hip import ops
    x, y = _subsets(2, 65, 33, 19, 3)
    for degree, gamma, coef0 in ((1, -0.5, 0.0), (2, 0.25, 1.0), (3, 1.0 / 19, 1.0), (4, 0.1, -0.5)):
        got = ops.feat_poly_sums(_dev(x), _dev(y), gamma, coef0, degree)
        for s in range(2):
            ref, sum_abs, addends = MO.poly_sum(x[s], y[s], gamma, coef0, degree)
            assert abs(float(got[s]) - ref) <= MO.poly_sum_bound(19, addends, sum_abs), degree
    with pytest.raises(ValueError, match="degree"):
        ops.feat_poly_sums(_dev(x), _dev(y), 0.1, 1.0, 5)


@pytest.mark.parametrize("d", [1, 16, 67, 130])
def test_both_orientations_are_one_tile_body(d):
    """x . y through the rows operand (feat_poly_sums: X Y^T of one row each, gamma 1, coef0 0, degree 1) and through the
    columns operand (fid_xty: X^T Y of one column each) is the same k-ascending fp64 MFMA accumulation of exact products
    (csrc/f64_tile.h), and everything the poly epilogue adds to it is zero: the two results are equal bit for bit.
    d: below a k-step, exactly one staged chunk, a ragged last chunk, several chunks with a ragged tail."""
    from sivae_hip import ops
    g = np.random.default_rng(4099 + d)
    x = _dev((1.7 * g.standard_normal(d)).astype(np.float32))
    y = _dev((0.6 * g.standard_normal(d) + 0.1).astype(np.float32))
    if d > 1:  # mixed signs in both vectors and in the products
        assert (x.min() < 0 < x.max()) and (y.min() < 0 < y.max()) and ((x * y).min() < 0 < (x * y).max())
    rows = ops.feat_poly_sums(x[None, None], y[None, None], gamma=1.0, coef0=0.0, degree=1)
    cols = ops.fid_xty(x.double()[:, None], y.double()[:, None])
    assert tuple(rows.shape) == (1,) and tuple(cols.shape) == (1, 1) and rows.dtype == cols.dtype == torch.float64
    print("d %d: rows %r, columns %r" % (d, float(rows[0]), float(cols[0, 0])))
    assert float(rows[0]) != 0.0 and torch.equal(rows.view(1, 1), cols)


def test_kid_against_the_oracle(monkeypatch):
    from sivae_hip import fidelity as FD
    real, fake = _sets(*RECORDED)
    ri, fi = FD.kid_indices(130, 97, subsets=5, subset_size=70, seed=3)
    mean_ref, std_ref, bound = MO.kid(real, fake, ri.numpy(), fi.numpy())
    x, y = _dev(real), _dev(fake)
    mean, std = FD.kid(x, y, indices=(ri, fi))
    print("kid: %.12g +- %.6g, oracle %.12g +- %.6g, bound %.3e" % (mean, std, mean_ref, std_ref, bound))
    assert isinstance(mean, float) and isinstance(std, float) and mean_ref > 100 * bound
    # every subset's MMD^2 is within `bound`: so is their mean; the deviation moves by at most twice that
    assert abs(mean - mean_ref) <= bound and abs(std - std_ref) <= 2 * bound
    assert FD.kid(x, y, subsets=5, subset_size=70, seed=3) == (mean, std)                # the seeded draw is this draw
    assert FD.kid(x, y, subsets=5, subset_size=70, seed=4) != (mean, std)
    monkeypatch.setattr(FD, "FEAT_MACS_PER_LAUNCH", 2 * 70 * 70 * 67)                    # two subsets per launch
    assert FD.kid(x, y, indices=(ri, fi)) == (mean, std)
    mean_self, _ = FD.kid(x, x, subsets=3, subset_size=100, seed=1)
    assert abs(mean_self) < mean                                                         # the same distribution


# ------------------------------------------------------------------------------------------------ the whole pass
class _Generator(torch.nn.Module):
    """stand-in for the VAE: sample(noise) -> [b, 3, 8, 8] images in (0, 1)"""

    def __init__(self, zdim=8):
        super().__init__()
        self.zdim = zdim
        self.fc = torch.nn.Linear(zdim, 3 * 8 * 8)
        with torch.no_grad():
            g = torch.Generator().manual_seed(11)
            self.fc.weight.copy_(torch.randn(3 * 8 * 8, zdim, generator=g))
            self.fc.bias.copy_(torch.randn(3 * 8 * 8, generator=g))

    def sample(self, z):
        return torch.sigmoid(self.fc(z)).reshape(-1, 3, 8, 8)


class _Recording(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net, self.seen = net, []

    def forward(self, x):
        out = self.net(x)
        self.seen.append(out[0])
        return out


def test_whole_pass_with_stand_ins():
    from sivae_hip import fid as F
    from sivae_hip import fidelity as FD
    from sivae_hip import rng
    batches, net, num, b, _, _ = FX.loader_case()
    net = _Recording(net.to(DEV))
    model_s = _Generator().to(DEV)
    rng.manual_seed(77)
    fid = F.calculate_fid_given_dataset(batches, model_s, b, True, 16, DEV, num, inception=net)
    net.seen.clear()
    rng.manual_seed(77)
    out = FD.calculate_fidelity_given_dataset(batches, model_s, b, True, 16, DEV, num, inception=net, k=3, kid_subsets=6,
                                              kid_subset_size=40)
    assert sorted(out) == ["coverage", "density", "fid", "kid_mean", "kid_std", "precision", "recall"]
    assert all(isinstance(v, float) and math.isfinite(v) for v in out.values())
    assert out["fid"] == fid                                   # one pass per side, the same moments
    n_real = math.ceil(num / b)
    assert len(net.seen) == n_real + math.ceil(num / b)        # ... and no second Inception pass for the rows
    rows = [torch.cat([torch.nn.functional.adaptive_avg_pool2d(o, (1, 1)).flatten(1) for o in part])[:num].contiguous()
            for part in (net.seen[:n_real], net.seen[n_real:])]
    assert rows[0].shape == rows[1].shape == (num, 16)
    figures = FD.prdc(rows[0], rows[1], k=3)
    for name in ("precision", "recall", "density", "coverage"):
        assert out[name] == figures[name], name
    assert (out["kid_mean"], out["kid_std"]) == FD.kid(rows[0], rows[1], subsets=6, subset_size=40)
    # real= skips the real side
    real = FD.real_features(batches, net, 16, DEV, num)
    assert torch.equal(real[1], rows[0])
    net.seen.clear()
    rng.manual_seed(77)
    short = FD.calculate_fidelity_given_dataset(batches, model_s, b, True, 16, DEV, num, inception=net, k=3, kid_subsets=6,
                                                kid_subset_size=40, real=real)
    assert short == out and len(net.seen) == math.ceil(num / b)
    print("stand-in figures: %s" % out)


def test_feature_bank():
    from sivae_hip import fidelity as FD
    bank = FD.FeatureBank(16, DEV, 50)
    g = torch.Generator().manual_seed(2)
    a = torch.rand(30, 16, generator=g).to(DEV)
    m = torch.rand(30, 16, 2, 2, generator=g).to(DEV)
    bank.update(a).update(m).update(a[:0])
    assert bank.rows_seen == 60 and tuple(bank.rows().shape) == (50, 16)
    pooled = torch.nn.functional.adaptive_avg_pool2d(m, (1, 1)).flatten(1)      # what ActivationStatistics does to maps
    assert torch.equal(bank.rows(30), a) and torch.equal(bank.rows()[30:], pooled[:20])
    with pytest.raises(ValueError, match="kept"):
        bank.rows(51)
    with pytest.raises(ValueError, match="expected activations"):
        bank.update(torch.rand(3, 15).to(DEV))
    with pytest.raises(TypeError, match="float32 ROCm tensor"):
        bank.update(torch.rand(3, 16))


def _train_once(tmp_path, monkeypatch, capsys, extra):
    import train_soft_intro_vae as T
    _, net, _, _, _, _ = FX.loader_case()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SIVAE_SYNTHETIC_IMAGES", "16")
    monkeypatch.delenv("SIVAE_FID", raising=False)
    monkeypatch.delenv("SIVAE_FID_CACHE_REAL", raising=False)
    if extra:
        monkeypatch.setenv("SIVAE_FID_EXTRA", "1")
    else:
        monkeypatch.delenv("SIVAE_FID_EXTRA", raising=False)
    monkeypatch.setattr(T, "FID_ARGS", dict(dims=16, num_images=16))
    monkeypatch.setattr(T, "FID_INCEPTION", net)
    capsys.readouterr()
    T.train_soft_intro_vae(dataset="synthetic-cifar10", z_dim=16, batch_size=8, num_workers=0, num_epochs=1, beta_kl=1.0,
                           beta_rec=1.0, beta_neg=256, seed=5, save_interval=50, device=DEV, with_fid=True)
    return capsys.readouterr().out


def test_trainer_extra_branch(tmp_path, monkeypatch, capsys):
    """SIVAE_FID_EXTRA=1: one `fidelity:` line per FID pass, in front of the `fid:` line; unset: the FID pass of before,
    through fid.calculate_fid_given_dataset, and not one line more"""
    from sivae_hip import fid as F
    from sivae_hip import fidelity as FD
    calls = {"fid": 0, "fidelity": 0}
    real_fid, real_fidelity = F.calculate_fid_given_dataset, FD.calculate_fidelity_given_dataset

    def count(name, fn):
        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(F, "calculate_fid_given_dataset", count("fid", real_fid))
    monkeypatch.setattr(FD, "calculate_fidelity_given_dataset", count("fidelity", real_fidelity))
    plain = _train_once(tmp_path, monkeypatch, capsys, extra=False)
    assert calls == {"fid": 1, "fidelity": 0} and "fidelity:" not in plain
    assert plain.count("calculating fid...") == 1 and len(re.findall(r"^fid: (\S+)$", plain, flags=re.M)) == 1
    extra = _train_once(tmp_path, monkeypatch, capsys, extra=True)
    assert calls == {"fid": 1, "fidelity": 1}
    lines = extra.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("fidelity: ")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("fid: ")
    m = re.fullmatch(r"fidelity: precision (\S+) recall (\S+) density (\S+) coverage (\S+) kid (\S+) \+- (\S+)", lines[at[0]])
    assert m and all(math.isfinite(float(v)) for v in m.groups())
    assert all(0.0 <= float(v) <= 1.0 for v in (m.group(1), m.group(2), m.group(4)))
    assert math.isfinite(float(re.findall(r"^fid: (\S+)$", extra, flags=re.M)[0]))
    # apart from that line the two runs print the same kinds of lines in the same order
    kinds = lambda text: [l.split()[0] for l in text.splitlines() if l.strip() and not l.startswith("fidelity: ")]
    assert kinds(plain) == kinds(extra)


# ------------------------------------------------------------------------------------------------ errors
def test_errors():
    from sivae_hip import fidelity as FD
    real, fake = _sets(9, 70, 67, 19)
    x, y = _dev(real), _dev(fake)
    for bad_value in (float("nan"), float("inf"), float("-inf")):
        bad = x.clone()
        bad[4, 33] = bad_value
        for call in (lambda: FD.sqdist_matrix(bad, y), lambda: FD.knn_sqdist(bad), lambda: FD.knn_sqdist(y, bad, k=1),
                     lambda: FD.count_within(y, bad, torch.ones(9, dtype=torch.float64, device=DEV)),
                     lambda: FD.prdc(bad, y), lambda: FD.kid(y, bad, subsets=2, subset_size=5)):
            with pytest.raises(ValueError, match="non-finite"):
                call()
    for call in (lambda: FD.knn_sqdist(x.cpu()), lambda: FD.prdc(x, y.cpu()), lambda: FD.sqdist_matrix(x.cpu(), y),
                 lambda: FD.count_within(y, x, torch.ones(9, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for k in (0, 9):
        with pytest.raises(ValueError, match="k must be in 1 .. 8"):
            FD.knn_sqdist(y, k=k)
        with pytest.raises(ValueError, match="k must be in 1 .. 8"):
            FD.prdc(y, y, k=k)
    with pytest.raises(ValueError, match="neighbours asked for"):
        FD.knn_sqdist(x[:3], k=3)                                  # n = k: a row has only n - 1 others
    with pytest.raises(ValueError, match="neighbours asked for"):
        FD.prdc(y, x[:4], k=4)
    assert tuple(FD.knn_sqdist(x[:4], k=3).shape) == (4, 3)        # n = k + 1 is enough
    assert tuple(FD.knn_sqdist(x, y[:3], k=3).shape) == (9, 3)     # cross: k rows are enough
    with pytest.raises(TypeError):
        FD.knn_sqdist(x.double())
    with pytest.raises(ValueError, match="dimensions differ"):
        FD.sqdist_matrix(x, y[:, :50])
    with pytest.raises(ValueError, match="radii"):
        FD.count_within(y, x, torch.ones(8, dtype=torch.float64, device=DEV))


# ------------------------------------------------------------------------------------------------ guarded
def test_guarded(monkeypatch):
    """every new op on guarded, poisoned outputs and exact workspaces: nothing is written outside a tensor, and no
    element that is read was left unwritten (a poisoned element would not compare equal to the unguarded run)"""
    from sivae_hip import fidelity as FD
    from sivae_hip import ops
    real, fake = _sets(*RECORDED)
    x, y, xs = _dev(real), _dev(fake), _strided(real)
    ri, fi = FD.kid_indices(130, 97, subsets=3, subset_size=70, seed=0)
    g2 = torch.Generator().manual_seed(9)
    act = torch.rand(20, 67, 2, 2, generator=g2).to(DEV)
    _lower_budget(monkeypatch, 130, 67)

    def run():
        p = FD.prdc(x, y, k=3)
        bank = FD.FeatureBank(67, DEV, 30).update(x[:25]).update(act)
        return (FD.sqdist_matrix(x, y), FD.sqdist_matrix(xs), FD.knn_sqdist(x, k=8), FD.knn_sqdist(y, xs, k=1),
                FD.count_within(y, x, p["radii_real"]), p["radii_real"], p["radii_fake"],
                torch.tensor([p[n] for n in ("precision", "recall", "density", "coverage")]),
                torch.tensor(FD.kid(x, y, indices=(ri, fi))), ops.feat_row_sqnorm(xs), bank.rows().clone())

    plain = run()
    with guarded(ops, FD) as g:
        kept = run()
        damage = g.verify()
    assert damage == [], "\n" + describe(damage)
    for a, b in zip(plain, kept):
        assert a.shape == b.shape and torch.equal(a, b)
