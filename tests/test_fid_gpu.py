"""FID on the device (csrc/fid.hip, sivae_hip/fid.py) on an MI355X: the fp64 moment kernel against np.mean / np.cov, its
independence of how the rows were fed, truncation and merge, the fp64 product in both forms, the Frechet distance against
the values recorded from the reference (tests/golden/fid.npz), the whole pass with stand-in networks, the trainer's
branch, and a guarded run.

Gates.  MOMENTS: 16 x the worst deviation, over every input of this file's moment tests, of the oracle's uncentred formula
(the finalize kernel's, in numpy) from the centred np.cov, relative to max|sigma|: both are fp64 evaluations of the same
quantity in different summation orders, and 16 is the project's margin for one more order.  DISTANCE, full rank: 1e-10
relative, a cap on c d eps lambda_max (a backward-stable symmetric solver's eigenvalue error) passed through the square root
at lambda_min / lambda_max >= 1e-6 (asserted when the fixture was recorded), d <= 192.  Rank deficient: 1e-6, the quantity
being conditioned like sqrt(eps) there (the reference's own result carries imaginary parts of 2e-8)."""
import functools
import math
import os
import re
import warnings

import numpy as np
import pytest
import torch

import fid_oracle as FO
from support import fid_features as FX
from support.guard import describe, guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DIMS = (1, 15, 16, 17, 48, 80, 192)
ROWS = (1, 3, 4, 5, 50, 67)
EPS64 = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _acts(d, n, seed=0, pad=0):
    """float32 [n, d + pad]: relu(z W + b), non-negative and correlated like pooled post-ReLU features"""
    g = np.random.Generator(np.random.PCG64(1000003 * d + 101 * n + seed))
    w = np.eye(d + pad) + 0.5 * g.standard_normal((d + pad, d + pad)) / math.sqrt(d + pad)
    a = np.maximum(g.standard_normal((n, d + pad)) @ w + 0.25 + 0.5 * g.random(d + pad), 0.0).astype(np.float32)
    a.setflags(write=False)
    return a


BIG, STRIDED, SEQ = (2048, 64), (80, 67), (80, 130)


@functools.lru_cache(maxsize=None)
def _gate():
    inputs = [_acts(d, n) for d in DIMS for n in ROWS if n > 1]
    inputs += [_acts(*BIG), _acts(*STRIDED, pad=13)[:, 5:85], _acts(*STRIDED, pad=13)[:50, 5:85], _acts(*SEQ),
               _acts(*SEQ)[:100], np.concatenate([_acts(*STRIDED)[:40], _acts(*STRIDED)])]
    worst = max(FO.uncentred_deviation(a) for a in inputs)
    print("moment gate: 16 x %.3e" % worst)
    assert 0 < worst < 1e-12
    return 16 * worst


def _check_moments(tag, mu, sigma, act):
    """(mu, sigma) device fp64 against np.mean / np.cov of act in float64, under the gate"""
    mu_ref, sigma_ref = FO.centred_moments(act)
    mu, sigma = mu.cpu().numpy(), sigma.cpu().numpy()
    assert mu.dtype == np.float64 and sigma.dtype == np.float64 and sigma.shape == sigma_ref.shape
    e_mu = np.abs(mu - mu_ref).max() / np.abs(mu_ref).max()
    assert np.array_equal(sigma, sigma.T, equal_nan=True), tag
    if act.shape[0] == 1:
        assert np.isnan(sigma).all() and np.isnan(sigma_ref).all(), tag
        print("%s: mu %.2e (gate %.2e), sigma NaN as np.cov's" % (tag, e_mu, _gate()))
    else:
        e_sigma = np.abs(sigma - sigma_ref).max() / np.abs(sigma_ref).max()
        print("%s: mu %.2e, sigma %.2e (gate %.2e)" % (tag, e_mu, e_sigma, _gate()))
        assert e_sigma <= _gate(), tag
    assert e_mu <= _gate(), tag


def _stats(act, flush_rows=1024, batch=None):
    from sivae_hip import fid as F
    st = F.ActivationStatistics(act.shape[1], DEV, flush_rows=flush_rows)
    x = torch.from_numpy(np.array(act)).to(DEV)
    for i in range(0, x.shape[0], batch or x.shape[0]):
        st.update(x[i:i + (batch or x.shape[0])])
    return st


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("d", DIMS)
def test_moments_against_numpy(d):
    """one MFMA tile, partial tiles, a diagonal plus an off-diagonal block tile (80, 192), K tails (every n)"""
    for n in ROWS:
        act = _acts(d, n)
        st = _stats(act)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            mu, sigma = st.finalize()
        assert (n == 1) == any(issubclass(x.category, RuntimeWarning) for x in w)
        _check_moments("d %d n %d" % (d, n), mu, sigma, act)
        cnt, s, G = st.state()
        n_ref, s_ref, G_ref = FO.moment_state(act)
        assert cnt == n_ref
        G = G.cpu().numpy()
        tile = np.arange(d) // 64
        upper = tile[:, None] <= tile[None, :]
        assert (G[~upper] == 0).all()                     # the tiles below the diagonal are never touched
        assert np.abs(np.where(upper, G - G_ref, 0)).max() <= max(_gate(), 4 * n * EPS64) * np.abs(G_ref).max()
        assert np.abs(s.cpu().numpy() - s_ref).max() <= max(_gate(), 4 * n * EPS64) * np.abs(s_ref).max()


def test_moments_2048():
    act = _acts(*BIG)
    mu, sigma = _stats(act).finalize()
    _check_moments("d 2048 n 64", mu, sigma, act)


def test_moments_strided_input():
    """rows with a stride and an offset that is only 4-byte aligned, straight into the kernel"""
    from sivae_hip import ops
    base = _acts(*STRIDED, pad=13)
    x = torch.from_numpy(np.array(base)).to(DEV)[:, 5:85]
    assert x.stride() == (93, 1) and x.data_ptr() % 8 == 4
    G, s = ops.fid_state(80, DEV)
    ops.fid_moments(x, 67, G, s)
    mu, sigma = ops.fid_finalize(G, s, 67)
    _check_moments("strided d 80 n 67", mu, sigma, base[:, 5:85])
    # fewer rows than the tensor holds: the rest is not read into the moments
    G2, s2 = ops.fid_state(80, DEV)
    ops.fid_moments(x, 50, G2, s2)
    mu2, sigma2 = ops.fid_finalize(G2, s2, 50)
    _check_moments("strided d 80 first 50 of 67", mu2, sigma2, base[:50, 5:85])


def test_result_does_not_depend_on_the_batches_or_the_run():
    act = _acts(*SEQ)
    runs = [_stats(act, flush_rows=64, batch=b) for b in (None, 50, 7, None)]
    outs = []
    for st in runs:
        n, s, G = st.state()
        assert n == 130 and st.rows_seen == 130
        outs.append((s, G) + st.finalize())
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    _check_moments("130 rows in blocks of 64", outs[0][2], outs[0][3], act)


def test_finalize_num_cuts_inside_a_block():
    """rows beyond num must not enter the moments (the reference's activations[:num_images])"""
    act = _acts(*SEQ)
    st = _stats(act, flush_rows=64, batch=50)
    mu, sigma = st.finalize(100)                           # inside the second block of 64
    _check_moments("first 100 of 130", mu, sigma, act[:100])
    ref = _stats(act[:100], flush_rows=64)
    for a, b in zip((mu, sigma), ref.finalize()):
        assert torch.equal(a, b)                           # the arithmetic of the truncated sequence itself
    mu_all, sigma_all = st.finalize()                      # the accumulator is unchanged by finalize
    _check_moments("all 130 after a cut", mu_all, sigma_all, act)
    with pytest.raises(ValueError, match="last full block"):
        st.finalize(50)                                    # the first block is in the moments already
    with pytest.raises(ValueError, match="seen"):
        st.finalize(131)


def test_merge_of_two_halves():
    act = _acts(*SEQ)
    a, b = _stats(act[:65], flush_rows=64), _stats(act[65:], flush_rows=64)
    a.merge(b)
    assert a.rows_seen == 130 and b.rows_seen == 65
    mu, sigma = a.finalize()
    _check_moments("merge 65 + 65", mu, sigma, act)


# ------------------------------------------------------------------------------------------------ fp64 product
@pytest.mark.parametrize("K,M,N", [(5, 3, 7), (70, 100, 130), (64, 128, 64), (131, 65, 1)])
def test_xty_plain(K, M, N):
    from sivae_hip import ops
    g = torch.Generator().manual_seed(K * 1000 + M)
    xb, y = torch.randn(K, M + 3, generator=g, dtype=torch.float64), torch.randn(K, N, generator=g, dtype=torch.float64)
    x = xb[:, 2:2 + M]                                      # a row stride
    c = ops.fid_xty(xb.to(DEV)[:, 2:2 + M], y.to(DEV)).cpu()
    ref = x.t() @ y
    bound = 2 * (K + 2) * EPS64 * (x.abs().t() @ y.abs())  # two fp64 dot products of K terms, any order
    err = ((c - ref).abs() / bound).max().item()
    print("x^T y %s: worst error / bound %.3f" % ((K, M, N), err))
    assert c.shape == (M, N) and err <= 1.0


@pytest.mark.parametrize("K,M", [(33, 100), (4, 1), (64, 64), (200, 192)])
def test_xty_symmetric(K, M):
    from sivae_hip import ops
    g = torch.Generator().manual_seed(K * 1000 + M + 1)
    x = torch.randn(K, M, generator=g, dtype=torch.float64)
    c = ops.fid_xty(x.to(DEV), x.to(DEV), symmetric=True).cpu()
    assert torch.equal(c, c.t())                            # the mirror is exact
    bound = 2 * (K + 2) * EPS64 * (x.abs().t() @ x.abs())
    assert ((c - x.t() @ x).abs() <= bound).all()
    # a product that is symmetric only up to rounding (X != Y): the entries on and above the diagonal win
    s = torch.randn(K, K, generator=g, dtype=torch.float64)
    y = (s + s.t()) @ x
    c2 = ops.fid_xty(x.to(DEV), y.to(DEV), symmetric=True).cpu()
    full = ops.fid_xty(x.to(DEV), y.to(DEV)).cpu()
    assert torch.equal(c2, c2.t()) and torch.equal(torch.triu(c2), torch.triu(full))


# ------------------------------------------------------------------------------------------------ distance
@pytest.mark.parametrize("d,n", FX.FULL_RANK)
def test_distance_full_rank(d, n):
    from sivae_hip import fid as F
    p = FX.pair(d, n)
    got = F.frechet_distance(p["mu1"], p["sigma1"], p["mu2"], p["sigma2"])
    rel = abs(got - p["fid"]) / abs(p["fid"])
    print("frechet_distance (%d, %d): %.15g, reference %.15g, %.2e relative (cap 1e-10)" % (d, n, got, p["fid"], rel))
    assert isinstance(got, float) and rel <= 1e-10


def test_distance_rank_deficient():
    from sivae_hip import fid as F
    p = FX.pair(*FX.RANK_DEFICIENT)
    got = F.frechet_distance(p["mu1"], p["sigma1"], p["mu2"], p["sigma2"])
    rel = abs(got - p["fid"]) / abs(p["fid"])
    print("frechet_distance (64, 50): %.15g, reference %.15g, %.2e relative (cap 1e-6)" % (got, p["fid"], rel))
    assert math.isfinite(got) and rel <= 1e-6


def test_distance_takes_numpy_cpu_and_device_inputs():
    from sivae_hip import fid as F
    p = FX.pair(16, 64)
    args = [p[k] for k in ("mu1", "sigma1", "mu2", "sigma2")]
    a = F.frechet_distance(*args)
    b = F.frechet_distance(*[torch.from_numpy(np.array(x)) for x in args])
    c = F.frechet_distance(*[torch.from_numpy(np.array(x)).to(DEV) for x in args])
    assert a == b == c


def test_distance_of_device_statistics():
    """activations -> device moments -> distance, against the reference's value for the same activations (whose means
    are float32: the distance moves by the means' float32 rounding, bounded as in test_fid_host.py, no more)"""
    from sivae_hip import fid as F
    d, n = 48, 200
    p = FX.pair(d, n)
    m1, s1 = _stats(p["act1"], flush_rows=64).finalize()
    m2, s2 = _stats(p["act2"], flush_rows=64).finalize()
    got = F.frechet_distance(m1, s1, m2, s2)
    diff = p["mu1"].astype(np.float64) - p["mu2"].astype(np.float64)
    norm2 = float(diff.dot(diff))
    slack = 2.0 ** -24 * (math.log2(n) + 2) * 2 * 2 * math.sqrt(norm2 * d) * float(max(p["mu1"].max(), p["mu2"].max()))
    print("device statistics -> distance: %.15g, reference %.15g (slack for its float32 means %.1e)"
          % (got, p["fid"], slack))
    assert abs(got - p["fid"]) <= slack + 1e-10 * p["fid"]


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
        self.seen.append((x, out[0]))
        return out


def test_whole_pass_with_stand_ins(monkeypatch):
    from sivae_hip import fid as F
    from sivae_hip import infer, ops, rng
    batches, net, num, b, mu_ref, sigma_ref = FX.loader_case()
    net = _Recording(net.to(DEV))
    model_s = _Generator().to(DEV)

    # the real side against the fixture.  Features: sums of <= 28 non-negative float32 terms (no cancellation), then a
    # mean of 64: any two float32 evaluations differ by at most 2 (28 + 64 + 2) eps32 of the value; a covariance entry
    # moves by at most 4 delta amax n / (n - 1)
    mu, sigma = F.real_statistics(batches, net, 16, DEV, num)
    rows = torch.cat([torch.nn.functional.adaptive_avg_pool2d(o, (1, 1)).flatten(1) for _, o in net.seen])
    assert len(net.seen) == 5 and rows.shape[0] == 120     # the fifth batch is run and cut
    amax = float(rows.max())
    delta = 2 * (28 + 64 + 2) * 2.0 ** -24 * amax
    assert np.abs(mu.cpu().numpy() - mu_ref).max() <= delta + 10 * 2.0 ** -24 * amax   # (+ the reference's float32 mean)
    assert np.abs(sigma.cpu().numpy() - sigma_ref).max() <= 4 * delta * amax * num / (num - 1)
    # ... and, tightly, the oracle on the very features the device produced, truncated as the reference truncates
    mu_o, sigma_o = FO.centred_moments(rows[:num].cpu().numpy())
    gate = 16 * FO.uncentred_deviation(rows[:num].cpu().numpy())
    assert np.abs(mu.cpu().numpy() - mu_o).max() <= gate * np.abs(mu_o).max()
    assert np.abs(sigma.cpu().numpy() - sigma_o).max() <= gate * np.abs(sigma_o).max()

    # the full call; what it hands to frechet_distance is recorded
    handed = []
    real_fd = F.frechet_distance
    monkeypatch.setattr(F, "frechet_distance", lambda *a: handed.append(a) or real_fd(*a))
    net.seen.clear()
    rng.manual_seed(77)
    full = F.calculate_fid_given_dataset(batches, model_s, b, True, 16, DEV, num, inception=net)
    assert isinstance(full, float) and math.isfinite(full) and len(handed) == 1
    assert torch.equal(handed[0][0], mu) and torch.equal(handed[0][1], sigma)        # real side first, as the reference
    gen = net.seen[5:]
    assert len(net.seen) == 5 + math.ceil(num / b)
    # the generated side ran infer.generate's quantised feed on the process-wide stream
    rng.manual_seed(77)
    again = [ops.u8_to_f32(u8) for u8 in infer.generate(model_s, num, b, as_uint8=True, eval_mode=None)]
    assert all(torch.equal(x, y) for (x, _), y in zip(gen, again)) and len(again) == len(gen)
    assert (again[0] * 255 - (again[0] * 255).round()).abs().max() < 1e-3     # k / 255: the quantised feed
    feats = torch.cat([torch.nn.functional.adaptive_avg_pool2d(o, (1, 1)).flatten(1) for _, o in gen])[:num]
    m2_o, s2_o = FO.centred_moments(feats.cpu().numpy())
    gate2 = 16 * FO.uncentred_deviation(feats.cpu().numpy())
    assert np.abs(handed[0][2].cpu().numpy() - m2_o).max() <= gate2 * np.abs(m2_o).max()
    assert np.abs(handed[0][3].cpu().numpy() - s2_o).max() <= gate2 * np.abs(s2_o).max()

    # real_stats= skips the real side and gives the same scalar
    net.seen.clear()
    rng.manual_seed(77)
    short = F.calculate_fid_given_dataset(batches, model_s, b, True, 16, DEV, num, inception=net, real_stats=(mu, sigma))
    assert short == full and len(net.seen) == math.ceil(num / b)
    print("stand-in FID %.12g" % full)


def test_trainer_fid_branch(tmp_path, monkeypatch, capsys):
    """train_soft_intro_vae(with_fid=True) on the synthetic dataset with a stand-in feature network: a finite `fid:` line
    per pass, best_fid kept as the reference loop keeps it (reference train_soft_intro_vae.py:283-296)"""
    import train_soft_intro_vae as T
    _, net, _, _, _, _ = FX.loader_case()
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SIVAE_SYNTHETIC_IMAGES", "16")
    monkeypatch.delenv("SIVAE_FID", raising=False)
    monkeypatch.setattr(T, "FID_ARGS", dict(dims=16, num_images=16))
    monkeypatch.setattr(T, "FID_INCEPTION", net)
    calls = []
    from sivae_hip import fid as F
    real = F.calculate_fid_given_dataset
    monkeypatch.setattr(F, "calculate_fid_given_dataset", lambda *a, **k: calls.append(k) or real(*a, **k))
    T.train_soft_intro_vae(dataset="synthetic-cifar10", z_dim=16, batch_size=8, num_workers=0, num_epochs=2, beta_kl=1.0,
                           beta_rec=1.0, beta_neg=256, seed=5, save_interval=50, device=DEV, with_fid=True)
    out = capsys.readouterr().out
    fids = [float(x) for x in re.findall(r"^fid: (\S+)$", out, flags=re.M)]
    assert out.count("calculating fid...") == 2 and len(fids) == 2 and all(math.isfinite(f) for f in fids)
    assert len(calls) == 2 and all(k["dims"] == 16 and k["num_images"] == 16 for k in calls)   # the device path ran
    saves = os.listdir(tmp_path / "saves") if (tmp_path / "saves").exists() else []
    if fids[1] < fids[0]:
        assert "best fid updated: {} -> {}".format(fids[0], fids[1]) in out
        assert any("_fid_{}_".format(fids[1]) in s for s in saves)
    else:
        assert "best fid updated" not in out and not any("_fid_" in s for s in saves)


# ------------------------------------------------------------------------------------------------ guarded
def test_guarded():
    """every launch of the FID path on guarded, poisoned outputs: nothing is written outside a tensor, and nothing that
    is read was left unwritten (a poisoned element is NaN and fails the checks)"""
    from sivae_hip import fid as F
    from sivae_hip import ops
    act, p = _acts(*STRIDED), FX.pair(16, 64)
    with guarded(ops) as g:
        st = F.ActivationStatistics(80, DEV, flush_rows=32)
        x = torch.from_numpy(np.array(act)).to(DEV)
        for i in range(0, 67, 10):
            st.update(x[i:i + 10])
        mu, sigma = st.finalize()
        other = F.ActivationStatistics(80, DEV, flush_rows=32).update(x[:40])
        other.merge(st)
        mu_m, sigma_m = other.finalize(107)
        d16 = F.frechet_distance(p["mu1"], p["sigma1"], p["mu2"], p["sigma2"])
        c = ops.fid_xty(x.double()[:, :70], x.double()[:, 3:80])
        damage = g.verify()
    assert damage == [], "\n" + describe(damage)
    _check_moments("guarded d 80 n 67", mu, sigma, act)
    _check_moments("guarded merge 40 + 67", mu_m, sigma_m, np.concatenate([act[:40], act]))
    assert abs(d16 - p["fid"]) <= 1e-10 * p["fid"]
    assert torch.isfinite(c).all()
