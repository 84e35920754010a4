"""CPU-side checks of FID on the device (csrc/fid.hip, sivae_hip/fid.py): the numpy oracle tests/fid_oracle.py against
the fixture recorded from the reference (tests/golden/fid.npz), the argument validation of the three entry points (every
call returns before any launch), and the Python surface."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import fid_oracle as FO
from sivae_hip import fid as F
from sivae_hip import lib, ops
from support import fid_features as FX

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53


# ------------------------------------------------------------------------------------------------ oracle vs fixture
@pytest.mark.parametrize("d,n", FX.FULL_RANK + (FX.RANK_DEFICIENT,))
def test_oracle_moments_against_the_reference(d, n):
    p = FX.pair(d, n)
    for side in "12":
        act, mu_ref, sigma_ref = p["act" + side], p["mu" + side], p["sigma" + side]
        assert act.shape == (n, d) and act.dtype == np.float32 and (act >= 0).all()
        mu, sigma = FO.centred_moments(act)
        # the reference's mean is a float32 pairwise sum of non-negative float32 values: (log2 n + 2) roundings
        assert mu_ref.dtype == np.float32
        assert (np.abs(mu - mu_ref) <= (np.log2(n) + 2) * EPS32 * mu).all()
        err = np.abs(sigma - sigma_ref).max() / np.abs(sigma_ref).max()
        dev = FO.uncentred_deviation(act)
        print("(%d, %d) side %s: oracle sigma vs reference %.2e, uncentred vs centred %.2e" % (d, n, side, err, dev))
        assert err <= 8 * EPS64                      # (the same np.cov on the same values)
        # the uncentred fp64 form loses (mean^2 + var) / var of a rounding per term; these features: well below 1e-12
        assert dev <= 1e-12
        mu_u, _ = FO.uncentred_moments(act)
        assert np.abs(mu_u - mu).max() <= 4 * EPS64 * np.abs(mu).max() * np.log2(n)


def test_oracle_state_is_additive_and_one_row_gives_nan():
    act = FX.pair(48, 200)["act1"]
    n, s, G = FO.moment_state(act)
    n1, s1, G1 = FO.moment_state(act[:77])
    n2, s2, G2 = FO.moment_state(act[77:])
    assert n1 + n2 == n and np.allclose(s1 + s2, s, rtol=1e-14, atol=0) and np.allclose(G1 + G2, G, rtol=1e-13, atol=0)
    mu, sigma = FO.uncentred_moments(act[:1])
    assert np.array_equal(mu, act[0].astype(np.float64)) and np.isnan(sigma).all()
    with pytest.warns(RuntimeWarning):
        assert np.isnan(np.cov(act[:1].astype(np.float64), rowvar=False)).all()


@pytest.mark.parametrize("d,n", FX.FULL_RANK)
def test_oracle_distance_full_rank(d, n):
    p = FX.pair(d, n)
    mine = FO.frechet_distance(p["mu1"], p["sigma1"], p["mu2"], p["sigma2"])
    rel = abs(mine - p["fid"]) / abs(p["fid"])
    print("(%d, %d): symmetric form vs the reference function: %.2e relative" % (d, n, rel))
    assert rel <= 1e-12
    assert p["sqrtm_imag"] == 0.0
    # the reference's own flow takes |mu1 - mu2|^2 in float32: the means' difference is rounded (d roundings of size
    # eps32 max|mu|), then a float32 dot product
    diff = p["mu1"].astype(np.float64) - p["mu2"].astype(np.float64)
    norm2 = float(diff.dot(diff))
    slack = EPS32 * (2 * np.sqrt(norm2 * d) * float(max(p["mu1"].max(), p["mu2"].max())) + (d + 2) * norm2)
    assert abs(p["fid_f32"] - p["fid"]) <= slack


def test_oracle_distance_rank_deficient():
    d, n = FX.RANK_DEFICIENT
    p = FX.pair(d, n)
    mine = FO.frechet_distance(p["mu1"], p["sigma1"], p["mu2"], p["sigma2"])
    rel = abs(mine - p["fid"]) / abs(p["fid"])
    print("(%d, %d): symmetric form vs the reference function: %.2e relative; sqrtm's imaginary parts %.1e"
          % (d, n, rel, p["sqrtm_imag"]))
    assert np.isfinite(mine) and rel <= 1e-6
    assert np.linalg.matrix_rank(p["sigma1"]) == n - 1


def test_oracle_on_the_loader_case():
    """the reference's statistics of the first num_images images of a loader whose last batch is cut"""
    batches, net, num, b, mu_ref, sigma_ref = FX.loader_case()
    assert sum(x.shape[0] for x, _ in batches) > num and num % b != 0
    with torch.no_grad():
        feats = torch.cat([torch.nn.functional.adaptive_avg_pool2d(net(x)[0], (1, 1)).flatten(1) for x, _ in batches])
    act = feats.numpy()[:num]
    assert (act >= 0).all() and act.shape == (num, 16)
    mu, sigma = FO.centred_moments(act)
    assert (np.abs(mu - mu_ref) <= (np.log2(num) + 2) * EPS32 * mu).all()
    assert np.abs(sigma - sigma_ref).max() <= 8 * EPS64 * np.abs(sigma_ref).max()


# ------------------------------------------------------------------------------------------------ entry points
def test_fid_entry_points_validate_arguments():
    """null and misaligned pointers, d = 0, d > 8192, negative n, short strides, a flag outside {0, 1}: the documented
    codes, before any launch (no device here), in the manner of test_pc_emd_host.py"""
    L = lib.load()
    null, one, odd4, odd8 = None, ctypes.c_void_p(16), ctypes.c_void_p(18), ctypes.c_void_p(20)
    ok = dict(A=one, stride=8, n=4, d=8, G=one, s=one, stream=null)

    def mo(**kw):
        a = dict(ok, **kw)
        return L.sivae_fid_moments(*[a[k] for k in ok])

    for k in ("A", "G", "s"):
        assert mo(**{k: null}) == -1, k
    assert mo(d=0) == -2 and mo(d=-1) == -2 and mo(d=8193, stride=8193) == -2 and mo(n=-1) == -2
    assert mo(stride=7) == -2
    assert mo(A=odd4) == -2 and mo(G=odd8) == -2 and mo(s=odd8) == -2
    assert mo(n=0) == 0                                     # nothing to add: no launch

    okf = dict(G=one, s=one, n=4, d=8, mu=one, sigma=one, stream=null)

    def fi(**kw):
        a = dict(okf, **kw)
        return L.sivae_fid_finalize(*[a[k] for k in okf])

    for k in ("G", "s", "mu", "sigma"):
        assert fi(**{k: null}) == -1, k
        assert fi(**{k: odd8}) == -2, k
    assert fi(d=0) == -2 and fi(d=8193) == -2 and fi(n=0) == -2 and fi(n=-5) == -2

    okx = dict(X=one, ldx=8, Y=one, ldy=8, C=one, ldc=8, K=4, M=8, N=8, sym=0, stream=null)

    def xy(**kw):
        a = dict(okx, **kw)
        return L.sivae_fid_xty_f64(*[a[k] for k in okx])

    for k in ("X", "Y", "C"):
        assert xy(**{k: null}) == -1, k
        assert xy(**{k: odd8}) == -2, k
    for k in ("K", "M", "N"):
        assert xy(**{k: 0}) == -2 and xy(**{k: -2}) == -2, k
    assert xy(M=8193, ldx=8193) == -2 and xy(N=8193, ldy=8193, ldc=8193) == -2
    assert xy(ldx=7) == -2 and xy(ldy=7) == -2 and xy(ldc=7) == -2
    assert xy(sym=2) == -6 and xy(sym=-1) == -6
    assert xy(sym=1, M=4, ldx=4) == -2                      # the symmetric form is square
    assert L.sivae_abi_version() == 1


def test_header_cites_the_reference_lines():
    text = open(lib.HEADER_PATH).read()
    part = text[text.index("fid.hip"):]
    for name in ("sivae_fid_moments", "sivae_fid_finalize", "sivae_fid_xty_f64"):
        assert name in part
    assert len(re.findall(r"fid_score\.py:\d+", part)) >= 3


# ------------------------------------------------------------------------------------------------ Python surface
def test_signature_is_the_references_plus_two_keywords():
    """the reference's parameter names, in its order (soft_intro_vae/metrics/fid_score.py:454)"""
    params = inspect.signature(F.calculate_fid_given_dataset).parameters
    assert list(params) == ["dataloader", "model_s", "batch_size", "cuda", "dims", "device", "num_images", "inception",
                            "real_stats"]
    assert params["inception"].default is None and params["real_stats"].default is None
    assert all(params[k].default is inspect.Parameter.empty for k in list(params)[:7])
    assert list(inspect.signature(F.ActivationStatistics.__init__).parameters) == ["self", "dims", "device", "flush_rows"]
    assert inspect.signature(F.ActivationStatistics.__init__).parameters["flush_rows"].default == 1024
    assert list(inspect.signature(F.frechet_distance).parameters) == ["mu1", "sigma1", "mu2", "sigma2"]
    assert list(inspect.signature(F.ActivationStatistics.finalize).parameters) == ["self", "num"]


def test_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.ActivationStatistics(16, torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fid_xty(torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 4, dtype=torch.float64))
    with pytest.raises(TypeError, match="float32"):
        ops.fid_moments(torch.zeros(4, 4, dtype=torch.float64), 4, torch.zeros(4, 4), torch.zeros(4))
    if not torch.cuda.is_available():
        p = FX.pair(16, 64)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            F.frechet_distance(p["mu1"], p["sigma1"], p["mu2"], p["sigma2"])
    for bad in (0, 8193):
        with pytest.raises(ValueError, match="8192"):
            ops.fid_state(bad, torch.device("cpu"))
    # the module's idiom: allocation through ops' torch (what tests/support/guard.py patches), none in fid.py
    src = inspect.getsource(F)
    assert "torch.empty" not in src and "torch.zeros" not in src and ".clone()" not in src


def test_trainer_switches():
    import train_soft_intro_vae as T
    src = inspect.getsource(T._calculate_fid)
    assert 'os.environ.get("SIVAE_FID", "device")' in src or 'os.environ.get("SIVAE_FID", "reference")' in src
    assert 'os.environ.get("SIVAE_FID_CACHE_REAL", "0") == "1"' in src
    assert "from metrics.fid_score import calculate_fid_given_dataset" in src
    assert T.FID_ARGS == dict(dims=2048, num_images=50000) and T.FID_INCEPTION is None
    readme = open(os.path.join(os.path.dirname(lib.HEADER_PATH), "..", "README.md")).read()
    assert "SIVAE_FID=" in readme and "SIVAE_FID_CACHE_REAL" in readme


def test_trainer_branch_dispatch(monkeypatch):
    """_calculate_fid without a device: the default goes to sivae_hip.fid and recomputes the real side every pass,
    SIVAE_FID_CACHE_REAL=1 keeps the first pass's, SIVAE_FID=reference makes the reference's call with its arguments"""
    import sys
    import types

    import train_soft_intro_vae as T
    log = []
    net = types.SimpleNamespace(to=lambda device: log.append(("to", device)))
    monkeypatch.setattr(T, "FID_INCEPTION", net)
    monkeypatch.setattr(F, "real_statistics", lambda loader, inception, dims, device, num: log.append(
        ("real", inception is net, dims, num)) or ("mu%d" % len(log), "sigma"))
    monkeypatch.setattr(F, "calculate_fid_given_dataset", lambda *a, **k: log.append(("fid", a, k)) or 1.5)
    monkeypatch.delenv("SIVAE_FID", raising=False)
    monkeypatch.delenv("SIVAE_FID_CACHE_REAL", raising=False)
    kept = {}
    for _ in range(2):
        assert T._calculate_fid("loader", "model", 50, "dev", kept) == 1.5
    assert [e[0] for e in log] == ["to", "real", "fid"] * 2 and kept == {}
    assert log[1] == ("real", True, 2048, 50000)
    a, k = log[2][1:]
    assert a == ("loader", "model", 50) and k == dict(cuda=True, dims=2048, device="dev", num_images=50000, inception=net,
                                                      real_stats=log[2][2]["real_stats"])
    del log[:]
    monkeypatch.setenv("SIVAE_FID_CACHE_REAL", "1")
    T._calculate_fid("loader", "model", 50, "dev", kept)
    T._calculate_fid("loader", "model", 50, "dev", kept)
    assert [e[0] for e in log] == ["to", "real", "fid", "to", "fid"]
    assert log[2][2]["real_stats"] is log[4][2]["real_stats"] is kept["stats"]
    del log[:]
    monkeypatch.setenv("SIVAE_FID", "reference")
    stub = types.ModuleType("metrics.fid_score")
    stub.calculate_fid_given_dataset = lambda *a, **k: log.append((a, k)) or 2.5
    monkeypatch.setitem(sys.modules, "metrics", types.ModuleType("metrics"))
    monkeypatch.setitem(sys.modules, "metrics.fid_score", stub)
    assert T._calculate_fid("loader", "model", 50, "dev", {}) == 2.5
    assert log == [(("loader", "model", 50), dict(cuda=True, dims=2048, device="dev", num_images=50000))]
    monkeypatch.setenv("SIVAE_FID", "host")
    with pytest.raises(ValueError, match="SIVAE_FID"):
        T._calculate_fid("loader", "model", 50, "dev", {})
