"""Host-side checks (no GPU) of the style variant's model class: the drop-in model.py has the reference's surface and
initial state (tests/golden/style_model.npz, recorded from the real reference), the new entry points of mapping.hip and
linear.hip validate their arguments before any launch, and CPU tensors are refused by the kernels' path and accepted by
the torch restatement."""
import ctypes
import hashlib
import inspect
import os

import numpy as np
import pytest
import torch

import style_model_fixture as MF
import style_net_fixture as NF
from sivae_hip import lib, ops, style


@pytest.fixture(scope="module")
def fx():
    return MF.Fixture()


@pytest.fixture(scope="module")
def model():
    return MF.import_model()


def test_model_imports_and_has_the_reference_surface(fx, model):
    names = fx.json("names")
    for name, sig in names["helpers"].items():
        assert str(inspect.signature(getattr(model, name))) == sig, name
    for name, sig in names["methods"].items():
        assert str(inspect.signature(getattr(model.SoftIntroVAEModelTL, name))) == sig, name
    assert str(inspect.signature(model.DLatent.__init__)) == names["dlatent"]
    assert model.FUSED is True


def test_state_dict_keys_order_and_initial_bits(fx, model):
    kw, keys = fx.json("model/kwargs"), fx.json("model/keys")
    assert keys[-1][0] == "dlatent_avg.buff"
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = model.SoftIntroVAEModelTL(**kw)
        sd = m.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == keys
        flat = np.concatenate([v.numpy().ravel() for v in sd.values()])
        assert flat.dtype == np.float32
        if seed == 0:
            assert np.array_equal(flat, fx["model/init0"])
        else:
            assert hashlib.sha256(flat.tobytes()).hexdigest() == fx["model/init1_sha256"]
    for name in MF.LAST:
        t = getattr(m, name)
        assert isinstance(t, torch.Tensor) and t.dim() == 0 and float(t) == 0.0, name
    assert (m.layer_count, m.latent_size, m.scale, m.gamma_r) == (kw["layer_count"], kw["latent_size"], kw["scale"], kw["gamma_r"])
    assert (m.beta_kl, m.beta_rec, m.beta_neg) == (kw["beta_kl"], kw["beta_rec"], kw["beta_neg"])
    assert (m.dlatent_avg_beta, m.style_mixing_prob, m.truncation_psi, m.truncation_cutoff) == (0.995, 0.9, None, None)
    # lerp walks parameters only: the buffer of dlatent_avg is not among them
    assert len(m._averaged()) == len(list(m.parameters())) == len(keys) - len(list(m.buffers()))
    assert not any(p is m.dlatent_avg.buff for p in m._averaged())


def test_set_model_require_grad(model, fx):
    m = model.SoftIntroVAEModelTL(**fx.json("model/kwargs"))
    model.set_model_require_grad(m.encoder, False)
    assert not any(p.requires_grad for p in m.encoder.parameters()) and all(p.requires_grad for p in m.decoder.parameters())


def test_fixture_holds_the_branches_it_is_there_for(fx):
    """re-asserted from the stored values, so that a vanished branch cannot pass silently"""
    fwd, gen = fx.runs("forward"), fx.runs("generate")
    assert len(fwd) == 9 and len(gen) == 4
    L = 2 * NF.CFG["layer_count"]
    metas = [fx.json(r + "/meta") for r in fwd + gen]
    assert {(m["branch"], m["lod"], m["blend"]) for m in metas if m["kind"] == "forward"} == {
        (b, lod, blend) for b in ("vae", "e_train", "d_train") for lod, blend in ((2, 1), (2, 0.75), (1, 1))}
    for m in metas:
        if m.get("branch") == "e_train":
            assert 1e-3 <= m["last_expelbo_rec"] <= 0.999 and 1e-3 <= m["last_expelbo_fake"] <= 0.999, m
        if m.get("branch") == "d_train":
            assert m["last_kl_diff"] == MF.LAST_IN["last_fake_kl"] - MF.LAST_IN["last_real_kl"]
        # no parameter's gradient vanishes, but for the first decoder layer's bias where the generator reports it so
        assert set(m["zero_grad_keys"]) <= {"decoder.decode_block.0.bias_1"}
        assert len(m["grad_keys"]) > 0
    for r in fwd + gen:
        m = fx.json(r + "/meta")
        shapes = {k: s for k, s in fx.json("model/keys")}
        grads = fx.grads(r, shapes)
        for k, g in grads.items():
            assert (float(g.abs().max()) > 0) == (k not in m["zero_grad_keys"]), (r, k)
    taken = [d for m in metas for d in m["mixing"]]
    assert any(t and c < L for t, c in taken) and any(not t for t, _ in taken)
    for kind in ("generate",):
        took = [fx.json(r + "/meta")["mixing"][0][0] for r in fx.runs(kind)]
        assert True in took and False in took
    # the average moved in every run (beta = 0.995 everywhere)
    for r in fwd + gen:
        assert not np.array_equal(fx[r + "/buff"], fx["model/buff_in"]), r


def test_fixture_is_smaller_than_the_network_fixture():
    assert os.path.getsize(MF.PATH) < os.path.getsize(os.path.join(NF.HERE, "golden", "style_net.npz"))
    assert os.path.getsize(MF.PATH) < 1 << 20


def test_new_entry_points_validate_arguments():
    """every call returns before any kernel launch (there is no GPU here): null -> -1, shape -> -2, workspace -> -4,
    range -> -5, mode / slope outside [0, 1] -> -6"""
    L = lib.load()
    null, one, odd = None, ctypes.c_void_p(16), ctypes.c_void_p(18)
    f = L.sivae_linear_lrelu_fwd
    assert f(null, one, one, one, 0.2, 8, 64, 64, one, 1 << 20, null) == -1
    assert f(one, one, one, one, 0.2, 8, 66, 64, one, 1 << 20, null) == -2
    assert f(one, one, one, one, 0.2, 128, 8192, 512, one, 16, null) == -4
    assert f(one, one, one, one, 1.5, 8, 64, 64, one, 1 << 20, null) == -6
    assert f(one, one, one, one, -0.1, 8, 64, 64, one, 1 << 20, null) == -6
    assert f(one, one, one, one, float("nan"), 8, 64, 64, one, 1 << 20, null) == -6
    # (the existing entry point keeps its signature and codes)
    assert L.sivae_linear_fwd(null, one, null, one, 0, 8, 64, 64, one, 1 << 20, null) == -1
    g = L.sivae_lrelu_bias_bwd
    assert g(null, one, 0.2, one, one, 4, 8, null) == -1
    assert g(one, one, 0.2, one, one, 0, 8, null) == -2 and g(one, one, 0.2, one, one, 4, 0, null) == -2
    assert g(one, one, 1.5, one, one, 4, 8, null) == -6 and g(one, one, -1.0, one, one, 4, 8, null) == -6
    assert g(one, odd, 0.2, one, one, 4, 8, null) == -2  # (4-byte alignment)
    assert g(one, one, 0.2, one, one, 1 << 20, 1 << 12, null) == -5
    assert g(one, one, 0.2, null, null, 4, 8, null) == 0  # (nothing asked for: nothing launched)
    p = L.sivae_pixel_norm_fwd
    assert p(null, one, one, 2, 8, 1e-8, null) == -1 and p(one, one, null, 2, 8, 1e-8, null) == -1
    assert p(one, one, one, 0, 8, 1e-8, null) == -2 and p(one, one, one, 2, 0, 1e-8, null) == -2
    assert p(one, one, one, 2, 8, -1.0, null) == -2 and p(one, odd, one, 2, 8, 1e-8, null) == -2
    assert p(one, one, one, 1 << 16, 1 << 16, 1e-8, null) == -5
    q = L.sivae_pixel_norm_bwd
    assert q(one, null, one, one, 2, 8, null) == -1 and q(one, one, one, one, 2, -1, null) == -2
    assert q(one, one, one, one, 1 << 16, 1 << 16, null) == -5
    s = L.sivae_styles_fwd
    #        s    s2    cut avg  upd  w    trunc psi tcut out  B  L  Z
    assert s(null, null, 0, null, 0, 0.0, 0, 0.7, 0, one, 2, 6, 8, null) == -1
    assert s(one, null, 0, null, 0, 0.0, 0, 0.7, 0, null, 2, 6, 8, null) == -1
    assert s(one, null, 0, null, 1, 0.005, 0, 0.7, 0, one, 2, 6, 8, null) == -1   # an update without the average
    assert s(one, null, 0, null, 0, 0.0, 1, 0.7, 4, one, 2, 6, 8, null) == -1     # a truncation without it
    assert s(one, null, 0, null, 0, 0.0, 0, 0.7, 0, one, 2, 0, 8, null) == -2
    assert s(one, one, 7, null, 0, 0.0, 0, 0.7, 0, one, 2, 6, 8, null) == -2       # mixing cutoff above L
    assert s(one, null, 0, one, 0, 0.0, 1, 0.7, 7, one, 2, 6, 8, null) == -2       # truncation cutoff above L
    assert s(one, null, 0, one, 2, 0.0, 0, 0.7, 0, one, 2, 6, 8, null) == -6       # flags are 0 / 1
    assert s(one, null, 0, one, 0, 0.0, 3, 0.7, 0, one, 2, 6, 8, null) == -6
    assert s(one, null, 0, one, 1, 1.5, 0, 0.7, 0, one, 2, 6, 8, null) == -6       # 1 - beta outside [0, 1]
    assert s(one, null, 0, one, 1, -0.5, 0, 0.7, 0, one, 2, 6, 8, null) == -6
    assert s(one, null, 0, null, 0, 0.0, 0, 0.7, 0, one, 1 << 14, 1 << 6, 1 << 12, null) == -5
    t = L.sivae_styles_bwd
    assert t(null, 0, 0, 0, 0.7, 0, one, null, 2, 6, 8, null) == -1
    assert t(one, 2, 0, 0, 0.7, 0, one, null, 2, 6, 8, null) == -6
    assert t(one, 0, 0, 0, 0.7, 0, one, one, 2, 6, 8, null) == -6                  # ds2 of a forward without s2
    assert t(one, 1, 9, 0, 0.7, 0, one, one, 2, 6, 8, null) == -2
    assert t(one, 0, 0, 1, 0.7, -1, one, null, 2, 6, 8, null) == -2
    assert t(one, 0, 0, 0, 0.7, 0, null, null, 2, 6, 8, null) == 0
    # which side of the contraction split a layer width is on (the LeakyReLU sits in the GEMM kernel or in the reduce)
    assert L.sivae_linear_workspace_bytes(2, 64, 32) == 16 and L.sivae_linear_workspace_bytes(33, 512, 512) > 16


def test_python_wrappers_validate_before_the_library():
    x = torch.zeros(2, 8)
    for call in (lambda: ops.pixel_norm_fwd(x), lambda: ops.pixel_norm_bwd(x, x, torch.zeros(2)),
                 lambda: ops.linear_lrelu_fwd(x, torch.zeros(4, 8), torch.zeros(4)),
                 lambda: ops.lrelu_bias_bwd(x, x), lambda: ops.styles_fwd(x, 6), lambda: ops.styles_bwd(torch.zeros(2, 6, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="float32"):
        ops.pixel_norm_fwd(x.double())


def test_cpu_tensors_are_refused_by_the_kernels_and_accepted_by_the_restatement(model, monkeypatch):
    mu, logvar = torch.randn(3, 8), 0.1 * torch.randn(3, 8)
    x, r = torch.randn(3, 2, 4, 4), torch.randn(3, 2, 4, 4)
    assert model.FUSED
    for call in (lambda: model.calc_kl(logvar, mu, reduce="mean"), lambda: model.reparameterize(mu, logvar),
                 lambda: model.calc_reconstruction_loss(x, r, "mse", "mean"),
                 lambda: style.mapping(mu, [torch.zeros(8, 8)], [torch.zeros(8)], True),
                 lambda: style.styles(mu, 6)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    monkeypatch.setattr(model, "FUSED", False)
    kl = -0.5 * (1 + logvar - mu.pow(2) - logvar.exp()).sum(1)
    assert torch.equal(model.calc_kl(logvar, mu, reduce="none"), kl)
    assert torch.equal(model.calc_kl(logvar, mu, reduce="mean"), kl.mean())
    assert torch.equal(model.calc_kl(logvar, mu), kl.sum())
    rows = ((x - r) ** 2).view(3, -1).sum(1)
    assert torch.allclose(model.calc_reconstruction_loss(x, r, "mse", "none"), rows)
    assert torch.allclose(model.calc_reconstruction_loss(x, r, "mse", "mean"), rows.mean())
    assert torch.allclose(model.calc_reconstruction_loss(x, r, "l1", "sum"), (x - r).abs().sum())
    with pytest.raises(NotImplementedError):
        model.calc_reconstruction_loss(x, r, "mse", "avg")
    with pytest.raises(NotImplementedError):
        model.calc_reconstruction_loss(x, r, "huber", "sum")
    torch.manual_seed(3)
    z = model.reparameterize(mu, logvar)
    torch.manual_seed(3)
    assert torch.equal(z, mu + torch.randn_like(mu) * torch.exp(0.5 * logvar))
