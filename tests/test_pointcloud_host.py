"""CPU-side checks of the 3-D point-cloud slice: the torch restatement (tests/pc3d_oracle.py) against fixtures recorded
from the reference in float64, the drop-in modules' surface (state_dict keys / shapes, signatures), and the argument
validation of the new entry points (every call returns before any launch)."""
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import pc3d_oracle as O
from sivae_hip import lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


@pytest.mark.parametrize("name", ["pc3d_small", "pc3d_full"])
def test_restatement_equals_reference_fp64(name):
    """the vanilla-VAE objective through the restatement, weights by the recipe, equals the reference's float64 run to
    1e-10 relative: outputs, Chamfer, KL, loss, BatchNorm buffers, every gradient norm and gradient slice"""
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    z, seed = int(fx["meta_z"]), int(fx["meta_seed"])
    sd = O.leaves(O.recipe_state_dict(O.model_specs(z), seed))
    x, eps = torch.from_numpy(fx["x"]), torch.from_numpy(fx["eps"])
    upd = {}
    out = O.vae_objective(sd, x, eps, float(fx["meta_beta_rec"]), float(fx["meta_beta_kl"]), update=upd)
    for k in ("mu", "logvar", "rec", "chamfer", "kl", "loss"):
        assert _rel(out[k].detach().numpy(), fx[k]) <= 1e-10, k
    out["loss"].backward()
    for k in fx.files:
        if k.startswith("gnorm/"):
            g = sd[k[6:]].grad
            assert abs(float(g.norm()) - float(fx[k])) <= 1e-10 * float(fx[k]), k
            sl = fx["gslice/" + k[6:]]
            assert np.abs(g.reshape(-1)[:8].numpy() - sl).max() <= 1e-10 * float(fx[k]), k
        elif k.startswith("buf/"):
            assert _rel(upd[k[4:]].numpy(), fx[k]) <= 1e-10, k
    # eval mode: the running statistics the training pass left behind
    sd.update(upd)
    with torch.no_grad():
        mu_e, lv_e = O.encoder(sd, x, training=False, prefix="encoder.")
    assert _rel(mu_e.numpy(), fx["mu_eval"]) <= 1e-10 and _rel(lv_e.numpy(), fx["logvar_eval"]) <= 1e-10


def test_restatement_chamfer_equals_reference_fp64():
    fx = np.load(os.path.join(GOLD, "pc3d_chamfer.npz"))
    v = O.chamfer(torch.from_numpy(fx["preds"]), torch.from_numpy(fx["gts"]))
    assert _rel(v.numpy(), fx["chamfer"]) <= 1e-10


def test_chamfer_gradient_formula_equals_autograd():
    """the analytic gradient for given indices (what the kernel implements) is autograd's gradient of the restatement"""
    g = torch.Generator().manual_seed(5)
    gts, preds = torch.rand(2, 40, 3, generator=g, dtype=torch.float64), torch.rand(2, 23, 3, generator=g, dtype=torch.float64)
    w = torch.rand(2, generator=g, dtype=torch.float64)
    p, q = preds.clone().requires_grad_(True), gts.clone().requires_grad_(True)
    loss, ip, ig = O.chamfer(p, q, return_indices=True)
    (loss * w).sum().backward()
    dP, dG = O.chamfer_grads_from_indices(w, preds, gts, ip, ig)
    assert _rel(dP.numpy(), p.grad.numpy()) <= 1e-12 and _rel(dG.numpy(), q.grad.numpy()) <= 1e-12


def _models():
    import soft_intro_vae_3d.models.vae as V
    return V


@pytest.mark.parametrize("fixture_key,build", [
    ("keys_model", lambda V, z: V.SoftIntroVAE(O.config(z))),
    ("keys_bootstrap", lambda V, z: V.SoftIntroVAEBootstrap(O.config(z))),
    ("keys_nobn", lambda V, z: V.EncoderNoBatchNorm(O.config(z))),
    ("keys_nobn_nobias", lambda V, z: V.EncoderNoBatchNorm(O.config(z, use_bias_e=False))),
    ("keys_decoder_nobias", lambda V, z: V.Decoder(O.config(z, use_bias_d=False))),
])
def test_dropin_state_dict_keys_and_shapes(fixture_key, build):
    fx = np.load(os.path.join(GOLD, "pc3d_full.npz"))
    z = int(fx["meta_z"])
    want = [(k, tuple(s)) for k, s in json.loads(str(fx[fixture_key]))]
    m = build(_models(), z)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want


def test_recipe_state_dict_loads_strict():
    V = _models()
    for boot, cls in ((False, V.SoftIntroVAE), (True, V.SoftIntroVAEBootstrap)):
        specs = O.model_specs(16, bootstrap=boot)
        sd = O.recipe_state_dict(specs, 3, torch.float32)
        m = cls(O.config(16))
        m.load_state_dict(sd, strict=True)
        assert m.zdim == 16 and m.encoder.conv[0].weight.shape == (64, 3, 1)
        assert torch.equal(m.decoder.model[8].weight, sd["decoder.model.8.weight"])
    specs = O.encoder_specs(16, bn=False)
    V.EncoderNoBatchNorm(O.config(16)).load_state_dict(O.recipe_state_dict(specs, 4, torch.float32), strict=True)


def test_dropin_signatures_match_the_reference():
    """constructor and method parameter lists of soft_intro_vae_3d/models/vae.py and losses/chamfer_loss.py"""
    V = _models()
    from soft_intro_vae_3d.losses.chamfer_loss import ChamferLoss

    def params(f):
        return list(inspect.signature(f).parameters)

    for cls in (V.Encoder, V.EncoderNoBatchNorm, V.Decoder, V.SoftIntroVAE, V.SoftIntroVAEBootstrap):
        assert params(cls.__init__) == ["self", "config"], cls
    assert params(V.Encoder.forward) == ["self", "x"] and params(V.EncoderNoBatchNorm.forward) == ["self", "x"]
    assert params(V.Decoder.forward) == ["self", "input"]
    assert params(V.SoftIntroVAE.forward) == ["self", "x", "deterministic"]
    assert inspect.signature(V.SoftIntroVAE.forward).parameters["deterministic"].default is False
    assert params(V.SoftIntroVAEBootstrap.forward) == ["self", "x", "deterministic", "use_target_decoder"]
    assert inspect.signature(V.SoftIntroVAEBootstrap.forward).parameters["use_target_decoder"].default is True
    assert params(V.SoftIntroVAEBootstrap.sample) == ["self", "z", "use_target_decoder"]
    assert inspect.signature(V.SoftIntroVAEBootstrap.sample).parameters["use_target_decoder"].default is False
    assert params(V.SoftIntroVAE.sample) == ["self", "z"]
    for cls in (V.SoftIntroVAE, V.SoftIntroVAEBootstrap):
        assert params(cls.encode) == ["self", "x"] and params(cls.decode) == ["self", "z"]
        assert params(cls.sample_with_noise) == ["self", "num_samples", "device"]
    assert params(V.SoftIntroVAEBootstrap.decode_target) == ["self", "z"]
    assert params(V.reparameterize)[:2] == ["mu", "logvar"]
    assert params(ChamferLoss.__init__) == ["self"] and params(ChamferLoss.forward) == ["self", "preds", "gts"]
    m = V.SoftIntroVAEBootstrap(O.config(8))
    assert m.zdim == 8 and hasattr(m, "encoder") and hasattr(m, "decoder") and hasattr(m, "target_decoder")


def test_cpu_tensors_are_rejected():
    V = _models()
    from soft_intro_vae_3d.losses.chamfer_loss import ChamferLoss
    from sivae_hip import pointcloud as PC
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ChamferLoss()(torch.zeros(1, 4, 3), torch.zeros(1, 5, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.max_points(torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.SoftIntroVAE(O.config(8)).encode(torch.zeros(2, 3, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.Decoder(O.config(8))(torch.zeros(2, 8))


def test_pointcloud_entry_points_validate_arguments():
    """null pointers, zero sizes, missing / short workspaces: the documented codes"""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    big = 1 << 20
    assert L.sivae_chamfer_workspace_bytes(2, 2048, 2048) == 2 * 16 * 4
    assert L.sivae_chamfer_workspace_bytes(3, 33, 70) == 3 * 2 * 4 and L.sivae_chamfer_workspace_bytes(0, 8, 8) == 0
    f = L.sivae_chamfer_fwd
    assert f(null, one, one, one, one, 2, 8, 8, one, big, null) == -1
    assert f(one, one, one, null, one, 2, 8, 8, one, big, null) == -1
    assert f(one, one, one, one, one, 0, 8, 8, one, big, null) == -2
    assert f(one, one, one, one, one, 2, 0, 8, one, big, null) == -2
    assert f(one, one, one, one, one, 2, 8, 0, one, big, null) == -2
    assert f(one, one, one, one, one, 70000, 8, 8, one, big, null) == -2     # (the batch is a grid dimension)
    assert f(one, one, one, one, one, 2, 1 << 29, 8, one, big, null) == -5
    assert f(one, one, one, one, one, 2, 8, 8, null, 0, null) == -4
    assert f(one, one, one, one, one, 2, 2048, 2048, one, 64, null) == -4
    b = L.sivae_chamfer_bwd
    assert b(null, one, one, one, one, one, one, 2, 8, 8, null) == -1
    assert b(one, one, one, one, null, one, one, 2, 8, 8, null) == -1
    assert b(one, one, one, one, one, null, null, 2, 8, 8, null) == -1       # (one of the two gradients must be asked for)
    assert b(one, one, one, one, one, one, null, 2, 0, 8, null) == -2
    nb = L.sivae_relu_bn_workspace_bytes(32, 256, 2048)
    assert nb > 0 and nb % (256 * 2 * 8) == 0 and L.sivae_relu_bn_workspace_bytes(4, 5, 1) == 5 * 2 * 8
    assert L.sivae_relu_bn_workspace_bytes(0, 5, 1) == 0
    s = L.sivae_relu_bn_stats
    assert s(null, 2, 4, 8, 1e-5, 0.1, null, null, null, one, one, one, big, null) == -1
    assert s(one, 2, 4, 8, 1e-5, 0.1, one, null, null, one, one, one, big, null) == -1   # running mean without running var
    assert s(one, 2, 0, 8, 1e-5, 0.1, null, null, null, one, one, one, big, null) == -2
    assert s(one, 2, 4, 0, 1e-5, 0.1, null, null, null, one, one, one, big, null) == -2
    assert s(one, 2, 4, 8, 1e-5, 0.1, null, null, null, one, one, null, 0, null) == -4
    assert s(one, 32, 256, 2048, 1e-5, 0.1, null, null, null, one, one, one, 16, null) == -4
    assert s(one, 1 << 12, 1 << 12, 1 << 12, 1e-5, 0.1, null, null, null, one, one, one, big, null) == -5
    a = L.sivae_relu_bn_apply
    assert a(one, one, one, one, null, one, 2, 4, 8, null) == -1 and a(one, one, one, one, one, one, 0, 4, 8, null) == -2
    w = L.sivae_relu_bn_bwd
    assert w(one, one, one, one, one, null, one, one, 2, 4, 8, one, big, null) == -1
    assert w(one, one, one, one, one, one, one, one, 2, 4, 0, one, big, null) == -2
    assert w(one, one, one, one, one, one, one, one, 2, 4, 8, null, 0, null) == -4
    m = L.sivae_max_points_fwd
    assert m(one, null, one, 2, 4, 8, null) == -1 and m(one, one, one, 2, 4, 0, null) == -2
    mb = L.sivae_max_points_bwd
    assert mb(one, null, one, 2, 4, 8, null) == -1 and mb(one, one, one, 0, 4, 8, null) == -2


def test_relu_bn_slice_counts():
    """sivae_relu_bn_workspace_bytes(B, C, N) = C * S * 16 tells the number S of slices a channel's B * N values are cut
    into.  The shapes of tests/test_pointcloud_paths_gpu.py::test_relu_bn_sliced must give S > 1 (the S of the issue's
    table), the four shapes of tests/test_pointcloud_gpu.py::test_relu_bn give S = 1: if the slicing policy changes, this
    says that the GPU cases no longer reach the multi-slice reduction"""
    L = lib.load()
    sliced = O.RELU_BN_SLICED
    assert sorted(sliced.values()) == [2, 2, 3, 3, 16]
    single = [(3, 64, 100), (2, 512, 2048), (4, 5, 1), (1, 7, 33)]
    got = {}
    for B, C, N in list(sliced) + single:
        nbytes = L.sivae_relu_bn_workspace_bytes(B, C, N)
        assert nbytes > 0 and nbytes % (C * 16) == 0, (B, C, N, nbytes)
        got[(B, C, N)] = nbytes // (C * 16)
    assert got == {**sliced, **{k: 1 for k in single}}, got
    assert L.sivae_relu_bn_workspace_bytes(32, 512, 2048) == 512 * 4 * 16  # (the training shape of the last stage)
    # the seam case's slice length is 3072: ceil(B N / S) rounded up to 1024
    for B, C, N in [(3, 5, 1368), (3, 7, 2731)]:
        S = sliced[(B, C, N)]
        assert ((B * N + S - 1) // S + 1023) // 1024 * 1024 == 3072


def test_build_imports_the_pointcloud_modules():
    import __graft_entry__ as G
    src = inspect.getsource(G.build)
    assert "sivae_hip.pointcloud" in src or "pointcloud" in src
    from sivae_hip import pointcloud as PC
    for name in ("chamfer_distance", "relu_bn", "max_points", "pointwise_conv"):
        assert callable(getattr(PC, name))
