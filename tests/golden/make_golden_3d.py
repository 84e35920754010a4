"""Generate the 3-D point-cloud fixtures from the REAL reference (runs only where the reference checkout is mounted).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_3d.py [/path/to/reference]

The reference's soft_intro_vae_3d/models/vae.py and losses/chamfer_loss.py are imported BY FILE PATH under private module
names (its `models` package must not be confused with this project's drop-in of the same name), calc_kl comes from its
train_soft_intro_vae_3d.py (plotting / dataset imports stubbed).  Everything runs in float64 on the CPU.

  pc3d_<case>.npz   one vanilla-VAE objective (train_soft_intro_vae_3d.py:225-231) through the reference's SoftIntroVAE:
                    inputs (x, eps), mu, logvar, the decoder output, per-cloud Chamfer values, KL, the loss, the
                    BatchNorm buffers after the pass, every parameter-gradient norm and the first values of every
                    gradient, and the list of state_dict keys and shapes (also of SoftIntroVAEBootstrap and
                    EncoderNoBatchNorm)
  pc3d_chamfer.npz  ChamferLoss on two seeded clouds of unequal size

Weights are NOT stored (the decoder alone is 27 MB): they are rebuilt on both sides by tests/pc3d_oracle.py's
`recipe_state_dict` from numpy's PCG64.  Nothing of the reference is copied: fixtures are inputs / outputs only.
"""
import importlib.machinery
import importlib.util
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pc3d_oracle as O  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
REF3D = os.path.join(REF, "soft_intro_vae_3d")


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _ref_modules():
    vae = _by_path("_ref3d_vae", os.path.join(REF3D, "models", "vae.py"))
    ch = _by_path("_ref3d_chamfer", os.path.join(REF3D, "losses", "chamfer_loss.py"))
    # the training script: only calc_kl is used; everything it imports besides torch / numpy is stubbed
    stubs = ["matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "tqdm", "utils", "utils.pcutil",
             "utils.util", "metrics", "metrics.jsd", "datasets", "datasets.transforms3d", "models", "models.vae"]
    saved = {k: sys.modules.get(k) for k in stubs}
    for name in stubs:
        m = mock.MagicMock(name=name)
        m.__spec__ = importlib.machinery.ModuleSpec(name, None)
        m.__path__ = []
        sys.modules[name] = m
    try:
        tr = _by_path("_ref3d_train", os.path.join(REF3D, "train_soft_intro_vae_3d.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return vae, ch, tr


def _keys(model):
    return json.dumps([[k, list(v.shape)] for k, v in model.state_dict().items()])


def _np(t):
    return t.detach().cpu().numpy().copy()


def make_case(vae, ch, tr, name, z, B, N, seed):
    torch.set_default_dtype(torch.float64)
    try:
        cfg = O.config(z)
        model = vae.SoftIntroVAE(cfg).double().train()
        sd = O.recipe_state_dict(O.model_specs(z), seed)
        assert [k for k in model.state_dict()] == list(sd), "recipe order differs from the reference's state_dict"
        model.load_state_dict(sd, strict=True)
        g = np.random.Generator(np.random.PCG64(1000 + seed))
        x = torch.from_numpy(g.random(size=(B, 3, N)) - 0.5)
        eps = torch.from_numpy(g.standard_normal(size=(B, z)))
        mu, logvar = model.encode(x)
        rec = model.decode(mu + eps * torch.exp(0.5 * logvar))
        chv = ch.ChamferLoss()(x.permute(0, 2, 1) + 0.5, rec.permute(0, 2, 1) + 0.5)
        klv = tr.calc_kl(logvar, mu, logvar_o=float(np.log(0.2 ** 2)), reduce="mean")
        loss = 20.0 * chv.mean() + 1.0 * klv
        loss.backward()
        out = dict(meta_z=z, meta_B=B, meta_N=N, meta_seed=seed, meta_beta_rec=20.0, meta_beta_kl=1.0, x=_np(x), eps=_np(eps),
                   mu=_np(mu), logvar=_np(logvar), rec=_np(rec), chamfer=_np(chv), kl=_np(klv), loss=_np(loss),
                   keys_model=_keys(model), keys_bootstrap=_keys(vae.SoftIntroVAEBootstrap(cfg)),
                   keys_nobn=_keys(vae.EncoderNoBatchNorm(cfg)),
                   keys_nobn_nobias=_keys(vae.EncoderNoBatchNorm(O.config(z, use_bias_e=False))),
                   keys_decoder_nobias=_keys(vae.Decoder(O.config(z, use_bias_d=False))))
        for k, p in model.named_parameters():
            out["gnorm/" + k] = np.float64(p.grad.norm().item())
            out["gslice/" + k] = _np(p.grad.reshape(-1)[:8])
        for k, v in model.state_dict().items():
            if "running_" in k or "num_batches" in k:
                out["buf/" + k] = _np(v)
        # eval mode (running statistics) on the same input, after the training pass updated the buffers
        model.eval()
        with torch.no_grad():
            mu_e, lv_e = model.encode(x)
        out["mu_eval"], out["logvar_eval"] = _np(mu_e), _np(lv_e)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
        print(name, "loss %.12g" % float(loss.detach()), os.path.getsize(os.path.join(HERE, name + ".npz")), "bytes")
    finally:
        torch.set_default_dtype(torch.float32)


def make_chamfer(ch):
    g = np.random.Generator(np.random.PCG64(77))
    preds = torch.from_numpy(g.random(size=(3, 33, 3)))
    gts = torch.from_numpy(g.random(size=(3, 70, 3)))
    v = ch.ChamferLoss()(preds, gts)
    np.savez_compressed(os.path.join(HERE, "pc3d_chamfer.npz"), preds=_np(preds), gts=_np(gts), chamfer=_np(v))
    print("pc3d_chamfer", _np(v))


if __name__ == "__main__":
    with mock.patch("torch.cuda.is_available", return_value=False):  # (ChamferLoss picks its index type by it)
        vae, ch, tr = _ref_modules()
        make_case(vae, ch, tr, "pc3d_small", z=16, B=3, N=100, seed=1)
        make_case(vae, ch, tr, "pc3d_full", z=128, B=2, N=2048, seed=2)
        make_chamfer(ch)
