"""Generate the style variant's model fixture from the REAL reference (runs only where the reference checkout is at hand).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_style_model.py /path/to/reference

The reference's style_soft_intro_vae/model.py (with its own net.py) is imported from its own directory and runs on the
CPU in float64 at make_golden_net.py's CFG (startf=4, maxf=8, layer_count=3, latent_size=8, B = 2) with mapping_layers=3,
scale = 1 / (3 16^2) and betas at which the exp-ELBO terms carry signal.  torch.randn and torch.randn_like are wrapped
for the length of a run: every draw is rounded through float32 and recorded in call order; Python's `random` is seeded
per run and model.random is wrapped to record the mixing decisions.  (torch.lerp is wrapped too, to take the float32
truncation coefficients of model.py:198 next to float64 tensors.)  style_model.npz holds

  names                 JSON: the signatures of the helpers and of SoftIntroVAEModelTL.__init__ / generate / encode /
                        forward / lerp
  model/kwargs          JSON: the constructor arguments of the forward runs; model/gen_kwargs those of the generate runs
  model/keys            JSON: the state dict's [key, shape] pairs in order
  model/init<seed>      the constructor's state dict for torch.manual_seed(seed), float32, joined in the order of keys;
                        for the second seed its SHA-256
  model/param/<key>     the float64 values the runs used in place of init<SEEDS[0]> for every bias and noise weight
  <run>/meta            JSON: kind (forward / generate), branch, lod, blend, seed, the shapes of the draws in call order,
                        mixing (one [taken, cutoff or null] per random.random() call), grad_keys (the parameters that
                        received a gradient, in order), zero_grad_keys (those among them whose gradient is zero to float64 rounding),
                        requires_grad (the keys whose flag is set afterwards), and the scalars loss and last_* (float64)
  <run>/x, <run>/draws  the image batch (forward runs) and the draws joined in call order (exact in float32)
  <run>/buff_in, /buff  dlatent_avg.buff before and after the call
  <run>/grads, /grad_x  the gradients of the loss (forward) or of sum(out g) (generate: <run>/out, <run>/g) for the
                        parameters of grad_keys, joined, and for x, as float32

The entries are stored joined (make_golden_net.pack).  The generator asserts what a test could otherwise pass without:
every recorded expelbo_rec / expelbo_fake lies in [1e-3, 0.999]; the mixing branch is recorded both taken and not
taken, with a cutoff below the number of layers; no parameter but the first decoder layer's bias may have a gradient that is zero to float64 rounding (with noise=True, as
recorded here, that one is not zero either: zero_grad_keys is empty in every run).
Nothing of the reference is copied: the fixture holds inputs, recorded results and names only.
"""
import hashlib
import inspect
import json
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_net import B, CFG, SEEDS, exact32, pack  # noqa: E402

KW = dict(CFG, mapping_layers=3, generator="GeneratorDefault", encoder="EncoderDefault", scale=1.0 / (3 * 16 ** 2),
          beta_kl=0.5, beta_rec=0.75, beta_neg=16.0, gamma_r=1e-8, dlatent_avg_beta=0.995, style_mixing_prob=0.9)
GEN_KW = dict(KW, truncation_psi=0.7, truncation_cutoff=4)
FORWARD_RUNS = [(2, 1), (2, 0.75), (1, 1)]  # (lod, blend)
BRANCHES = ("vae", "e_train", "d_train")
LAST = ("last_rec_loss", "last_real_kl", "last_fake_kl", "last_kl_diff", "last_expelbo_fake", "last_expelbo_rec")
LAST_IN = dict(last_fake_kl=0.75, last_real_kl=0.25)  # what last_kl_diff of the d_train branch is formed from
NOT_MIXED_SEED = 119  # random.seed(119), (217), (228): the first random.random() is above the mixing probability 0.9
GENERATE_SEEDS = (200, 201, 217, 228)
ZERO_REL = 1e-12
HELPERS = ("set_model_require_grad", "reparameterize", "calc_kl", "calc_reconstruction_loss")
METHODS = ("__init__", "generate", "encode", "forward", "lerp")


def run_name(kind, branch, lod, blend, seed):
    return "%s/%s/lod%d_blend%s_seed%d" % (kind, branch, lod, str(blend).replace(".", "p"), seed)


class Recorder:
    """wraps torch.randn / randn_like / lerp and the model module's `random` for the length of a run"""

    def __init__(self, model_module):
        self.mod, self.draws, self.mixing = model_module, [], []

    def __enter__(self):
        self.saved = (torch.randn, torch.randn_like, torch.lerp, self.mod.random)
        randn, randn_like, lerp = self.saved[:3]

        def keep(t):
            t32 = t.float()
            self.draws.append(t32.numpy().copy())
            return t32.to(t.dtype)
        torch.randn = lambda *a, **k: keep(randn(*a, **k))
        torch.randn_like = lambda *a, **k: keep(randn_like(*a, **k))
        torch.lerp = lambda a, b, w: lerp(a, b, w.to(a.dtype) if isinstance(w, torch.Tensor) else w)
        rec = self

        class Random:
            @staticmethod
            def random():
                v = random.random()
                rec.mixing.append([None, None, v])
                return v

            @staticmethod
            def randint(a, b):
                v = random.randint(a, b)
                rec.mixing[-1][1] = v
                return v
        self.mod.random = Random
        return self

    def __exit__(self, *exc):
        torch.randn, torch.randn_like, torch.lerp, self.mod.random = self.saved

    def decisions(self, prob):
        return [[v < prob, cut] for _, cut, v in self.mixing]


def seeded(model_module, kw, g, out=None):
    torch.manual_seed(SEEDS[0])
    torch.set_default_dtype(torch.float32)
    m = model_module.SoftIntroVAEModelTL(**kw).double()
    torch.set_default_dtype(torch.float64)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "bias" in k or "noise_weight" in k:
                p.copy_(0.4 * torch.randn(*p.shape, generator=g, dtype=torch.float64))
                if out is not None:
                    out["model/param/%s" % k] = p.detach().numpy().copy()
    return m


def finish(out, pre, m, rec, meta, x=None):
    have = [(k, p.grad) for k, p in m.named_parameters() if p.grad is not None]
    out[pre + "/grads"] = np.concatenate([v.numpy().ravel() for _, v in have]).astype(np.float32)
    if x is not None:
        out[pre + "/x"] = x.detach().numpy().astype(np.float32)
        out[pre + "/grad_x"] = x.grad.numpy().astype(np.float32)
    out[pre + "/draws"] = np.concatenate([d.ravel() for d in rec.draws])
    out[pre + "/buff"] = m.dlatent_avg.buff.detach().numpy().copy()
    # (in float64 a gradient that cancels comes out as a few 1e-17 of the others, not as 0.0: "zero" is below ZERO_REL of
    # the largest parameter gradient of the run)
    top = max(float(v.abs().max()) for _, v in have)
    meta.update(draw_shapes=[list(d.shape) for d in rec.draws], mixing=rec.decisions(m.style_mixing_prob),
                grad_keys=[k for k, _ in have], zero_grad_keys=[k for k, v in have if float(v.abs().max()) <= ZERO_REL * top],
                requires_grad=[k for k, p in m.named_parameters() if p.requires_grad])
    out[pre + "/meta"] = np.array(json.dumps(meta))
    return meta


def main(ref):
    sys.path.insert(0, os.path.join(ref, "style_soft_intro_vae"))
    import model as M  # noqa: E402  (the reference's, with its own net.py)

    out = {}
    sig = lambda f: str(inspect.signature(f))  # noqa: E731
    out["names"] = np.array(json.dumps(dict(helpers={h: sig(getattr(M, h)) for h in HELPERS},
                                            methods={k: sig(getattr(M.SoftIntroVAEModelTL, k)) for k in METHODS},
                                            dlatent=sig(M.DLatent.__init__))))
    out["model/kwargs"], out["model/gen_kwargs"] = np.array(json.dumps(KW)), np.array(json.dumps(GEN_KW))
    for seed in SEEDS:
        torch.manual_seed(seed)
        sd = M.SoftIntroVAEModelTL(**KW).state_dict()
        flat = np.concatenate([v.numpy().ravel() for v in sd.values()])
        if seed == SEEDS[0]:
            out["model/init%d" % seed] = flat
        else:
            out["model/init%d_sha256" % seed] = np.array(hashlib.sha256(flat.tobytes()).hexdigest())
    out["model/keys"] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))

    torch.set_default_dtype(torch.float64)
    try:
        g = torch.Generator().manual_seed(2468)
        m = seeded(M, KW, g, out)
        mg = seeded(M, GEN_KW, torch.Generator().manual_seed(2468))
        buff_in = 0.5 * exact32(*m.dlatent_avg.buff.shape, generator=g)
        out["model/buff_in"] = buff_in.numpy().copy()
        metas, L = [], 2 * CFG["layer_count"]
        for ri, (lod, blend) in enumerate(FORWARD_RUNS):
            res = 4 * 2 ** lod
            for bi, branch in enumerate(BRANCHES):
                seed = NOT_MIXED_SEED if (ri, branch) == (1, "e_train") else 100 + 10 * ri + bi
                pre = run_name("forward", branch, lod, blend, seed)
                for p in m.parameters():
                    p.grad = None
                with torch.no_grad():
                    m.dlatent_avg.buff.copy_(buff_in)
                for k in LAST:
                    setattr(m, k, torch.tensor(LAST_IN.get(k, 0.0)))
                x = exact32(B, CFG["channels"], res, res, generator=g).requires_grad_(True)
                random.seed(seed)
                torch.manual_seed(seed)
                with Recorder(M) as rec:
                    loss = m(x, lod, blend, branch == "d_train", branch == "e_train")
                    loss.backward()
                meta = dict(kind="forward", branch=branch, lod=lod, blend=blend, seed=seed, loss=float(loss.detach()),
                            **{k: float(getattr(m, k)) for k in LAST})
                metas.append(finish(out, pre, m, rec, meta, x))
                if branch == "e_train":
                    for k in ("last_expelbo_fake", "last_expelbo_rec"):
                        assert 1e-3 <= meta[k] <= 0.999, (pre, k, meta[k])
        for seed in GENERATE_SEEDS:
            lod, blend = 1, 1
            pre = run_name("generate", "mixing", lod, blend, seed)
            for p in mg.parameters():
                p.grad = None
            with torch.no_grad():
                mg.dlatent_avg.buff.copy_(buff_in)
            random.seed(seed)
            torch.manual_seed(seed)
            with Recorder(M) as rec:
                img = mg.generate(lod, blend, count=B, mixing=True, noise=True)
            w = exact32(*img.shape, generator=g)
            (img * w).sum().backward()
            out[pre + "/out"], out[pre + "/g"] = img.detach().numpy().astype(np.float32), w.numpy().astype(np.float32)
            metas.append(finish(out, pre, mg, rec, dict(kind="generate", lod=lod, blend=blend, seed=seed)))
        taken = [d for meta in metas for d in meta["mixing"]]
        assert any(t and c < L for t, c in taken) and any(not t for t, _ in taken), taken
        first_bias = "decoder.decode_block.0.bias_1"
        for meta in metas:
            assert set(meta["zero_grad_keys"]) <= {first_bias}, meta["zero_grad_keys"]
    finally:
        torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "style_model.npz")
    np.savez_compressed(path, **pack(out))
    print("wrote %s: %d entries, %d bytes" % (path, len(out), os.path.getsize(path)))
    for meta in metas:
        print(meta["kind"], meta.get("branch", ""), meta["lod"], meta["blend"], "mixing", meta["mixing"],
              {k: round(v, 5) for k, v in meta.items() if k.startswith("last_") or k == "loss"},
              "zero", meta["zero_grad_keys"], "n_grad", len(meta["grad_keys"]), "draws", len(meta["draw_shapes"]))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
