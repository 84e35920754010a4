"""Generate the style variant's block fixture from the REAL reference (runs only where the reference checkout is at hand).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_style.py /path/to/reference

The reference's style_soft_intro_vae/net.py is imported from its own directory (it needs its lreq, registry and utils
next to it) and runs on the CPU in float64.  style_blocks.npz holds, per covered block `<case>`:

  <case>/init<seed>/<key>   the constructor's state dict for torch.manual_seed(seed), float32 as constructed
  <case>/coef/<key>         the lr_equalization_coef attribute of every parameter that carries one
  <case>/param/<key>        the float64 state the block ran with: init<SEEDS[0]> with every noise_weight_* and bias_*
                            replaced by seeded non-zero values (the reference initialises them to 0, which would hide them)
  <case>/in/<name>          the inputs (x; s1, s2 for a DecodeBlock)
  <case>/noise<i>           the noise tensors the block drew, re-drawn from the same seed in the same order
  <case>/out<i>, <case>/g<i>   the outputs and the recorded weights g of the scalar sum_i sum(out_i g_i)
  <case>/grad/<name or key> the gradient of that scalar for every input and every parameter that received one
  <case>/meta               JSON: block, constructor arguments, the noise argument, the seed of the noise

Nothing of the reference is copied: the fixture holds inputs, recorded results and names only.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0, 1)
NOISE_SEED = 77

# case -> (block, constructor arguments, x shape, the `noise` argument)
CASES = {
    "dec_per_sample": ("DecodeBlock", dict(inputs=8, outputs=6, latent_size=16, has_first_conv=True, fused_scale=False, layer=1),
                       (2, 8, 5, 7), True),
    "dec_batch_constant": ("DecodeBlock", dict(inputs=8, outputs=6, latent_size=16, has_first_conv=True, fused_scale=False,
                                               layer=1), (2, 8, 5, 7), "batch_constant"),
    "dec_no_noise": ("DecodeBlock", dict(inputs=8, outputs=6, latent_size=16, has_first_conv=True, fused_scale=False, layer=1),
                     (2, 8, 5, 7), False),
    "dec_no_first_conv": ("DecodeBlock", dict(inputs=6, outputs=6, latent_size=16, has_first_conv=False, fused_scale=False,
                                              layer=0), (2, 6, 4, 4), True),
    "enc": ("EncodeBlock", dict(inputs=6, outputs=8, latent_size=16, last=False, fused_scale=False), (2, 6, 8, 8), None),
    "enc_last": ("EncodeBlock", dict(inputs=6, outputs=8, latent_size=16, last=True, fused_scale=False), (2, 6, 4, 4), None),
}


def main(ref):
    sys.path.insert(0, os.path.join(ref, "style_soft_intro_vae"))
    import net  # noqa: E402  (the reference's)

    out = {}
    for case, (block, kw, xshape, noise) in CASES.items():
        cls = getattr(net, block)
        for seed in SEEDS:
            torch.manual_seed(seed)
            m = cls(**kw)
            for k, v in m.state_dict().items():
                out["%s/init%d/%s" % (case, seed, k)] = v.numpy().copy()
            if seed == SEEDS[0]:
                for k, p in m.named_parameters():
                    if hasattr(p, "lr_equalization_coef"):
                        out["%s/coef/%s" % (case, k)] = np.float64(p.lr_equalization_coef)
        torch.manual_seed(SEEDS[0])
        m = cls(**kw).double()
        g = torch.Generator().manual_seed(1234 + len(case))
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
        with torch.no_grad():
            for k, p in m.named_parameters():
                if k.startswith(("noise_weight_", "bias_")):
                    p.copy_(0.4 * rnd(*p.shape))
        for k, v in m.state_dict().items():
            out["%s/param/%s" % (case, k)] = v.numpy().copy()
        ins = {"x": rnd(*xshape).requires_grad_(True)}
        torch.set_default_dtype(torch.float64)  # (the block's own torch.randn calls)
        try:
            if block == "DecodeBlock":
                ins["s1"], ins["s2"] = rnd(xshape[0], 16).requires_grad_(True), rnd(xshape[0], 16).requires_grad_(True)
                torch.manual_seed(NOISE_SEED)
                outs = (m(ins["x"], ins["s1"], ins["s2"], noise),)
                if noise:
                    torch.manual_seed(NOISE_SEED)
                    shape = [1 if noise == "batch_constant" else xshape[0], 1, outs[0].shape[2], outs[0].shape[3]]
                    for i in range(2):
                        out["%s/noise%d" % (case, i)] = torch.randn(shape).numpy().copy()
            else:
                outs = m(ins["x"])
        finally:
            torch.set_default_dtype(torch.float32)
        gs = [rnd(*o.shape) for o in outs]
        sum((o * w).sum() for o, w in zip(outs, gs)).backward()
        for i, (o, w) in enumerate(zip(outs, gs)):
            out["%s/out%d" % (case, i)], out["%s/g%d" % (case, i)] = o.detach().numpy().copy(), w.numpy().copy()
        for k, v in ins.items():
            out["%s/in/%s" % (case, k)], out["%s/grad/%s" % (case, k)] = v.detach().numpy().copy(), v.grad.numpy().copy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out["%s/grad/%s" % (case, k)] = p.grad.numpy().copy()
        out["%s/meta" % case] = np.array(json.dumps(dict(block=block, kwargs=kw, noise=noise, noise_seed=NOISE_SEED)))
    path = os.path.join(HERE, "style_blocks.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
