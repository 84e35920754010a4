"""Generate the fixture of the style variant's fused_scale blocks from the REAL reference (runs only where the reference
checkout is at hand).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_style_scale.py /path/to/reference

The reference's style_soft_intro_vae/net.py is imported from its own directory and runs on the CPU in float64, as for
make_golden_style.py, whose layout style_scale_blocks.npz keeps (per covered block `<case>`: init<seed>/, coef/, param/,
in/, noise<i>, out<i>, g<i>, grad/, meta).  The two blocks are the ones with a stride-2 convolution over the transformed
kernel (fused_scale=True: the transposed form in the DecodeBlock, the strided form in the EncodeBlock), at shapes the
phase-form kernels take, with unequal channel counts and sides so that a missing transpose or a flip of one axis shows.
Every drawn input, weight g and replaced parameter is exact in float32, so the float32 run starts from the same numbers.

Nothing of the reference is copied: the fixture holds inputs, recorded results and names only.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0, 1)
NOISE_SEED = 78

# case -> (block, constructor arguments, x shape, the `noise` argument)
CASES = {
    "dec_fused_up": ("DecodeBlock", dict(inputs=8, outputs=6, latent_size=16, has_first_conv=True, fused_scale=True, layer=1),
                     (2, 8, 8, 16), True),
    "enc_fused_down": ("EncodeBlock", dict(inputs=6, outputs=8, latent_size=16, last=False, fused_scale=True),
                       (2, 6, 16, 32), None),
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
        g = torch.Generator().manual_seed(4321 + len(case))
        rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
        with torch.no_grad():
            for k, p in m.named_parameters():
                if k.startswith(("noise_weight_", "bias_")):
                    p.copy_((0.4 * rnd(*p.shape)).float().double())
        for k, v in m.state_dict().items():
            out["%s/param/%s" % (case, k)] = v.numpy().copy()
        ins = {"x": rnd(*xshape).requires_grad_(True)}
        torch.set_default_dtype(torch.float64)  # (the block's own torch.randn calls)
        try:
            if block == "DecodeBlock":
                ins["s1"], ins["s2"] = rnd(xshape[0], 16).requires_grad_(True), rnd(xshape[0], 16).requires_grad_(True)
                torch.manual_seed(NOISE_SEED)
                outs = (m(ins["x"], ins["s1"], ins["s2"], noise),)
                torch.manual_seed(NOISE_SEED)
                shape = [xshape[0], 1, outs[0].shape[2], outs[0].shape[3]]
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
    path = os.path.join(HERE, "style_scale_blocks.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
