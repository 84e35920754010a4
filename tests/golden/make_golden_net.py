"""Generate the style variant's network fixture from the REAL reference (runs only where the reference checkout is at hand).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net.py /path/to/reference

The reference's style_soft_intro_vae/net.py is imported from its own directory and runs on the CPU in float64 at
startf=4, maxf=8, layer_count=3, latent_size=8, channels=3 (resolutions 4 to 16, no fused_scale layer).  style_net.npz
holds

  names                     JSON: the registry entries {registry: {name: class}} and the signatures of __init__ and forward
  <class>/keys              JSON: the state dict's [key, shape] pairs in order
  <class>/init<seed>        the constructor's state dict for torch.manual_seed(seed), float32 as constructed, the tensors
                            flattened and joined in the order of keys (a file of many small arrays is mostly headers);
                            for the second seed <class>/init<seed>_sha256, the SHA-256 of those bytes
  <class>/coef, <class>/std JSON: the lr_equalization_coef of every parameter and the .std of every module that has one
  <class>/param/<key>       the float64 values the runs used in place of init<SEEDS[0]> for every bias and noise weight
                            (the reference initialises them to 0, which would hide them); every other tensor is init's
  <class>/<run>/meta        JSON: the arguments of the run (lod, blend, noise) or the constructor's (mappings), and
                            grad_keys, the parameters that received a gradient, in order
  <class>/<run>/in/<name>, out<i>, g<i>, grad/<input name>
                            inputs and the weights g of the scalar sum_i sum(out_i g_i) (drawn exact in float32 and
                            stored so), the outputs, and that scalar's gradient for every input.  The three encoders
                            run on the same image, stored once as encoders/<run>/in/x.
  <class>/<run>/grads       that scalar's gradient for the parameters of grad_keys, joined likewise.  Outputs and
                            gradients are stored as float32: 2^-24 of figures that are held to 1e-4 and 1e-5.
  <class>/<run>/rgb/<name>  what went into and came out of the RGB layers for the first sample, in float64 (the oracle's
                            sub-results): x, prev, y for Generator; other, y for Encoder (its image is in/x)

The entries are stored joined (see pack).  Nothing of the reference is copied: the fixture holds inputs, recorded results and names only.
"""
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS = (0, 1)
CFG = dict(startf=4, maxf=8, layer_count=3, latent_size=8, channels=3)
RUNS = [(2, 1), (2, 0.25), (2, 0.75), (1, 0.75), (0, 1)]  # (lod, blend)
ENCODERS = ("Encoder_old", "EncoderWithFC", "Encoder")
MAPPINGS = {"Mapping": dict(num_layers=6), "VAEMappingToLatent_old": {}, "VAEMappingToLatentNoStyle": {},
            "VAEMappingFromLatent": dict(num_layers=6)}
B = 2


def run_name(lod, blend):
    return "lod%d_blend%s" % (lod, str(blend).replace(".", "p"))


def pack(out):
    """the entries joined into one array per kind (a zip member costs about 150 bytes of headers, and there are hundreds):
    `f32`, `f64`, and `index`, JSON {key: [kind, offset, shape]} with the text entries as {key: ["text", string]};
    tests/style_net_fixture.py reads it back"""
    blobs, index = {"f32": [], "f64": []}, {}
    fill = {"f32": 0, "f64": 0}
    for k, v in out.items():
        v = np.asarray(v)
        if v.dtype.kind == "U":
            index[k] = ["text", str(v)]
            continue
        kind = {"float32": "f32", "float64": "f64"}[str(v.dtype)]
        index[k] = [kind, fill[kind], list(v.shape)]
        blobs[kind].append(v.ravel())
        fill[kind] += v.size
    return dict(f32=np.concatenate(blobs["f32"]), f64=np.concatenate(blobs["f64"]),
                index=np.frombuffer(json.dumps(index).encode(), dtype=np.uint8))


def exact32(*shape, generator):
    """float64 values that are exact in float32"""
    return torch.randn(*shape, generator=generator, dtype=torch.float64).float().double()


def record_class(out, name, make):
    for seed in SEEDS:
        torch.manual_seed(seed)
        m = make()
        sd = m.state_dict()
        flat = np.concatenate([v.numpy().ravel() for v in sd.values()])
        if seed == SEEDS[0]:
            out["%s/init%d" % (name, seed)] = flat
        else:  # (bit-for-bit equality needs no more than a digest)
            out["%s/init%d_sha256" % (name, seed)] = np.array(hashlib.sha256(flat.tobytes()).hexdigest())
    out["%s/keys" % name] = np.array(json.dumps([[k, list(v.shape)] for k, v in sd.items()]))
    out["%s/coef" % name] = np.array(json.dumps({k: float(p.lr_equalization_coef) for k, p in m.named_parameters()
                                                 if hasattr(p, "lr_equalization_coef")}))
    out["%s/std" % name] = np.array(json.dumps({k: float(mod.std) for k, mod in m.named_modules()
                                                if isinstance(getattr(mod, "std", None), (float, np.floating))}))


def seeded_model(out, name, make, g):
    torch.manual_seed(SEEDS[0])
    m = make().double()
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "bias" in k or "noise_weight" in k:
                p.copy_(0.4 * torch.randn(*p.shape, generator=g, dtype=torch.float64))
                out["%s/param/%s" % (name, k)] = p.detach().numpy().copy()
    return m


def record_run(out, pre, m, ins, call, g, meta, store_inputs=True):
    for p in m.parameters():
        p.grad = None
    outs = call()
    outs = outs if isinstance(outs, tuple) else (outs,)
    gs = [exact32(*o.shape, generator=g) for o in outs]
    sum((o * w).sum() for o, w in zip(outs, gs)).backward()
    for i, (o, w) in enumerate(zip(outs, gs)):
        out["%s/out%d" % (pre, i)], out["%s/g%d" % (pre, i)] = o.detach().numpy().astype(np.float32), w.numpy().astype(np.float32)
    for k, v in ins.items():
        if store_inputs:
            out["%s/in/%s" % (pre, k)] = v.detach().numpy().astype(np.float32)
        out["%s/grad/%s" % (pre, k)] = v.grad.numpy().astype(np.float32)
    have = [(k, p.grad) for k, p in m.named_parameters() if p.grad is not None]
    out["%s/grads" % pre] = np.concatenate([v.numpy().ravel() for _, v in have]).astype(np.float32)
    out["%s/meta" % pre] = np.array(json.dumps(dict(meta, grad_keys=[k for k, _ in have])))


def main(ref):
    sys.path.insert(0, os.path.join(ref, "style_soft_intro_vae"))
    import net  # noqa: E402  (the reference's)

    out = {}
    classes = ENCODERS + ("Generator", "FromRGB", "ToRGB", "MappingBlock") + tuple(MAPPINGS)
    names = dict(registries={r: {k: v.__name__ for k, v in getattr(net, r).items() if not k.startswith("DCGAN")}
                             for r in ("ENCODERS", "GENERATORS", "MAPPINGS")},
                 signatures={c: dict(init=str(inspect.signature(getattr(net, c).__init__)),
                                     forward=str(inspect.signature(getattr(net, c).forward))) for c in classes})
    out["names"] = np.array(json.dumps(names))
    torch.set_default_dtype(torch.float64)  # (the reference's own torch.zeros / torch.randn calls)
    try:
        for ci, name in enumerate(ENCODERS + ("Generator",)):
            make = lambda: getattr(net, name)(**CFG)  # noqa: E731
            torch.set_default_dtype(torch.float32)
            record_class(out, name, make)
            g = torch.Generator().manual_seed(4321 + (name == "Generator"))
            m = seeded_model(out, name, make, g)
            torch.set_default_dtype(torch.float64)
            L, n = CFG["layer_count"], CFG["latent_size"]
            for lod, blend in RUNS:
                pre = "%s/%s" % (name, run_name(lod, blend))
                seen, hooks = {}, []
                if name == "Generator":
                    # (noise=False, the layers' fixed bump: the reference draws its noise on the default device itself)
                    ins = {"styles": exact32(B, 2 * L, n, generator=g).requires_grad_(True)}
                    hooks.append(m.to_rgb[lod].register_forward_hook(lambda mod, i, o: seen.update(x=i[0])))
                    if blend != 1:
                        hooks.append(m.to_rgb[lod - 1].register_forward_hook(lambda mod, i, o: seen.update(prev=o)))
                    call = lambda: m(ins["styles"], lod, blend, False)  # noqa: E731
                    meta = dict(lod=lod, blend=blend, noise=False)
                else:
                    res = 4 * 2 ** lod
                    gx = torch.Generator().manual_seed(97 + 10 * lod + int(8 * blend))  # (the same image for the three)
                    ins = {"x": exact32(B, CFG["channels"], res, res, generator=gx).requires_grad_(True)}
                    out["encoders/%s/in/x" % run_name(lod, blend)] = ins["x"].detach().numpy().astype(np.float32)
                    first = L - lod - 1
                    if blend == 1:
                        hooks.append(m.encode_block[first].register_forward_pre_hook(lambda mod, i: seen.update(y=i[0])))
                    else:
                        hooks.append(m.encode_block[first].register_forward_hook(lambda mod, i, o: seen.update(other=o[0])))
                        hooks.append(m.encode_block[first + 1].register_forward_pre_hook(lambda mod, i: seen.update(y=i[0])))
                    call = lambda: m(ins["x"], lod, blend)  # noqa: E731
                    meta = dict(lod=lod, blend=blend)
                record_run(out, pre, m, ins, call, g, meta, store_inputs=name == "Generator")
                seen["y"] = seen.get("y", torch.from_numpy(out[pre + "/out0"])) if name != "Generator" else call()
                for h in hooks:
                    h.remove()
                for k, v in seen.items() if name in ("Generator", "Encoder") else ():
                    out["%s/rgb/%s" % (pre, k)] = v.detach().numpy()[:1].copy()  # (the first sample)
        for ci, (name, extra) in enumerate(MAPPINGS.items()):
            for layers in (3, 5):
                cname = "%s%d" % (name, layers)
                kw = dict(extra, mapping_layers=layers, latent_size=8, dlatent_size=8, mapping_fmaps=12)
                make = lambda: getattr(net, name)(**kw)  # noqa: E731
                torch.set_default_dtype(torch.float32)
                record_class(out, cname, make)
                g = torch.Generator().manual_seed(8765 + 10 * ci + layers)
                m = seeded_model(out, cname, make, g)
                torch.set_default_dtype(torch.float64)
                shape = (B, 1, 8) if "ToLatent" in name else (B, 8)
                ins = {"x": exact32(*shape, generator=g).requires_grad_(True)}
                record_run(out, cname + "/run", m, ins, lambda: m(ins["x"]), g, dict(cls=name, kwargs=kw))
    finally:
        torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "style_net.npz")
    np.savez_compressed(path, **pack(out))
    print("wrote %s: %d entries, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
