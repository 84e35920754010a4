"""A plain torch restatement of the style variant's RGB layers (csrc/rgb.hip, sivae_hip.style.to_rgb / from_rgb) for the
CPU, written from the formulas in include/sivae_hip.h, not from the kernels.  Everything runs in the dtype of its inputs
(float64 for the checks; float32 to measure what the arithmetic itself loses); gradients come from autograd.

    python style_rgb_oracle.py     prints the float32 restatement's loss against the float64 one over CASES and
                                   EDGE_CASES
"""
import torch
import torch.nn.functional as F

from style_oracle import nerr, viol  # noqa: F401  (the project's two error measures, re-exported)


def lrelu2(t):
    t = torch.where(t > 0, t, t * 0.2)
    return torch.where(t > 0, t, t * 0.2)


def lerp(a, b, w):
    """torch's scalar-weight formula"""
    return a + w * (b - a) if abs(w) < 0.5 else b - (b - a) * (1 - w)


def up2(p):
    return p.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def avg2(x):
    return ((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])) / 4


def to_rgb(x, w, bias, prev=None, blend=1.0):
    """x [B, C, H, W], w [K, C], bias [K], prev [B, K, H/2, W/2] -> y [B, K, H, W]"""
    conv = torch.einsum("kc,bchw->bkhw", w, x) + bias.view(1, -1, 1, 1)
    return conv if prev is None else lerp(up2(prev), conv, blend)


def pre_activation(img, w, bias, pool=False):
    u = avg2(img) if pool else img
    return torch.einsum("ck,bkhw->bchw", w, u) + bias.view(1, -1, 1, 1)


def from_rgb(img, w, bias, pool=False, other=None, blend=1.0):
    """img [B, K, H, W], w [C, K], bias [C], other [B, C, Ho, Wo] -> y [B, C, Ho, Wo]"""
    a = lrelu2(pre_activation(img, w, bias, pool))
    return a if other is None else lerp(a, other, blend)


# ------------------------------------------------------------------------------------------------ the check cases
# (B, C, H, W, K); H x W is the resolution of x (to_rgb) and of the image (from_rgb)
CASES = [(1, 1, 4, 4, 1),        # a plane smaller than a wave; K = 1
         (3, 5, 5, 7, 3),        # odd everything and scalar tails; plain forms only
         (3, 5, 6, 10, 3),       # a row that is no multiple of 4 elements, with blend and pool
         (2, 3, 2, 2, 3),        # prev and the pooled image are 1 x 1
         (2, 16, 8, 8, 3),       # a plain middling case
         (4, 130, 4, 4, 3),      # more channels than a wave's slice of them, on a tiny plane
         (2, 3, 64, 64, 3),      # a 64 x 64 plane
         (1, 2, 128, 128, 4),    # K = 4
         (1, 1, 256, 256, 3)]    # the largest plane: 65536-term dw and dbias sums
# What CASES leaves out of csrc/rgb.hip's launch logic: K = 2; C = 9 (cpw = 2: a wave with one channel, waves that start
# past C); K = 4 with an odd C > 8; planes of several 256-pixel tiles with a partial last one, plain and pooled; more than
# 256 blocks, so that a thread of the merge kernel adds more than one partial.  tests/test_style_edges_host.py keeps it so.
EDGE_CASES = [(2, 5, 6, 10, 2),       # K = 2, plain, blended and pooled
              (1, 9, 8, 8, 2),        # K = 2; C = 9
              (1, 2, 36, 44, 2),      # K = 2 on several tiles
              (2, 11, 6, 10, 4),      # K = 4 (8 values a channel in the partials) with an odd C > 8
              (2, 9, 6, 10, 3),       # C = 9 with K = 3: two channels per wave sum, an odd slice
              (2, 3, 20, 20, 3),      # H W = 400: two tiles, the second partial, 16-byte chunks
              (2, 3, 17, 19, 3),      # H W = 323: the same with scalar accesses (plain only)
              (2, 3, 4, 5, 3),        # H W % 4 = 0 with an odd W: 16-byte chunks across row ends
              (1, 3, 36, 44, 3),      # H W = 1584: 7 tiles, the last partial; pooled 18 x 22 = 396: two tiles, rows of 22
              (300, 5, 4, 4, 3),      # 300 blocks: the merge kernel's second round, 4 values a channel, both layers
              (259, 2, 4, 4, 4)]      # 259 blocks with 8 values a channel
BLENDS = (0.25, 0.75)            # the two branches of torch's lerp
KINK_MARGIN = 2.0 ** -18
MAX_SEEDS = 64


def variants(case):
    """None (plain) and, where H and W are even, the two blends"""
    return (None,) + (BLENDS if case[2] % 2 == 0 and case[3] % 2 == 0 else ())


def case_id(case):
    return "x".join(map(str, case))


def _rand(case, salt, seed):
    B, C, H, W, K = case
    g = torch.Generator().manual_seed(salt + 1000 * seed + 17 * B + 31 * C + 7 * H + W + 101 * K)
    return lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # (exact in float32)


def to_inputs(case, blend=None, seed=0):
    """float64 inputs of a to_rgb check, each value exact in float32: x, w, bias, prev (None when plain), and g, the
    upstream gradient"""
    B, C, H, W, K = case
    r = _rand(case, 3000, seed)
    d = dict(x=r(B, C, H, W), w=0.5 * r(K, C), bias=0.25 * r(K), g=r(B, K, H, W), blend=blend)
    d["prev"] = None if blend is None else r(B, K, H // 2, W // 2)
    return d


def kink_margin(d):
    """min over the pre-activations of |t| / (|bias| + sum_k |w| |u|), in float64"""
    pool = d["blend"] is not None
    t = pre_activation(d["img"], d["w"], d["bias"], pool)
    s = pre_activation(d["img"].abs(), d["w"].abs(), d["bias"].abs(), pool)
    return float((t.abs() / s).min())


def from_inputs(case, blend=None, seed=0):
    """float64 inputs of a from_rgb check: img, w, bias, other (None when plain; then the image is pooled too), g.  The
    seed moves on until every pre-activation keeps KINK_MARGIN times the sum of its terms' magnitudes away from 0: a float32
    t carries at most a few 2^-24 of that sum, so no correct kernel can see another sign and the activation's kink stays out
    of the gradient check."""
    B, C, H, W, K = case
    for s in range(seed, seed + MAX_SEEDS):
        r = _rand(case, 4000 + (500 if blend is not None else 0), s)
        Ho, Wo = (H // 2, W // 2) if blend is not None else (H, W)
        d = dict(img=r(B, K, H, W), w=0.5 * r(C, K), bias=0.25 * r(C), g=r(B, C, Ho, Wo), blend=blend, seed=s)
        d["other"] = None if blend is None else r(B, C, Ho, Wo)
        if kink_margin(d) >= KINK_MARGIN:
            return d
    raise RuntimeError("no seed keeps the pre-activations of %s away from the kink" % (case,))


def _leaf(t, dtype):
    return None if t is None else t.to(dtype).clone().requires_grad_(True)


def to_reference(d, dtype=torch.float64):
    """-> dict(y, dx, dw, dbias, dprev (None when plain)) in `dtype`"""
    x, w, b, p = (_leaf(d[k], dtype) for k in ("x", "w", "bias", "prev"))
    y = to_rgb(x, w, b, p, 1.0 if d["blend"] is None else d["blend"])
    (y * d["g"].to(dtype)).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, dbias=b.grad, dprev=None if p is None else p.grad)


def from_reference(d, dtype=torch.float64):
    """-> dict(y, dimg, dw, dbias, dother (None when plain)) in `dtype`"""
    img, w, b, o = (_leaf(d[k], dtype) for k in ("img", "w", "bias", "other"))
    y = from_rgb(img, w, b, d["blend"] is not None, o, 1.0 if d["blend"] is None else d["blend"])
    (y * d["g"].to(dtype)).sum().backward()
    return dict(y=y.detach(), dimg=img.grad, dw=w.grad, dbias=b.grad, dother=None if o is None else o.grad)


TO_GRADS, FROM_GRADS = ("dx", "dw", "dbias", "dprev"), ("dimg", "dw", "dbias", "dother")


def fp32_loss():
    """worst normalised error of the float32 restatement against the float64 one over CASES and EDGE_CASES:
    (forward, gradients)"""
    fwd = grad = 0.0
    for case in CASES + EDGE_CASES:
        for blend in variants(case):
            for d, ref, keys in ((to_inputs(case, blend), to_reference, TO_GRADS),
                                 (from_inputs(case, blend), from_reference, FROM_GRADS)):
                r64, r32 = ref(d), ref(d, torch.float32)
                fwd = max(fwd, nerr(r32["y"], r64["y"]))
                grad = max([grad] + [nerr(r32[k], r64[k]) for k in keys if r64[k] is not None])
    return fwd, grad


if __name__ == "__main__":
    print("float32 restatement vs float64 over CASES and EDGE_CASES: forward %.3e, gradients %.3e" % fp32_loss())
