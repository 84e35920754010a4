"""A plain torch restatement of the style variant's layers (csrc/style.hip, sivae_hip.style, style_soft_intro_vae/blocks.py)
for the CPU: the three ops and the two blocks as functions of tensors and a state dict.  Everything runs in the dtype of
its inputs (float64 for the checks; float32 to measure what the arithmetic itself loses); gradients come from autograd.
Written from the formulas in include/sivae_hip.h, not from the kernels."""
import math

import torch
import torch.nn.functional as F

K_BUMP = 0.8 / math.sqrt(2.0 * math.pi)


def lrelu(p):
    return torch.where(p > 0, p, p * 0.2)


def plane_stats(t):
    m = t.mean(dim=(2, 3), keepdim=True)
    v = ((t - m) ** 2).mean(dim=(2, 3), keepdim=True)
    return m, v


def style_layer(x, noise_weight, bias, style, noise=None, mode=0, layer=0, eps=1e-8):
    """-> y; mode 0: the fixed bump, 1: noise [B, 1, H, W], 2: noise [1, 1, H, W]"""
    B, C = x.shape[:2]
    if mode == 0:
        s = math.sqrt(layer + 1.0)
        u = x + s * K_BUMP * torch.exp(-x * x / (2.0 * s * s))
    else:
        assert noise.shape[0] == (B if mode == 1 else 1)
        u = x + noise_weight.view(1, C, 1, 1) * noise
    t = lrelu(u + bias.view(1, C, 1, 1))
    m, v = plane_stats(t)
    xh = (t - m) / torch.sqrt(v + eps)
    st = style.view(B, 2, C, 1, 1)
    return xh * (st[:, 0] + 1) + st[:, 1]


def stat_norm(x, bias, eps=1e-5):
    """-> (xn, m [B, C], std [B, C])"""
    C = x.shape[1]
    t = lrelu(x + bias.view(1, C, 1, 1))
    m, v = plane_stats(t)
    return (t - m) / torch.sqrt(v + eps), m.flatten(1), torch.sqrt(v).flatten(1)


def blur(x):
    C = x.shape[1]
    f = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype)
    w = (f[:, None] * f[None, :] / 16.0).view(1, 1, 3, 3).repeat(C, 1, 1, 1)
    return F.conv2d(x, w, padding=1, groups=C)


def _shifted_sum(w):
    w = F.pad(w, (1, 1, 1, 1))
    return w[:, :, 1:, 1:] + w[:, :, :-1, 1:] + w[:, :, 1:, :-1] + w[:, :, :-1, :-1]


def _noise_mode(noise):
    return 0 if not noise else (2 if noise == "batch_constant" else 1)


def decode_block(P, x, s1, s2, noise, noises, has_first_conv=True, fused_scale=False, layer=0):
    """P: the block's state dict; noises: the two noise tensors in the order the block draws them (ignored in mode 0)"""
    mode = _noise_mode(noise)
    if has_first_conv:
        if fused_scale:
            x = F.conv_transpose2d(x, _shifted_sum(P["conv_1.weight"]), stride=2, padding=1)
        else:
            x = F.conv2d(x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3), P["conv_1.weight"], padding=1)
        x = blur(x)
    st = F.linear(s1, P["style_1.weight"], P["style_1.bias"])
    x = style_layer(x, P["noise_weight_1"], P["bias_1"], st, noises[0] if mode else None, mode, layer)
    x = F.conv2d(x, P["conv_2.weight"], padding=1)
    st = F.linear(s2, P["style_2.weight"], P["style_2.bias"])
    return style_layer(x, P["noise_weight_2"], P["bias_2"], st, noises[1] if mode else None, mode, layer)


def encode_block(P, x, last=False, fused_scale=False):
    """-> (x, w1, w2)"""
    x, m, std = stat_norm(F.conv2d(x, P["conv_1.weight"], padding=1), P["bias_1"])
    w1 = F.linear(torch.cat((m, std), dim=1), P["style_1.weight"], P["style_1.bias"])
    if last:
        x = lrelu(F.linear(x.flatten(1), P["dense.weight"], P["dense.bias"]))
        return x, w1, F.linear(x, P["style_2.weight"], P["style_2.bias"])
    x = blur(x)
    if fused_scale:
        x = F.conv2d(x, _shifted_sum(P["conv_2.weight"]) * 0.25, stride=2, padding=1)
    else:
        x = F.avg_pool2d(F.conv2d(x, P["conv_2.weight"], padding=1), 2, 2)
    x, m, std = stat_norm(x, P["bias_2"])
    return x, w1, F.linear(torch.cat((m, std), dim=1), P["style_2.weight"], P["style_2.bias"])


# ------------------------------------------------------------------------------------------------ the ops' check cases
# (B, C, H, W): a plane smaller than a wave; odd everything with scalar tails; a plain case; the largest single-read plane;
# a two-read plane; the largest plane; H W = 2; many channels on a tiny plane
CASES = [(1, 1, 4, 4), (3, 5, 5, 7), (2, 3, 8, 8), (2, 2, 64, 64), (1, 2, 128, 128), (1, 1, 256, 256), (2, 3, 2, 1),
         (4, 130, 4, 4)]
# One case per launch configuration (NT, EPT) of csrc/style.hip and per edge inside it, beyond what CASES holds: the top and
# the bottom of <256, 4>; the bottom and the middle of <256, 16> (register slots skipped, a partly filled slot); the bottom,
# the middle and the top minus one of <1024, 16>; the bottom and the middle of <1024, 64>, which the backward streams with
# a partial last stride; the streamed forward with 16-byte chunks and with a scalar tail.  H W % 4 != 0 gives the tail.
# tests/test_style_edges_host.py reads the thresholds from the source and says which row is missing when one moves.
EDGE_CASES = [(2, 3, 16, 16), (1, 2, 1, 257), (2, 3, 32, 32), (1, 2, 25, 41), (1, 2, 37, 61), (1, 1, 17, 241),
              (1, 2, 96, 100), (1, 1, 127, 129), (1, 1, 1, 16385), (1, 1, 160, 200), (1, 1, 257, 256), (1, 1, 255, 259)]
# (mode, layer, noise_weight is zero)
DEC_VARIANTS = [(1, 0, False), (2, 0, False), (0, 0, False), (0, 3, False), (1, 0, True)]


def dec_inputs(case, mode, zero_nw=False, seed=0):
    """float64 inputs of a style_layer check, each value exact in float32: x, noise_weight, bias, style, noise, and the
    upstream gradient g"""
    B, C, H, W = case
    g = torch.Generator().manual_seed(1000 * seed + 17 * B + 31 * C + 7 * H + W + 101 * mode)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    d = dict(x=r(B, C, H, W), noise_weight=0.5 * r(C), bias=0.25 * r(C), style=0.5 * r(B, 2 * C), g=r(B, C, H, W))
    d["noise"] = None if mode == 0 else r(B if mode == 1 else 1, 1, H, W)
    if zero_nw:
        d["noise_weight"] = torch.zeros(C, dtype=torch.float64)
    return d


def enc_inputs(case, seed=0):
    B, C, H, W = case
    g = torch.Generator().manual_seed(2000 * seed + 17 * B + 31 * C + 7 * H + W)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    return dict(x=r(B, C, H, W), bias=0.25 * r(C), g=r(B, C, H, W), gm=r(B, C), gs=r(B, C))


def dec_reference(d, mode, layer, dtype=torch.float64):
    """-> dict(y, dx, dnw (None in mode 0), dbias, dstyle) in `dtype`, the planes' statistics m and r = 1 / sqrt(v + eps)
    [B, C] in float64, and `lead`: the size of the leading term of the instance norm's backward, max |r (style + 1)| max |g|
    (see nerr)"""
    x, nw, b, st = (d[k].to(dtype).clone().requires_grad_(True) for k in ("x", "noise_weight", "bias", "style"))
    nz = None if d["noise"] is None else d["noise"].to(dtype)
    y = style_layer(x, nw, b, st, nz, mode, layer)
    (y * d["g"].to(dtype)).sum().backward()
    with torch.no_grad():
        B, C = x.shape[:2]
        u = x + (nw.view(1, C, 1, 1) * nz if mode else math.sqrt(layer + 1.0) * K_BUMP * torch.exp(-x * x / (2.0 * (layer + 1.0))))
        m, v = plane_stats(lrelu(u + b.view(1, C, 1, 1)))
        lead = float(((st.view(B, 2, C, 1, 1)[:, 0] + 1).abs() / torch.sqrt(v + 1e-8)).max() * d["g"].abs().max())
    return dict(y=y.detach(), dx=x.grad, dnw=None if mode == 0 else nw.grad, dbias=b.grad, dstyle=st.grad, lead=lead,
                m=m.double().flatten(1), r=(1.0 / torch.sqrt(v.double() + 1e-8)).flatten(1))


def enc_reference(d, dtype=torch.float64):
    """-> dict(xn, m, std, dx, dbias)"""
    x, b = (d[k].to(dtype).clone().requires_grad_(True) for k in ("x", "bias"))
    xn, m, std = stat_norm(x, b)
    ((xn * d["g"].to(dtype)).sum() + (m * d["gm"].to(dtype)).sum() + (std * d["gs"].to(dtype)).sum()).backward()
    return dict(xn=xn.detach(), m=m.detach(), std=std.detach(), dx=x.grad, dbias=b.grad)


def nerr(a, ref, lead=0.0):
    """normalised error max |a - ref| / max(max |ref|, lead), inf for a value that is not finite.  `lead` is for the
    decoder layer's gradients with respect to x, bias and noise_weight: dt = r (style + 1) (dy - mean dy - xh mean(dy xh))
    is a difference whose terms have the size lead = max |r (style + 1)| max |dy| and which can cancel altogether (on a
    plane of two elements xh is +-1 whatever t is, and the exact gradient is 0 to the order of eps): any evaluation in
    fp32 then carries an error of 2^-24 lead, which only a measure against the terms' size can judge."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return float((a - ref).abs().max() / max(float(ref.abs().max()), lead, 1e-30))


def viol(a, ref, rtol=1e-4, atol_scale=1e-5):
    """the project's element-wise forward criterion |a - ref| <= rtol |ref| + atol_scale max |ref| (tests/test_e2e_gpu.py)
    -> the worst ratio of error to bound (<= 1 passes), inf for a value that is not finite"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return float(((a - ref).abs() / (rtol * ref.abs() + atol_scale * float(ref.abs().max()) + 1e-300)).max())


LEAD_KEYS = ("dx", "dnw", "dbias")  # (the decoder gradients that come out of dt)

# ------------------------------------------------------------------------------------------------ planted planes
PLANT_STRIDES = (256, 1024, 4096)  # the elements a block of 64, 256 and 1024 threads covers with one 4-element chunk each
PLANT_CASES = EDGE_CASES + [(1, 1, 256, 256)]


def planted(n):
    """{flat index: value} of a plane of n elements: the first and the last element, and for every stride s with 2 s < n
    the first element of a thread's second chunk (s) and of the last, possibly partial, round of chunks (where that round
    is the last element alone, as at n = 1025, it carries this value).  Every value is exact in float32 and large against the unit-variance data around it, so a sum that drops one of these elements is
    wrong by far more than any rounding."""
    at = {0: -32.0, n - 1: 64.0}
    for s in PLANT_STRIDES:
        if 2 * s < n:
            at[s] = 48.0
            at[(n - 1) // s * s] = -24.0
    return at


def plant(d, keys=("x", "g")):
    """a copy of the inputs d with planted() written into every plane of d[k], k in keys"""
    d = dict(d)
    for k in keys:
        t = d[k].clone()
        flat = t.view(t.shape[0], t.shape[1], -1)
        for e, v in planted(flat.shape[2]).items():
            flat[:, :, e] = v
        d[k] = t
    return d



def fp32_loss():
    """worst normalised error of the float32 restatement against the float64 one over CASES and EDGE_CASES:
    (forward, gradients)"""
    fwd = grad = 0.0
    for case in CASES + EDGE_CASES:
        for mode, layer, zero_nw in DEC_VARIANTS:
            d = dec_inputs(case, mode, zero_nw)
            r64, r32 = dec_reference(d, mode, layer), dec_reference(d, mode, layer, torch.float32)
            fwd = max(fwd, nerr(r32["y"], r64["y"]))
            grad = max([grad] + [nerr(r32[k], r64[k], r64["lead"] if k in LEAD_KEYS else 0.0)
                                 for k in ("dx", "dnw", "dbias", "dstyle") if r64[k] is not None])
        d = enc_inputs(case)
        r64, r32 = enc_reference(d), enc_reference(d, torch.float32)
        fwd = max([fwd] + [nerr(r32[k], r64[k]) for k in ("xn", "m", "std")])
        grad = max([grad] + [nerr(r32[k], r64[k]) for k in ("dx", "dbias")])
    return fwd, grad


if __name__ == "__main__":
    print("float32 restatement vs float64 over CASES and EDGE_CASES: forward %.3e, gradients %.3e" % fp32_loss())
