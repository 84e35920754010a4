"""GPU checks of the blur folded into the style chains: style.style_layer(..., blur=True) and style.stat_norm(...,
blur=True) (csrc/style.hip's *_blur_* kernels through sivae_hip.ops.style_*(..., blur=True)) and blocks.FUSE_BLUR.

The yardstick is the composition the fused forms replace, style.blur around the plain chain, which tests/test_style_gpu.py
holds to the reference: every output and gradient of a fused form is torch.equal to the composition's.  Beside it the same
outputs stand against the float64 oracle (O.blur composed with O.style_layer / O.stat_norm) under the criteria and gates of
tests/test_style_gpu.py, unchanged: O.viol <= 1 forward, O.nerr <= S.GRAD_GATE with the decoder's `lead` for the gradients.

Shapes: O.CASES + O.EDGE_CASES (every (NT, EPT) configuration, scalar tails, skipped and partly filled slots, the streamed
forms), BLUR_EDGES (single rows and columns, chunks that straddle a row end on the 16-byte and on the scalar path) and one
plane at, just below and just above the LDS bound of the decoder backward, each with a W that is no multiple of 4.  The bound
is asked of the library (ops.style_dec_blur_bwd_fused); tests/test_style_blur_fused_host.py holds it against the source.

The border test reads the stencil back exactly.  Mode 0 adds the layer's bump, which no plane of ones survives exactly, so
the decoder's read goes through mode 1 with a zero noise weight, zero bias and zero style: u = blur(x) + 0 noise = blur(x),
t = blur(x) > 0, and y = fma((t - m) r, 1, 0) is, with the m and r the kernel returns, one float32 subtraction and one
multiplication, which torch repeats bit for bit; m itself is the exact (H - 1/2)(W - 1/2) / (H W).  The encoder backward's
read goes through a constant plane (t - m = 0 exactly): dx = r (blur(g) - mean blur(g)) with every sum exact."""
import functools
import math
import sys

import numpy as np
import pytest
import torch

import style_oracle as O
import test_style_gpu as S

pytestmark = pytest.mark.gpu

DEV = S.DEV
put = S.put
CID = lambda c: "x".join(map(str, c))  # noqa: E731
MODES = (0, 1, 2)
DEC_KEYS = ("y", "m", "r", "dx", "dnw", "dbias", "dstyle")
ENC_KEYS = ("xn", "m", "std", "dx", "dbias")

# the blur's own edges: H in {1, 2} and W in {1, 2, 3}; H W % 4 == 0 with W % 4 != 0 (a 16-byte chunk over a row end);
# the same on the scalar path
BLUR_EDGES = [(1, 1, 1, 2), (2, 3, 2, 1), (1, 2, 9, 1), (1, 2, 1, 9), (1, 2, 7, 2), (2, 2, 5, 3), (1, 2, 6, 6), (1, 2, 10, 26),
              (3, 5, 5, 7)]


def lds_bound():
    """the largest H W the decoder backward finishes in one launch, found by bisection of the library's query"""
    from sivae_hip import ops
    lo, hi = 1, 1 << 30  # fused at lo, not at hi
    assert ops.style_dec_blur_bwd_fused(1, lo) and not ops.style_dec_blur_bwd_fused(1, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ops.style_dec_blur_bwd_fused(1, mid) else (lo, mid)
    return lo


def bound_cases(bound):
    """{'at' | 'below' | 'above': (1, 1, H, W)} with H W = bound, bound - 1, bound + 1 and W the largest divisor of H W up to
    its square root that is no multiple of 4"""
    def plane(n):
        w = max(d for d in range(1, math.isqrt(n) + 1) if n % d == 0 and d % 4)
        return (1, 1, n // w, w)
    return {"at": plane(bound), "below": plane(bound - 1), "above": plane(bound + 1)}


LDS_BOUND = lds_bound()
BOUND = bound_cases(LDS_BOUND)
ALL_CASES = list(dict.fromkeys(O.CASES + O.EDGE_CASES + BLUR_EDGES + list(BOUND.values())))


# ------------------------------------------------------------------------------------------------ runners
def run_dec(d, mode, layer=0, fused=True, wants=(True, True, True, True), place=put):
    """forward and backward through the ops: the fused entry points, or the blur kernel around the plain ones"""
    from sivae_hip import ops
    x, nz, nw, b, st, g = (place(d[k]) for k in ("x", "noise", "noise_weight", "bias", "style", "g"))
    if fused:
        y, m, r = ops.style_dec_fwd(x, nz, nw, b, st, mode, layer, blur=True)
        dx, dnw, db, ds = ops.style_dec_bwd(g, x, nz, nw, b, st, m, r, mode, layer, *wants, blur=True)
    else:
        bx = ops.style_blur(x)
        y, m, r = ops.style_dec_fwd(bx, nz, nw, b, st, mode, layer)
        dx, dnw, db, ds = ops.style_dec_bwd(g, bx, nz, nw, b, st, m, r, mode, layer, *wants)
        dx = None if dx is None else ops.style_blur(dx)
    return dict(y=y, m=m, r=r, dx=dx, dnw=dnw, dbias=db, dstyle=ds)


def run_enc(d, fused=True, wants=(True, True), ups=(True, True, True), place=put):
    """ups: which of the three upstream gradients are given (None for the others)"""
    from sivae_hip import ops
    x, b = place(d["x"]), place(d["bias"])
    g, gm, gs = (place(d[k]) if u else None for k, u in zip(("g", "gm", "gs"), ups))
    if fused:
        xn, m, std = ops.style_enc_fwd(x, b, blur=True)
        dx, db = ops.style_enc_bwd(g, gm, gs, x, b, m, std, 1e-5, *wants, blur=True)
    else:
        xn, m, std = ops.style_enc_fwd(x, b)
        dx, db = ops.style_enc_bwd(None if g is None else ops.style_blur(g), gm, gs, x, b, m, std, 1e-5, *wants)
        xn = ops.style_blur(xn)
    return dict(xn=xn, m=m, std=std, dx=dx, dbias=db)


def auto_dec(d, mode, layer, fused):
    """through sivae_hip.style and one torch backward -> y and the four gradients"""
    from sivae_hip import style
    C = d["x"].shape[1]
    x, nw, b, st = (put(t).requires_grad_(True) for t in (d["x"], d["noise_weight"].view(1, C, 1, 1), d["bias"].view(1, C, 1, 1),
                                                          d["style"]))
    nz = put(d["noise"])
    y = style.style_layer(x, nw, b, st, nz, mode, layer, blur=True) if fused else \
        style.style_layer(style.blur(x), nw, b, st, nz, mode, layer)
    y.backward(put(d["g"]))
    return dict(y=y.detach(), dx=x.grad, dnw=nw.grad, dbias=b.grad, dstyle=st.grad)


def auto_enc(d, fused):
    from sivae_hip import style
    C = d["x"].shape[1]
    x, b = put(d["x"]).requires_grad_(True), put(d["bias"].view(1, C, 1, 1)).requires_grad_(True)
    if fused:
        xn, m, std = style.stat_norm(x, b, blur=True)
    else:
        xn, m, std = style.stat_norm(x, b)
        xn = style.blur(xn)
    torch.autograd.backward((xn, m, std), (put(d["g"]), put(d["gm"]), put(d["gs"])))
    return dict(xn=xn.detach(), m=m.detach(), std=std.detach(), dx=x.grad, dbias=b.grad)


def same(got, want, keys, what):
    for k in keys:
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), (what, k)


# ------------------------------------------------------------------------------------------------ the float64 references
def dec_reference(d, mode, layer):
    """O.blur composed with O.style_layer in float64 -> y, the gradients, and m, r, lead of the layer on blur(x)"""
    x, nw, b, st = (d[k].clone().requires_grad_(True) for k in ("x", "noise_weight", "bias", "style"))
    y = O.style_layer(O.blur(x), nw, b, st, d["noise"], mode, layer)
    (y * d["g"]).sum().backward()
    inner = O.dec_reference(dict(d, x=O.blur(d["x"])), mode, layer)  # (the statistics and the size of the leading term)
    return dict(y=y.detach(), dx=x.grad, dnw=None if mode == 0 else nw.grad, dbias=b.grad, dstyle=st.grad, m=inner["m"],
                r=inner["r"], lead=inner["lead"])


def enc_reference(d):
    x, b = (d[k].clone().requires_grad_(True) for k in ("x", "bias"))
    xn, m, std = O.stat_norm(x, b)
    bxn = O.blur(xn)
    ((bxn * d["g"]).sum() + (m * d["gm"]).sum() + (std * d["gs"]).sum()).backward()
    return dict(xn=bxn.detach(), m=m.detach(), std=std.detach(), dx=x.grad, dbias=b.grad)


@functools.lru_cache(maxsize=None)
def dec_case(case, mode, planted=False):
    d = O.dec_inputs(case, mode)
    d = O.plant(d) if planted else d
    return d, dec_reference(d, mode, 0)


@functools.lru_cache(maxsize=None)
def enc_case(case, planted=False):
    d = O.enc_inputs(case)
    d = O.plant(d) if planted else d
    return d, enc_reference(d)


def hold_dec(got, ref, what):
    vs = {k: O.viol(got[k], ref[k]) for k in ("y", "m", "r")}
    errs = {k: O.nerr(got[k], ref[k], ref["lead"] if k in O.LEAD_KEYS else 0.0)
            for k in ("dx", "dnw", "dbias", "dstyle") if ref[k] is not None}
    print("%s: %s of the criterion; %s (gate %.1e)" % (what, ", ".join("%s %.3f" % kv for kv in vs.items()),
                                                       ", ".join("%s %.2e" % kv for kv in errs.items()), S.GRAD_GATE))
    for k, v in vs.items():
        assert got[k].shape == ref[k].shape and v <= 1.0, (k, v)
    for k, e in errs.items():
        assert e <= S.GRAD_GATE, (k, e)


def hold_enc(got, ref, what):
    vs = {k: O.viol(got[k], ref[k]) for k in ("xn", "m", "std")}
    errs = {k: O.nerr(got[k], ref[k]) for k in ("dx", "dbias")}
    print("%s: %s of the criterion; %s (gate %.1e)" % (what, ", ".join("%s %.3f" % kv for kv in vs.items()),
                                                       ", ".join("%s %.2e" % kv for kv in errs.items()), S.GRAD_GATE))
    for k, v in vs.items():
        assert got[k].shape == ref[k].shape and v <= 1.0, (k, v)
    for k, e in errs.items():
        assert e <= S.GRAD_GATE, (k, e)


# ------------------------------------------------------------------------------------------------ 1. the composition's bits
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ALL_CASES, ids=CID)
def test_style_layer_is_the_composition_bit_for_bit(case, mode):
    d = O.dec_inputs(case, mode)
    for layer in (0, 3) if mode == 0 else (0,):
        fused, comp = auto_dec(d, mode, layer, True), auto_dec(d, mode, layer, False)
        assert (fused["dnw"] is None) == (mode == 0)
        same(fused, comp, ("y", "dx", "dnw", "dbias", "dstyle"), (case, mode, layer))
        same(run_dec(d, mode, layer), run_dec(d, mode, layer, fused=False), DEC_KEYS, (case, mode, layer, "ops"))


@pytest.mark.parametrize("case", ALL_CASES, ids=CID)
def test_stat_norm_is_the_composition_bit_for_bit(case):
    d = O.enc_inputs(case)
    same(auto_enc(d, True), auto_enc(d, False), ENC_KEYS, case)
    for bits in range(8):  # every subset of the three upstream gradients, None for the others
        ups = tuple(bool(bits >> i & 1) for i in range(3))
        same(run_enc(d, ups=ups), run_enc(d, fused=False, ups=ups), ENC_KEYS, (case, ups))


@pytest.mark.parametrize("case", [(2, 3, 8, 8), (1, 2, 6, 6), (1, 2, 5, 7)], ids=CID)
def test_stat_norm_on_a_constant_plane(case):
    """std == 0: the dropped dstd term is the plain kernel's, every gradient finite and the composition's"""
    d = O.enc_inputs(case)
    d = dict(d, x=torch.full_like(d["x"], 0.5), bias=torch.zeros_like(d["bias"]))
    fused, comp = run_enc(d), run_enc(d, fused=False)
    assert torch.equal(fused["std"], torch.zeros_like(fused["std"])) and torch.equal(fused["xn"], torch.zeros_like(fused["xn"]))
    assert all(bool(torch.isfinite(fused[k]).all()) for k in ENC_KEYS)
    same(fused, comp, ENC_KEYS, case)
    same(auto_enc(d, True), auto_enc(d, False), ENC_KEYS, (case, "autograd"))


# ------------------------------------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ALL_CASES, ids=CID)
def test_style_layer_against_the_oracle(case, mode):
    d, ref = dec_case(case, mode)
    hold_dec(run_dec(d, mode), ref, "blur > style_layer %s mode %d" % (case, mode))


@pytest.mark.parametrize("case", ALL_CASES, ids=CID)
def test_stat_norm_against_the_oracle(case):
    d, ref = enc_case(case)
    hold_enc(run_enc(d), ref, "stat_norm > blur %s" % (case,))


# ------------------------------------------------------------------------------------------------ 3. borders
def blurred_ones(H, W):
    """blur of a plane of ones, exact: (3/4 | 1) x (3/4 | 1), a side of one element 1/2"""
    side = lambda n: torch.tensor([0.5] if n == 1 else [0.75] + [1.0] * (n - 2) + [0.75])  # noqa: E731
    return side(H)[:, None] * side(W)[None, :]


BORDER_PLANES = [(1, 2), (2, 1), (9, 1), (1, 9), (7, 2), (5, 3), (6, 6), (10, 26), (5, 7), (37, 61)] + \
    [c[2:] for c in BOUND.values()]


@pytest.mark.parametrize("plane", BORDER_PLANES, ids=CID)
def test_a_plane_of_ones_through_the_decoders_input_side(plane):
    """corners 9/16, edges 12/16, interior 1, read back exactly (module docstring)"""
    from sivae_hip import ops
    H, W = plane
    B, C = 2, 2
    x = torch.ones(B, C, H, W, device=DEV)
    zc, zs = torch.zeros(C, device=DEV), torch.zeros(B, 2 * C, device=DEV)
    nz = torch.randn(B, 1, H, W, generator=torch.Generator().manual_seed(H + W)).to(DEV)
    y, m, r = ops.style_dec_fwd(x, nz, zc, zc, zs, 1, 0, blur=True)
    bx = blurred_ones(H, W).to(DEV)
    if H > 2 and W > 2:
        assert sorted(set(bx.flatten().tolist())) == [9 / 16, 12 / 16, 1.0]
        assert bx[0, 0] == bx[-1, -1] == bx[0, -1] == bx[-1, 0] == 9 / 16 and bx[0, 1] == bx[1, 0] == 12 / 16 and bx[1, 1] == 1
    want_m = torch.tensor(bx.double().sum().item() / (H * W)).float()  # (the sum is exact; one rounding to float32)
    assert torch.equal(m, want_m.to(DEV).expand(B, C))
    assert torch.equal(y, (bx[None, None] - m[:, :, None, None]) * r[:, :, None, None])
    if H > 2 or W > 2:  # (the plane of ones does not blur to a constant: the borders show)
        assert float(y.abs().max()) > 0


@pytest.mark.parametrize("plane", BORDER_PLANES, ids=CID)
def test_a_gradient_of_ones_through_the_encoder_backwards_read(plane):
    from sivae_hip import ops
    H, W = plane
    B, C = 2, 2
    x = torch.full((B, C, H, W), 0.5, device=DEV)
    zc = torch.zeros(C, device=DEV)
    _, m, std = ops.style_enc_fwd(x, zc, blur=True)
    assert torch.equal(std, torch.zeros_like(std))
    dx, _ = ops.style_enc_bwd(torch.ones_like(x), None, None, x, zc, m, std, blur=True)
    bg = blurred_ones(H, W)
    k1 = torch.tensor(bg.double().sum().item() / (H * W)).float()
    r = torch.tensor(1.0 / math.sqrt(float(np.float32(1e-5)))).float()
    want = (r * (bg - k1)).to(DEV)  # (t - m = 0 exactly: what is left of dt is r (blur(g) - mean blur(g)), the slope 1)
    assert torch.equal(dx, want[None, None].expand(B, C, H, W))


PLANT_CASES = [c for c in BLUR_EDGES if c[2] * c[3] > 2] + list(BOUND.values()) + [(1, 2, 25, 41), (1, 1, 255, 259)]


@pytest.mark.parametrize("case", PLANT_CASES, ids=CID)
def test_planted_planes_against_the_oracle(case):
    """O.planted values at the first and last elements (and at the chunk and round starts) of x and of the upstream
    gradient: a tap or a sum that loses one of them is wrong by far more than any rounding"""
    d, ref = dec_case(case, 1, True)
    hold_dec(run_dec(d, 1), ref, "planted blur > style_layer %s" % (case,))
    e, ref = enc_case(case, True)
    hold_enc(run_enc(e), ref, "planted stat_norm > blur %s" % (case,))


# ------------------------------------------------------------------------------------------------ 4. isolation
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [(3, 5, 5, 7), (2, 3, 8, 8), (2, 2, 64, 64), (2, 2, 5, 3), (2, 3, 2, 1), (2, 3, 32, 32)], ids=CID)
def test_a_sample_and_a_channel_alone(case, mode):
    d, e = O.dec_inputs(case, mode), O.enc_inputs(case)
    C = case[1]
    whole, ewhole = run_dec(d, mode), run_enc(e)
    shared = ("noise_weight", "bias") + (("noise",) if mode == 2 else ())
    alone = run_dec({k: (v if k in shared or v is None else v[1:2]) for k, v in d.items()}, mode)
    for k in ("y", "m", "r", "dx", "dstyle"):
        assert torch.equal(whole[k][1:2], alone[k]), ("sample 1 alone", k)
    ealone = run_enc({k: (v if k == "bias" else v[1:2]) for k, v in e.items()})
    for k in ("xn", "m", "std", "dx"):
        assert torch.equal(ewhole[k][1:2], ealone[k]), ("sample 1 alone", k)
    c = C - 1  # the last channel alone: its planes, its parameters, its two style columns
    pick = dict(x=d["x"][:, c:c + 1], g=d["g"][:, c:c + 1], noise=d["noise"], noise_weight=d["noise_weight"][c:c + 1],
                bias=d["bias"][c:c + 1], style=d["style"][:, [c, C + c]])
    one = run_dec({k: (None if v is None else v.contiguous()) for k, v in pick.items()}, mode)
    for k in ("y", "m", "r", "dx"):
        assert torch.equal(whole[k][:, c:c + 1], one[k]), ("channel alone", k)
    assert torch.equal(whole["dstyle"][:, [c, C + c]], one["dstyle"]) and torch.equal(whole["dbias"][c:c + 1], one["dbias"])
    assert mode == 0 or torch.equal(whole["dnw"][c:c + 1], one["dnw"])
    eone = run_enc(dict(x=e["x"][:, c:c + 1].contiguous(), g=e["g"][:, c:c + 1].contiguous(), bias=e["bias"][c:c + 1],
                        gm=e["gm"][:, c:c + 1].contiguous(), gs=e["gs"][:, c:c + 1].contiguous()))
    for k in ("xn", "m", "std", "dx"):
        assert torch.equal(ewhole[k][:, c:c + 1], eone[k]), ("channel alone", k)
    assert torch.equal(ewhole["dbias"][c:c + 1], eone["dbias"])


@pytest.mark.parametrize("poison", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("plane", [(2, 1), (1, 9), (5, 7), (6, 6), (10, 26), (37, 61)] + [c[2:] for c in BOUND.values()], ids=CID)
def test_the_neighbour_planes_are_never_read(plane, poison):
    """the plane in the middle of three, the planes before and after it in memory all NaN or 1e30 (x, the upstream gradients
    and, per sample, nothing else): bit-equal to the same plane among zeros.  A tap that leaves the plane by a row or an
    element reads the poison"""
    H, W = plane
    d, e = O.dec_inputs((1, 3, H, W), 1), O.enc_inputs((1, 3, H, W))

    def among(t, v):
        t = t.clone()
        t[:, 0], t[:, 2] = v, v
        return t

    got = {v: (run_dec(dict(d, x=among(d["x"], v), g=among(d["g"], v)), 1),
               run_enc(dict(e, x=among(e["x"], v), g=among(e["g"], v)))) for v in (0.0, poison)}
    for k in ("y", "m", "r", "dx"):
        assert torch.equal(got[poison][0][k][:, 1], got[0.0][0][k][:, 1]), k
    for k in ("dnw", "dbias"):
        assert torch.equal(got[poison][0][k][1], got[0.0][0][k][1]), k
    assert torch.equal(got[poison][0]["dstyle"][:, [1, 4]], got[0.0][0]["dstyle"][:, [1, 4]])
    for k in ("xn", "m", "std", "dx"):
        assert torch.equal(got[poison][1][k][:, 1], got[0.0][1][k][:, 1]), k
    assert torch.equal(got[poison][1]["dbias"][1], got[0.0][1]["dbias"][1])


# ------------------------------------------------------------------------------------------------ 5., 6. alignment, two runs
def shifted(t):
    """t on the device one element behind a 512-byte aligned base"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# H W % 4 == 0: the aligned run is the 16-byte instantiation, the shifted one the scalar instantiation
ALIGN_CASES = [(1, 2, 6, 6), (1, 2, 10, 26), (2, 3, 8, 8), (2, 2, 64, 64), (1, 2, 96, 100), BOUND["at"], (1, 1, 257, 256)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", ALIGN_CASES, ids=CID)
def test_alignment_and_run_change_no_bit(case, mode):
    assert case[2] * case[3] % 4 == 0
    d, e = O.dec_inputs(case, mode), O.enc_inputs(case)
    moved = lambda planes: (lambda t: None if t is None else (shifted(put(t)) if any(t is p for p in planes) else put(t)))  # noqa: E731
    base, ebase = run_dec(d, mode), run_enc(e)
    same(run_dec(d, mode), base, DEC_KEYS, "two runs")
    same(run_enc(e), ebase, ENC_KEYS, "two runs")
    same(run_dec(d, mode, place=moved([d["x"], d["noise"], d["g"]])), base, DEC_KEYS, "alignment")
    same(run_dec(d, mode, place=moved([d["x"]])), base, DEC_KEYS, "alignment of x alone")
    same(run_enc(e, place=moved([e["x"], e["g"]])), ebase, ENC_KEYS, "alignment")
    same(run_enc(e, place=moved([e["g"]])), ebase, ENC_KEYS, "alignment of the gradient alone")


# ------------------------------------------------------------------------------------------------ 7. wanted gradients
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("case", [(3, 5, 5, 7), BOUND["below"], BOUND["above"]], ids=CID)
def test_each_subset_of_wanted_gradients(case, mode):
    d, e = O.dec_inputs(case, mode), O.enc_inputs(case)
    full = run_dec(d, mode)
    keys = ("dx", "dnw", "dbias", "dstyle")
    for bits in range(16):
        wants = tuple(bool(bits >> i & 1) for i in range(4))
        got = run_dec(d, mode, wants=wants)
        for k, w in zip(keys, wants):
            if w and not (k == "dnw" and mode == 0):
                assert torch.equal(got[k], full[k]), (wants, k)
            else:
                assert got[k] is None, (wants, k)
    full = run_enc(e)
    for wants in ((True, False), (False, True), (False, False)):
        got = run_enc(e, wants=wants)
        for k, w in zip(("dx", "dbias"), wants):
            assert (torch.equal(got[k], full[k]) if w else got[k] is None), (wants, k)


# ------------------------------------------------------------------------------------------------ 8. guarded
@pytest.mark.parametrize("case", [(1, 1, 1, 2), (3, 5, 5, 7), BOUND["below"], BOUND["at"], BOUND["above"]], ids=CID)
def test_guarded(case):
    """both ops, forward and backward, on guarded, poisoned outputs and exact workspaces, the inputs at an aligned base and
    one element behind it: nothing written outside a tensor, no element left at the poison value, the unguarded results"""
    from sivae_hip import ops
    from support.guard import describe, guarded
    d, d0, e = O.dec_inputs(case, 1), O.dec_inputs(case, 0), O.enc_inputs(case)
    base_d, base_0, base_e = run_dec(d, 1), run_dec(d0, 0, 1), run_enc(e)
    for off in (0, 1):
        with guarded(ops) as g:
            pl = lambda t: None if t is None else g.place(put(t), offset_elems=off)  # noqa: E731
            got_d, got_0, got_e = run_dec(d, 1, place=pl), run_dec(d0, 0, 1, place=pl), run_enc(e, place=pl)
            damage = g.verify()
            assert not damage, "guard damage:\n%s" % describe(damage)
        for got, base, keys in ((got_d, base_d, DEC_KEYS), (got_0, base_0, DEC_KEYS), (got_e, base_e, ENC_KEYS)):
            for k in keys:
                if base[k] is None:
                    assert got[k] is None
                else:
                    assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], base[k]), (case, off, k)


# ------------------------------------------------------------------------------------------------ 9. the blocks
@pytest.fixture(scope="module")
def blocks():
    sys.path.insert(0, S.BLOCKS_DIR)
    try:
        import blocks as B
    finally:
        sys.path.remove(S.BLOCKS_DIR)
    return B


def block_run(blocks, monkeypatch, kind, args, shape, fuse, noise=True):
    """one forward and backward of a block with FUSE_BLUR = fuse -> (outputs, {name: gradient}, ops.style_blur calls in the
    forward, in the backward, the style calls in order, did a torch convolution run)"""
    from sivae_hip import ops, style
    torch.manual_seed(0)
    m = getattr(blocks, kind)(*args)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # (the biases and noise weights start at zero: give them values)
        for k, p in m.named_parameters():
            if k.startswith(("bias_", "noise_weight_")):
                p.copy_(0.25 * torch.randn(p.shape, generator=g))
    m = m.to(DEV)
    x = put(torch.randn(*shape, generator=g)).requires_grad_(True)
    L = args[2]
    ins = dict(x=x)
    if kind == "DecodeBlock":
        ins.update(s1=put(torch.randn(shape[0], L, generator=g)).requires_grad_(True),
                   s2=put(torch.randn(shape[0], L, generator=g)).requires_grad_(True))
    calls, blurs, torch_conv = [], [], []

    def spy(name, f, log):
        def call(*a, **kw):
            log.append((name, bool(kw.get("blur", False))) if log is calls else name)
            return f(*a, **kw)
        return call

    monkeypatch.setattr(blocks, "FUSE_BLUR", fuse)
    monkeypatch.setattr(ops, "style_blur", spy("style_blur", ops.style_blur, blurs))
    monkeypatch.setattr(style, "style_layer", spy("style_layer", style.style_layer, calls))
    monkeypatch.setattr(style, "stat_norm", spy("stat_norm", style.stat_norm, calls))
    monkeypatch.setattr(style, "blur", spy("blur", style.blur, calls))
    for name in ("conv2d", "conv_transpose2d"):
        monkeypatch.setattr(torch.nn.functional, name, spy(name, getattr(torch.nn.functional, name), torch_conv))
    torch.manual_seed(5)  # (the noise the block draws: the same for both settings)
    outs = m(ins["x"], ins["s1"], ins["s2"], noise) if kind == "DecodeBlock" else m(ins["x"])
    outs = outs if isinstance(outs, tuple) else (outs,)
    fwd_blurs = len(blurs)
    go = [put(torch.randn(o.shape, generator=g)) for o in outs]
    torch.autograd.backward(outs, go)
    torch.cuda.synchronize()
    monkeypatch.undo()
    grads = {k: v.grad for k, v in list(ins.items()) + list(m.named_parameters())}
    return [o.detach() for o in outs], grads, fwd_blurs, len(blurs) - fwd_blurs, calls, bool(torch_conv)


# kind, constructor arguments, input shape; the fused_scale rows at the smallest shape tests/test_style_scale_conv_gpu.py uses
BLOCK_CASES = [("DecodeBlock", (8, 6, 16, True, False, 1), (2, 8, 4, 4)), ("EncodeBlock", (6, 8, 16, False, False), (2, 6, 8, 8)),
               ("DecodeBlock", (8, 6, 16, True, True, 1), (2, 8, 8, 16)), ("EncodeBlock", (6, 8, 16, False, True), (2, 6, 16, 32))]


# (the three noise modes for the decoder; the encoder takes no noise)
BLOCK_RUNS = [(row, noise) for row in BLOCK_CASES
              for noise in ((True, "batch_constant", False) if row[0] == "DecodeBlock" else (True,))]


@pytest.mark.parametrize("row,noise", BLOCK_RUNS,
                         ids=["%s-%s-%s" % (r[0], "fused_scale" if r[1][4] else "plain", n) for r, n in BLOCK_RUNS])
def test_blocks_with_the_switch_on_against_off(blocks, monkeypatch, row, noise):
    kind, args, shape = row
    on = block_run(blocks, monkeypatch, kind, args, shape, True, noise)
    off = block_run(blocks, monkeypatch, kind, args, shape, False, noise)
    for a, b in zip(on[0], off[0]):
        assert torch.equal(a, b)
    assert set(on[1]) == set(off[1])
    for k in on[1]:
        a, b = on[1][k], off[1][k]
        assert (a is None) == (b is None), k
        if a is None:
            continue
        if on[5] or off[5]:  # (torch's own convolution backward ran: not bit-reproducible from call to call on this backend)
            assert O.nerr(a, b) <= S.GRAD_GATE, k
        else:
            assert torch.equal(a, b), k
    # no blur kernel with the switch on (every plane here is below the LDS bound); today's sequence with it off
    assert (on[2], on[3]) == (0, 0) and (off[2], off[3]) == (1, 1)
    if kind == "DecodeBlock":
        assert on[4] == [("style_layer", True), ("style_layer", False)]
        assert off[4] == [("blur", False), ("style_layer", False), ("style_layer", False)]
    else:
        assert on[4] == [("stat_norm", True), ("stat_norm", False)]
        assert off[4] == [("stat_norm", False), ("blur", False), ("stat_norm", False)]


def test_a_decoder_plane_above_the_bound_ends_with_one_blur_call(blocks, monkeypatch):
    """[1, 2, 64, 66] upscaled to 128 x 132 = 16896 elements a plane: the backward of the fused pair writes the gradient with
    respect to blur(x) and ops.style_blur finishes it, once; the forward still calls no blur.  That class measured as a
    loss, so the block's size test (blocks.FUSE_BLUR_DEC_MAX_HW, the LDS bound) keeps the composition for it: the fused
    pair is reached with the size test lifted, and with it in place the calls are today's"""
    kind, args, shape = "DecodeBlock", (2, 2, 4, True, False, 0), (1, 2, 64, 66)
    assert 4 * shape[2] * shape[3] > LDS_BOUND and blocks.FUSE_BLUR_DEC_MAX_HW == LDS_BOUND
    kept = block_run(blocks, monkeypatch, kind, args, shape, True)
    assert (kept[2], kept[3]) == (1, 1) and kept[4] == [("blur", False), ("style_layer", False), ("style_layer", False)]
    monkeypatch.setattr(blocks, "FUSE_BLUR_DEC_MAX_HW", None)
    on = block_run(blocks, monkeypatch, kind, args, shape, True)  # (its monkeypatch.undo() puts the size test back)
    assert blocks.FUSE_BLUR_DEC_MAX_HW == LDS_BOUND
    off = block_run(blocks, monkeypatch, kind, args, shape, False)
    assert (on[2], on[3]) == (0, 1) and (off[2], off[3]) == (1, 1)
    assert on[4] == [("style_layer", True), ("style_layer", False)]
    assert torch.equal(on[0][0], off[0][0])
    for k in on[1]:
        if on[5] or off[5]:
            assert O.nerr(on[1][k], off[1][k]) <= S.GRAD_GATE, k
        else:
            assert torch.equal(on[1][k], off[1][k]), k
