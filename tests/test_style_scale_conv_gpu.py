"""GPU checks of the style variant's fused_scale convolutions on the HIP kernels: ops.conv3x3_flip_transpose,
functional.conv_upscale / conv_downscale (one autograd node over the three phase-form upsample-convolution ops),
blocks._Conv3x3's choice between them and torch's stride-2 convolutions, the drop-in blocks against the fixture recorded
from the reference (tests/golden/style_scale_blocks.npz) and whole networks with the switch on against the switch off.

A shape is (B, Cl, Cf, h, w): "up" reads [B, Cl, h, w] and writes [B, Cf, 2h, 2w], "down" the other way round.

Tolerances.  The functions against the float64 CPU formula of the REFERENCE's form (F.conv_transpose2d / strided F.conv2d
over the four-shift sum of the weight): kernel_checks._err <= kernel_checks.WINO_TOL for the output, dx and dw, the figure
the same three kernels are held to in kernel_checks.py.  The weight transform adds no rounding (a copy; x 1/4 is exact and
commutes with every rounding of a linear kernel), so the gate is theirs unchanged.  Inputs are float32-exact doubles.
Blocks: the criteria of test_style_gpu.py (O.viol <= 1 for outputs, BLOCK_GRAD_GATE for gradients), imported.  Networks:
test_style_model_gpu.CLASS_GRAD_GATE between the kernels and torch's own stride-2 convolutions."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_checks as K
import style_net_fixture as NF
import style_oracle as O
import test_style_gpu as TS
import test_style_model_gpu as TM
from test_style_scale_conv_host import REFUSED, TAKEN, layer_args

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
ROWS = list(TAKEN)
FIRST, SPLITK = ROWS[0], (1, 128, 128, 8, 16)
KINDS = ("up", "down")
put = TS.put


def never(name):
    def fail(*a, **k):
        raise AssertionError("%s was called" % name)
    return fail


def shifted_sum(w):
    w = F.pad(w, (1, 1, 1, 1))
    return w[:, :, 1:, 1:] + w[:, :, :-1, 1:] + w[:, :, 1:, :-1] + w[:, :, :-1, :-1]


def torch_lines(kind, x, w):
    """the reference's form, which is also what blocks._Conv3x3 runs without the kernels"""
    if kind == "up":
        return F.conv_transpose2d(x, shifted_sum(w), None, stride=2, padding=1)
    return F.conv2d(x, shifted_sum(w) * 0.25, None, stride=2, padding=1)


def T(w):
    return w.transpose(0, 1).flip(2, 3)


def draw(kind, shape, seed=0):
    """float32-exact float64 x, parameter-layout w and upstream gradient gy of a layer"""
    B, Ci, Co, H, W = layer_args(kind, shape)
    g = torch.Generator().manual_seed(100 * seed + 7 * B + 13 * Ci + 29 * Co + 3 * H + W + (kind == "down"))
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()  # noqa: E731
    w = (r(Ci, Co, 3, 3) if kind == "up" else r(Co, Ci, 3, 3)) / math.sqrt(9.0 * Ci)
    x = r(B, Ci, H, W)
    gy = r(B, Co, 2 * H, 2 * W) if kind == "up" else r(B, Co, H // 2, W // 2)
    return x, w.float().double(), gy


def oracle(kind, x, w, gy):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = torch_lines(kind, x, w)
    dx, dw = torch.autograd.grad(y, (x, w), gy)
    return y.detach(), dx, dw


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """(x, w, gy) and the float64 reference (y, dx, dw), computed once and shared"""
    d = draw(kind, shape)
    return d, oracle(kind, *d)


def fn_of(kind):
    from sivae_hip import functional as SF
    return SF.conv_upscale if kind == "up" else SF.conv_downscale


def run(kind, x, w, gy, x_grad=True, w_grad=True):
    """the Function on the device -> (y, dx, dw, the parameter)"""
    xg = put(x).requires_grad_(x_grad)
    wg = torch.nn.Parameter(put(w), requires_grad=w_grad)
    y = fn_of(kind)(xg, wg)
    y.backward(put(gy))
    return y.detach(), xg.grad, wg.grad, wg


@pytest.fixture(scope="module")
def blocks():
    import sys
    sys.path.insert(0, TS.BLOCKS_DIR)
    try:
        import blocks as B
    finally:
        sys.path.remove(TS.BLOCKS_DIR)
    return B


# ------------------------------------------------------------------------------------------------ the weight transform
@pytest.mark.parametrize("scale", [1.0, 0.25, 0.3])
@pytest.mark.parametrize("rs", [(1, 1), (3, 5), (72, 20), (128, 128)], ids=lambda v: "%dx%d" % v)
def test_flip_transpose_is_exact(rs, scale):
    from sivae_hip import ops
    from support.guard import describe, guarded
    R, S = rs
    w = torch.randn(R, S, 3, 3, generator=torch.Generator().manual_seed(R + S)).to(DEV)
    want = w.transpose(0, 1).flip(2, 3) * scale
    got = ops.conv3x3_flip_transpose(w, scale)
    assert got.shape == (S, R, 3, 3) and got.is_contiguous() and torch.equal(got, want)
    if scale in (1.0, 0.25):  # (its own inverse, exactly)
        assert torch.equal(ops.conv3x3_flip_transpose(got, 1.0 / scale), w)
    with guarded(ops) as g:  # a destination 3 elements into a buffer, as a gradient slab view sits in its flat buffer
        out = g.place(torch.full((S, R, 3, 3), float("nan"), device=DEV), offset_elems=3)
        assert out.data_ptr() % 16 == 12
        res = ops.conv3x3_flip_transpose(w, scale, out=out)
        fresh = ops.conv3x3_flip_transpose(w, scale)  # (allocated by the proxy: guarded and poisoned)
        damage = g.verify()
        assert not damage, "guard damage:\n%s" % describe(damage)
    assert res is out and torch.equal(out, want) and torch.equal(fresh, want)
    with pytest.raises(ValueError):
        ops.conv3x3_flip_transpose(w, scale, out=torch.empty(R, S, 3, 3, device=DEV)[..., :2])
    with pytest.raises(ValueError):
        ops.conv3x3_flip_transpose(w.view(R, S, 9, 1))
    with pytest.raises(TypeError):
        ops.conv3x3_flip_transpose(w.double())


# ------------------------------------------------------------------------------------------------ the functions
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ROWS, ids=lambda s: "x".join(map(str, s)))
def test_functions_against_the_reference_form(shape, kind):
    (x, w, gy), (y_ref, dx_ref, dw_ref) = case(kind, shape)
    y, dx, dw, wg = run(kind, x, w, gy)
    errs = dict(y=K._err(y, y_ref), dx=K._err(dx, dx_ref), dw=K._err(dw, dw_ref))
    print("conv_%sscale %s: %s (gate %.1e)" % (kind, shape, ", ".join("%s %.2e" % kv for kv in errs.items()), K.WINO_TOL))
    assert dw.shape == wg.shape and dx.shape == x.shape
    for k, e in errs.items():
        assert e <= K.WINO_TOL, (k, e)


def three_ops(kind, shape):
    """bit for bit: the effective weight is T(w) (x 1/4 for down) and every result one call of an existing op
    -> (the Function's y, dx, dw; x, gy and the two packs of the effective weight on the device)"""
    from sivae_hip import ops
    (x, w, gy), _ = case(kind, shape)
    B, Cl, Cf, h, wd = shape
    y, dx, dw, _ = run(kind, x, w, gy)
    xg, gyg = put(x), put(gy)
    e = (T(put(w)) * (1.0 if kind == "up" else 0.25)).contiguous()
    assert e.shape == (Cf, Cl, 3, 3)
    wp0, wp1 = ops.PackedW(e, 0), ops.PackedW(e, 1)
    if kind == "up":
        assert torch.equal(y, ops.conv2d_fwd(xg, wp0, Cf, 3, upsample=True))
        assert torch.equal(dx, ops.conv2d_up_dgrad(gyg, wp0, Cl, wp1=wp1))
        de = ops.conv2d_wgrad(xg, gyg, 3, upsample=True)
    else:
        assert torch.equal(y, ops.conv2d_up_dgrad(xg, wp0, Cl, wp1=wp1))
        assert torch.equal(dx, ops.conv2d_fwd(gyg, wp0, Cf, 3, upsample=True))
        de = ops.conv2d_wgrad(gyg, xg, 3, upsample=True)
    assert de.shape == (Cf, Cl, 3, 3)
    assert torch.equal(dw, ops.conv3x3_flip_transpose(de, 1.0 if kind == "up" else 0.25))
    assert torch.equal(dw, T(de) * (1.0 if kind == "up" else 0.25))
    return (y, dx, dw), (xg, gyg, wp0, wp1)


@pytest.mark.parametrize("kind", KINDS)
def test_the_function_is_the_three_ops(kind):
    three_ops(kind, FIRST)


@pytest.mark.parametrize("kind", KINDS)
def test_refused_shapes_raise_in_the_function(kind):
    for shape in REFUSED:
        x, w, _ = draw(kind, shape)
        with pytest.raises(ValueError, match="no kernel route"):
            fn_of(kind)(put(x), put(w))
    x, w, _ = draw(kind, FIRST)
    with pytest.raises(RuntimeError, match="conv_%sscale of x" % kind):
        fn_of(kind)(put(x), put(w).transpose(0, 1).contiguous())  # (the other layer's layout)


# ------------------------------------------------------------------------------------------------ _Conv3x3's choice
def conv_module(blocks, kind, w):
    Ci, Co = (w.shape[0], w.shape[1]) if kind == "up" else (w.shape[1], w.shape[0])
    m = blocks._Conv3x3(Ci, Co, kind)
    with torch.no_grad():
        m.weight.copy_(w)
    return m.to(DEV)


def refused_inputs(kind):
    """the two refused rows; the second one's down input has odd sides (11 x 15)"""
    a = draw(kind, REFUSED[0])
    x, w, gy = draw(kind, REFUSED[1])
    if kind == "down":
        g = torch.Generator().manual_seed(5)
        x = torch.randn(1, 4, 11, 15, generator=g, dtype=torch.float64).float().double()
        gy = torch.randn(1, 4, 5, 7, generator=g, dtype=torch.float64).float().double()  # ((11 + 2 - 4) // 2 + 1 rows)
    return [a, (x, w, gy)]


def module_run(m, x, gy):
    xg = put(x).requires_grad_(True)
    m.weight.grad = None
    y = m(xg)
    y.backward(put(gy))
    return y.detach(), xg.grad, m.weight.grad


def lines_run(kind, x, w, gy):
    """today's torch lines on the device"""
    xg, wg = put(x).requires_grad_(True), put(w).requires_grad_(True)
    y = torch_lines(kind, xg, wg)
    y.backward(put(gy))
    return y.detach(), xg.grad, wg.grad


@pytest.mark.parametrize("kind", KINDS)
def test_refused_shapes_take_the_torch_lines(blocks, monkeypatch, kind):
    from sivae_hip import ops
    for x, w, gy in refused_inputs(kind):
        want = lines_run(kind, x, w, gy)
        m = conv_module(blocks, kind, w)
        for name in ("conv2d_fwd", "conv2d_up_dgrad", "conv2d_wgrad", "conv3x3_flip_transpose"):
            monkeypatch.setattr(ops, name, never("ops." + name))
        got = module_run(m, x, gy)
        monkeypatch.undo()
        assert torch.equal(got[0], want[0]), tuple(x.shape)
        # (the gradients of the same torch ops: torch's convolution backward is not bit-reproducible from call to call
        # on this backend, see test_switch_off_is_todays_lines)
        assert K._err(got[1], want[1]) <= K.WINO_TOL and K._err(got[2], want[2]) <= K.WINO_TOL, tuple(x.shape)


def no_torch_convolution(blocks, monkeypatch, kind, shape, tols=(K.WINO_TOL,) * 3):
    """with torch's convolutions patched to fail, forward and backward of a taken row pass (tols: of y, dx, dw)"""
    (x, w, gy), ref = case(kind, shape)
    m = conv_module(blocks, kind, w)
    monkeypatch.setattr(F, "conv_transpose2d", never("F.conv_transpose2d"))
    monkeypatch.setattr(F, "conv2d", never("F.conv2d"))
    monkeypatch.setattr(torch, "conv2d", never("torch.conv2d"))
    monkeypatch.setattr(torch, "conv_transpose2d", never("torch.conv_transpose2d"))
    got = module_run(m, x, gy)
    monkeypatch.undo()
    for a, b, tol in zip(got, ref, tols):
        assert K._err(a, b) <= tol
    assert "_sivae_scale_pack" in m.weight.__dict__ and "_sivae_pack" not in m.weight.__dict__


@pytest.mark.parametrize("kind", KINDS)
def test_taken_shapes_call_no_torch_convolution(blocks, monkeypatch, kind):
    """the converse of the refused shapes"""
    no_torch_convolution(blocks, monkeypatch, kind, FIRST)


@pytest.mark.parametrize("kind", KINDS)
def test_switch_off_is_todays_lines(blocks, monkeypatch, kind):
    from sivae_hip import ops
    (x, w, gy), ref = case(kind, FIRST)
    want = lines_run(kind, x, w, gy)
    m = conv_module(blocks, kind, w)
    monkeypatch.setattr(blocks, "SCALE_CONV", False)
    for name in ("conv2d_fwd", "conv2d_up_dgrad", "conv2d_wgrad", "conv3x3_flip_transpose"):
        monkeypatch.setattr(ops, name, never("ops." + name))
    xg = put(x).requires_grad_(True)
    y = m(xg)
    assert type(y.grad_fn).__name__ == "ConvolutionBackward0"  # (torch's own node: its backward is today's, too)
    y.backward(put(gy))
    monkeypatch.undo()
    assert torch.equal(y.detach(), want[0])
    # torch's convolution backward is not bit-reproducible from one call to the next on this backend (its weight gradient
    # differed in the last bits between two runs of the same lines), so the gradients of the same torch ops are held to
    # the fp32 gate instead of to equality
    assert K._err(xg.grad, want[1]) <= K.WINO_TOL and K._err(m.weight.grad, want[2]) <= K.WINO_TOL
    on = module_run(m, x, gy)  # (and on again: the kernels, which round differently from torch's convolution)
    assert all(K._err(a, b) <= K.WINO_TOL for a, b in zip(on, ref))
    assert not all(torch.equal(a, b) for a, b in zip(on, want))


# ------------------------------------------------------------------------------------------------ the cache
def stale_weight(blocks, kind, shape, tol=K.WINO_TOL, dx_tol=None):
    """the effective weight is cached on the parameter: an in-place edit (version counter), a fused optimizer step and a
    weight average (both write through raw pointers and bump the generation) each rebuild it.  dx_tol: the data gradient
    is held to the float64 one of the CURRENT weight after every change as well (where only the backward reads an operand
    of its own)"""
    from sivae_hip import functional as SF
    from sivae_hip.lreq_adam import LREQAdam, lerp_parameters
    (x, w, gy), (y_ref, _, _) = case(kind, shape)
    m = conv_module(blocks, kind, w)
    p, xg = m.weight, put(x)

    def check(y):
        now = p.detach().double().cpu()
        want = torch_lines(kind, x, now)
        assert K._err(y, want) <= tol
        if dx_tol is not None:
            _, dx, _ = module_run(m, x, gy)
            assert K._err(dx, oracle(kind, x, now, gy)[1]) <= dx_tol
            p.grad = None
        return y.detach().clone()

    y0 = check(m(xg))
    sw = SF.scale_packed(p, kind)
    assert SF.scale_packed(p, kind) is sw and torch.equal(m(xg), y0)  # (one build per weight version)
    with torch.no_grad():
        p.mul_(2)
    y1 = check(m(xg))
    assert SF.scale_packed(p, kind) is not sw and not torch.equal(y1, y0)
    p.grad = torch.randn(p.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    opt = LREQAdam([p], lr=0.1)
    opt.step()
    assert opt.last_step["fused"] == 1
    y2 = check(m(xg))
    assert not torch.equal(y2, y1)
    assert lerp_parameters([p], [torch.zeros_like(p)], 0.5)["fused"] == 1
    y3 = check(m(xg))
    assert not torch.equal(y3, y2)
    SF.repack([p], m)  # (the batched repack of the packed-weight cache leaves this cache alone)
    assert torch.equal(m(xg), y3)


@pytest.mark.parametrize("kind", KINDS)
def test_a_stale_effective_weight_would_show(blocks, kind):
    stale_weight(blocks, kind, FIRST)


# ------------------------------------------------------------------------------------------------ needs_input_grad
def wanted_gradients(monkeypatch, kind, shape):
    from sivae_hip import ops
    (x, w, gy), (_, dx_ref, dw_ref) = case(kind, shape)
    full = run(kind, x, w, gy)
    # a frozen weight: no weight gradient, no transform of one
    monkeypatch.setattr(ops, "conv2d_wgrad", never("ops.conv2d_wgrad"))
    y, dx, dw, _ = run(kind, x, w, gy, w_grad=False)
    monkeypatch.undo()
    assert dw is None and torch.equal(dx, full[1]) and torch.equal(y, full[0])
    # an input without a gradient: no data gradient (patched after the forward, which uses the other kernel's op)
    xg, wg = put(x), torch.nn.Parameter(put(w))
    y = fn_of(kind)(xg, wg)
    monkeypatch.setattr(ops, "conv2d_up_dgrad" if kind == "up" else "conv2d_fwd", never("the data gradient's op"))
    y.backward(put(gy))
    monkeypatch.undo()
    assert xg.grad is None and torch.equal(wg.grad, full[2])
    # nothing requires a gradient: the forward alone
    assert torch.equal(fn_of(kind)(put(x), put(w)), full[0])


@pytest.mark.parametrize("kind", KINDS)
def test_only_wanted_gradients_are_launched(monkeypatch, kind):
    wanted_gradients(monkeypatch, kind, FIRST)


def gradient_slabs(kind, shape):
    """the slot protocol of ConvBiasFn / LinearFn: no slab is claimed under no_grad; a claimed one receives the gradient
    (a view 3 elements into its buffer) and autograd receives None; a use beyond the slabs goes back to autograd"""
    (x, w, gy), _ = case(kind, shape)
    full = run(kind, x, w, gy)
    wg = torch.nn.Parameter(put(w))
    n = wg.numel()
    buf = torch.full((n + 8,), float("nan"), device=DEV)
    wg.__dict__["_sivae_slabs"] = [buf[3:3 + n].view(wg.shape)]
    wg.__dict__["_sivae_use"] = 0
    with torch.no_grad():
        y = fn_of(kind)(put(x), wg)
    assert wg.__dict__["_sivae_use"] == 0 and torch.equal(y, full[0])
    xg = put(x).requires_grad_(True)
    y = fn_of(kind)(xg, wg)
    assert wg.__dict__["_sivae_use"] == 1
    y2 = fn_of(kind)(xg, wg)  # (a second use: no slab left)
    assert wg.__dict__["_sivae_use"] == 1
    y.backward(put(gy))
    assert wg.grad is None and torch.equal(xg.grad, full[1])
    assert torch.equal(buf[3:3 + n].view(wg.shape), full[2])
    assert bool(torch.isnan(buf[:3]).all()) and bool(torch.isnan(buf[3 + n:]).all())
    y2.backward(put(gy))
    assert torch.equal(wg.grad, full[2])


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_slabs(kind):
    gradient_slabs(kind, FIRST)


# ------------------------------------------------------------------------------------------------ guarded
def guarded_run(shape, kinds=KINDS):
    """forward and backward of both functions on guarded, poisoned outputs and exact workspaces"""
    from sivae_hip import ops
    from support.guard import describe, guarded
    for kind in kinds:
        (x, w, gy), _ = case(kind, shape)
        base = run(kind, x, w, gy)
        with guarded(ops) as g:
            got = run(kind, x, w, gy)  # (a fresh parameter: its effective weight and operands are built in here)
            damage = g.verify()
            assert not damage, "guard damage:\n%s" % describe(damage)
        for a, b in zip(got[:3], base[:3]):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (kind, shape)


@pytest.mark.parametrize("shape", [FIRST, SPLITK], ids=lambda s: "x".join(map(str, s)))
def test_guarded(shape):
    guarded_run(shape)


# ------------------------------------------------------------------------------------------------ the blocks
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "style_scale_blocks.npz"))


@pytest.mark.parametrize("name", ["dec_fused_up", "enc_fused_down"])
def test_fused_scale_blocks_against_the_reference(fx, blocks, monkeypatch, name):
    """the drop-in blocks with fused_scale=True against the run recorded from the reference's net.py, as
    test_style_gpu.test_blocks_against_the_reference holds the fused_scale=False ones"""
    from sivae_hip import functional as SF
    meta = json.loads(str(fx[name + "/meta"]))
    pre = name + "/param/"
    m = getattr(blocks, meta["block"])(**meta["kwargs"])
    m.load_state_dict({k[len(pre):]: torch.from_numpy(fx[k]).float() for k in fx.files if k.startswith(pre)}, strict=True)
    m = m.to(DEV)
    pin = name + "/in/"
    ins = {k[len(pin):]: put(torch.from_numpy(fx[k])).requires_grad_(True) for k in fx.files if k.startswith(pin)}
    queue = [fx["%s/noise%d" % (name, i)] for i in range(2)] if meta["noise"] else []
    drawn, taken = [], []

    def randn(shape, device=None, **kw):
        nz = queue[len(drawn)]
        assert list(shape) == list(nz.shape) and str(device).startswith("cuda")
        drawn.append(1)
        return torch.from_numpy(nz).float().to(device)

    def counted(kind, f):
        def call(x, w):
            taken.append(kind)
            return f(x, w)
        return call

    monkeypatch.setattr(torch, "randn", randn)
    monkeypatch.setattr(SF, "conv_upscale", counted("up", SF.conv_upscale))
    monkeypatch.setattr(SF, "conv_downscale", counted("down", SF.conv_downscale))
    outs = m(ins["x"], ins["s1"], ins["s2"], meta["noise"]) if meta["block"] == "DecodeBlock" else m(ins["x"])
    monkeypatch.undo()
    assert len(drawn) == len(queue) and taken == ["up" if meta["block"] == "DecodeBlock" else "down"]
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * put(torch.from_numpy(fx["%s/g%d" % (name, i)]))).sum() for i, o in enumerate(outs)).backward()
    worst_v = max(O.viol(o, torch.from_numpy(fx["%s/out%d" % (name, i)])) for i, o in enumerate(outs))
    pg = name + "/grad/"
    have = dict(list(ins.items()) + list(m.named_parameters()))
    errs = {k[len(pg):]: O.nerr(have[k[len(pg):]].grad, torch.from_numpy(fx[k])) for k in fx.files if k.startswith(pg)}
    print("%s: outputs %.3f of the criterion, gradients worst %.2e (%s; gate %.1e)"
          % (name, worst_v, max(errs.values()), max(errs, key=errs.get), TS.BLOCK_GRAD_GATE))
    assert worst_v <= 1.0
    assert max(errs.values()) <= TS.BLOCK_GRAD_GATE, errs
    for k, p in m.named_parameters():  # (a parameter the reference gave no gradient gets none here)
        assert (p.grad is not None) == ((pg + k) in fx.files), k


@pytest.mark.parametrize("name", ["dec_fused_up", "enc_fused_down"])
def test_constructors_give_the_reference_state(fx, blocks, name):
    """state dicts bit for bit per seed and the coefficients custom_adam.py reads, built on the device's host side as the
    training script builds them"""
    meta = json.loads(str(fx[name + "/meta"]))
    cls = getattr(blocks, meta["block"])
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = cls(**meta["kwargs"])
        want = {k[len(name) + 7:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("%s/init%d/" % (name, seed))}
        sd = m.state_dict()
        assert list(sd) == list(want)
        for k, v in want.items():
            assert sd[k].dtype == v.dtype == torch.float32 and torch.equal(sd[k], v), (seed, k)
    coef = {k: float(fx[kk]) for kk in fx.files if kk.startswith(name + "/coef/") for k in [kk[len(name) + 6:]]}
    got = {k: float(p.lr_equalization_coef) for k, p in m.to(DEV).named_parameters() if hasattr(p, "lr_equalization_coef")}
    assert got == coef and len(coef) >= 6


# ------------------------------------------------------------------------------------------------ the networks
NET_CFG = dict(startf=2, maxf=8, layer_count=6, latent_size=8)  # 128 x 128: the smallest networks with fused_scale layers


def net_run(net, blocks, cls, on, leads, cfg=None, batch=2):
    """forward at lod 5 and the gradients of sum(out g) for every parameter, with blocks.SCALE_CONV = on.  leads: filled
    with the lead term of the generator's decode_block.0.bias_1, whose gradient is exactly 0 (the first layer normalises
    the constant plane, and the noise weights start at 0): measured against the size of the terms of that difference,
    lead = max |r (style + 1)| max |dy| from the layer's own call, as test_style_net_gpu measures it"""
    from sivae_hip import style
    torch.manual_seed(11)
    m = getattr(net, cls)(**(cfg or NET_CFG)).to(DEV)
    g = torch.Generator().manual_seed(12)
    old, style_layer, seen = blocks.SCALE_CONV, style.style_layer, []

    def spy(x, noise_weight, bias, st, *a, **k):
        y = style_layer(x, noise_weight, bias, st, *a, **k)
        if not seen:
            seen.append(float((st.detach()[:, :x.shape[1]] + 1).abs().max()) / 1e-8 ** 0.5)
            y.register_hook(lambda gr: leads.update({"decode_block.0.bias_1": seen[0] * float(gr.abs().max())}))
        return y

    blocks.SCALE_CONV = on
    style.style_layer = spy
    try:
        torch.manual_seed(13)  # (the generator's noise draws)
        if cls == "Generator":
            styles = torch.randn(batch, 12, 8, generator=g).to(DEV)
            out = m(styles, 5, 1, True)
            assert out.shape == (batch, 3, 128, 128)
        else:
            out = m(torch.randn(batch, 3, 128, 128, generator=g).to(DEV), 5, 1)
        (out * torch.randn(out.shape, generator=g).to(DEV)).sum().backward()
    finally:
        blocks.SCALE_CONV, style.style_layer = old, style_layer
    return out.detach(), {k: p.grad for k, p in m.named_parameters()}, m


def switch_on_against_off(blocks, monkeypatch, cls, cfg=None, batch=2):
    """the kernels against torch's own stride-2 convolutions inside whole networks (one fused_scale layer each at 128 x 128)
    -> the errors it held to the gate, and the module"""
    from sivae_hip import functional as SF
    net = NF.import_net()
    assert net.DecodeBlock is blocks.DecodeBlock  # (one blocks module: the switch below is the one the network reads)
    taken = []
    for kind, f in (("up", SF.conv_upscale), ("down", SF.conv_downscale)):
        monkeypatch.setattr(SF, "conv_%sscale" % kind, lambda x, w, f=f, kind=kind: (taken.append(kind), f(x, w))[1])
    leads = {}
    out_off, g_off, m = net_run(net, blocks, cls, False, leads, cfg, batch)
    assert taken == [] and (cls == "Generator") == bool(leads)
    out_on, g_on, _ = net_run(net, blocks, cls, True, {}, cfg, batch)
    monkeypatch.undo()
    assert taken == ["up" if cls == "Generator" else "down"]
    fused = [b for b in (m.decode_block if cls == "Generator" else m.encode_block) if b.fused_scale]
    assert len(fused) == 1
    errs = {"out": O.nerr(out_on, out_off)}
    for k, ref in g_off.items():
        assert (ref is None) == (g_on[k] is None), k
        if ref is not None and float(ref.abs().max()) == 0:
            assert float(g_on[k].abs().max()) == 0, k  # (a gradient that is exactly zero stays exactly zero)
        elif ref is not None:
            errs[k] = O.nerr(g_on[k], ref, leads.get(k, 0.0))
    print("%s 128x128 on against off: output %.2e, gradients worst %.2e (%s; gate %.0e)"
          % (cls, errs["out"], max(errs.values()), max(errs, key=errs.get), TM.CLASS_GRAD_GATE))
    assert max(errs.values()) <= TM.CLASS_GRAD_GATE, errs
    return errs, fused[0]


@pytest.mark.parametrize("cls", ["Generator", "Encoder"])
def test_networks_with_the_switch_on_against_off(blocks, monkeypatch, cls):
    switch_on_against_off(blocks, monkeypatch, cls)
