"""Host checks (no GPU) of the style variant's fused_scale convolutions on the HIP kernels: the routes
ops.scale_conv_routes chooses from integers alone, the argument checks of sivae_conv3x3_flip_transpose, the torch lines
blocks._Conv3x3 keeps for CPU tensors, the weight identities the feature rests on, and the new fixture.

A shape is (B, Cl, Cf, h, w): Cl channels on the low-resolution side [B, Cl, h, w], Cf on the full-resolution side
[B, Cf, 2h, 2w]; "up" reads the former, "down" the latter."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import style_oracle as O
from sivae_hip import lib

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS_DIR = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd", "style_soft_intro_vae")
SCALE_CASES = ("dec_fused_up", "enc_fused_down")

NARROW = ("conv_wino_up_kernel<2,3,false>", "conv_wino_up_dgrad_kernel<2,3>")
WIDE = ("conv_wino_up_kernel<1,4,false>", "conv_wino_up_dgrad_kernel<1,4>")
# shape -> (kernel of the upsample convolution, kernel of its phase data gradient, family and split of the latter)
TAKEN = {
    (2, 8, 6, 8, 16): NARROW + ("wino_up_dgrad", 1),
    (1, 20, 72, 16, 32): WIDE + ("wino_up_dgrad", 1),
    (1, 72, 20, 16, 32): WIDE + ("wino_up_dgrad", 1),
    (2, 72, 20, 8, 16): NARROW + ("wino_up_dgrad", 1),
    (1, 3, 5, 10, 18): NARROW + ("wino_up_dgrad", 1),
    (1, 128, 128, 8, 16): NARROW + ("wino_up_dgrad_splitk", 2),
}
POOL = ("conv_wino_up_kernel<1,4,false>", "conv_wino4_pool_kernel<false>")
# The routes TAKEN never takes, at 256 CUs (tests/test_style_scale_edges_host.py says what each row is for and holds the two
# tables to the route functions; tests/test_style_scale_edges_gpu.py runs them): the same layout, then the number of
# slices of the weight gradient
EDGE = {
    (8, 16, 16, 64, 64): POOL + ("wino4_pool", 1, 32),
    (8, 5, 24, 64, 64): POOL + ("wino4_pool", 1, 32),
    (8, 64, 16, 64, 64): POOL + ("wino4_pool", 1, 32),
    (8, 65, 16, 64, 64): WIDE + ("wino_up_dgrad", 1, 32),
    (7, 16, 16, 64, 64): WIDE + ("wino_up_dgrad", 1, 28),
    (8, 16, 15, 64, 64): WIDE + ("wino_up_dgrad", 1, 32),
    (8, 16, 16, 64, 72): WIDE + ("wino_up_dgrad", 1, 40),
    (8, 3, 65, 64, 64): POOL + ("wino4_pool", 1, 32),
    (1, 128, 128, 8, 32): WIDE + ("wino_up_dgrad_splitk", 2, 1),
    (1, 128, 256, 8, 16): NARROW + ("wino_up_dgrad_splitk", 4, 1),
    (1, 128, 512, 8, 16): NARROW + ("wino_up_dgrad_splitk", 8, 1),
    (5, 4, 6, 10, 40): WIDE + ("wino_up_dgrad", 1, 2),
    (1, 3, 5, 9, 18): NARROW + ("wino_up_dgrad", 1, 1),
    # the remaining combinations of tile, split and slices the closure sweep of the edges file meets
    (6, 3, 5, 9, 18): NARROW + ("wino_up_dgrad", 1, 2),
    (4, 65, 128, 10, 40): WIDE + ("wino_up_dgrad_splitk", 2, 2),
    (1, 65, 256, 10, 40): WIDE + ("wino_up_dgrad_splitk", 4, 1),
    (4, 65, 256, 10, 40): WIDE + ("wino_up_dgrad_splitk", 4, 2),
    (1, 65, 512, 10, 40): WIDE + ("wino_up_dgrad_splitk", 8, 1),
    (4, 65, 512, 10, 40): WIDE + ("wino_up_dgrad_splitk", 8, 2),
    (16, 65, 128, 8, 16): NARROW + ("wino_up_dgrad_splitk", 2, 2),
    (16, 65, 256, 8, 16): NARROW + ("wino_up_dgrad_splitk", 4, 2),
    (16, 65, 512, 8, 16): NARROW + ("wino_up_dgrad_splitk", 8, 2),
}
REFUSED = [(2, 3, 5, 4, 6), (1, 4, 4, 5, 7)]
# configs/ffhq256.yaml (startf 64, maxf 512, 7 layers): kind, Ci, Co, input side
FFHQ256 = [("up", 256, 128, 64), ("up", 128, 64, 128), ("down", 64, 128, 256), ("down", 128, 256, 128)]


def layer_args(kind, shape):
    """a shape of the table -> the (B, Ci, Co, H, W) of the layer's INPUT"""
    B, Cl, Cf, h, w = shape
    return (B, Cl, Cf, h, w) if kind == "up" else (B, Cf, Cl, 2 * h, 2 * w)


@pytest.fixture(scope="module")
def blocks():
    sys.path.insert(0, BLOCKS_DIR)
    try:
        import blocks as B
    finally:
        sys.path.remove(BLOCKS_DIR)
    return B


@pytest.mark.parametrize("kind", ["up", "down"])
@pytest.mark.parametrize("shape", list(TAKEN), ids=lambda s: "x".join(map(str, s)))
def test_routes_of_the_taken_shapes(shape, kind):
    from sivae_hip import ops
    conv_key, adj_key, adj_family, split = TAKEN[shape]
    r = ops.scale_conv_routes(kind, *layer_args(kind, shape))
    assert r.refused is None
    conv, adj = (r.forward, r.dgrad) if kind == "up" else (r.dgrad, r.forward)  # (the same two ops, seats swapped)
    assert (conv.family, conv.key, conv.ws_bytes) == ("wino_up", conv_key, 0)
    assert (adj.family, adj.key, adj.split) == (adj_family, adj_key, split)
    assert (adj.ws_bytes > 0) == (split > 1)
    assert (r.wgrad.family, r.wgrad.key) == ("wino_up_wgrad", "wino_up_wgrad_kernel") and r.wgrad.ws_bytes > 0
    assert all(x.error is None for x in (r.forward, r.dgrad, r.wgrad))
    # the routes are those of the ops the Function calls, at the sizes it calls them with
    B, Cl, Cf, h, w = shape
    assert conv == ops.conv2d_fwd_route(B, Cl, Cf, 2 * h, 2 * w, 3, upsample=True)
    assert adj == ops.conv2d_up_dgrad_route(B, Cf, Cl, 2 * h, 2 * w, has_wp1=True)
    assert r.wgrad == ops.conv2d_wgrad_route(B, Cl, Cf, 2 * h, 2 * w, 3, upsample=True)


@pytest.mark.parametrize("kind", ["up", "down"])
def test_refused_shapes(kind):
    from sivae_hip import ops
    for shape in REFUSED:
        assert ops.scale_conv_routes(kind, *layer_args(kind, shape)).refused, shape
        assert not ops.conv2d_up_dgrad_supported(shape[3], shape[4])
    odd = ops.scale_conv_routes("down", 1, 4, 4, 11, 15)
    assert odd.refused and "odd" in odd.refused and odd.forward is None
    assert ops.scale_conv_routes("down", 1, 4, 4, 32, 15).refused and ops.scale_conv_routes("down", 1, 4, 4, 11, 32).refused
    with pytest.raises(ValueError):
        ops.scale_conv_routes("sideways", 1, 4, 4, 16, 16)


def test_a_route_with_an_error_refuses_the_layer(monkeypatch):
    from sivae_hip import ops
    bad = ops.Route("direct", "sivae_conv2d_fwd", error=(ValueError, "planted"))
    monkeypatch.setattr(ops, "conv2d_wgrad_route", lambda *a, **k: bad)
    assert ops.scale_conv_routes("up", 2, 8, 6, 8, 16).refused == "planted"
    monkeypatch.undo()
    assert ops.scale_conv_routes("up", 2, 8, 6, 8, 16).refused is None


@pytest.mark.parametrize("B", [4, 8])
def test_the_ffhq256_layers_are_taken(B):
    from sivae_hip import ops
    for kind, Ci, Co, side in FFHQ256:
        r = ops.scale_conv_routes(kind, B, Ci, Co, side, side)
        assert r.refused is None, (kind, Ci, Co, side, r.refused)
        assert {r.forward.family, r.dgrad.family} <= {"wino_up", "wino_up_dgrad", "wino_up_dgrad_splitk", "wino4_pool"}
        assert r.wgrad.family == "wino_up_wgrad"


def test_entry_point_validates_arguments():
    """the documented codes, before any launch (the pointers are not memory)"""
    L = lib.load()
    null, one, odd = None, ctypes.c_void_p(64), ctypes.c_void_p(66)
    f = L.sivae_conv3x3_flip_transpose
    assert lib.parse_header()["sivae_conv3x3_flip_transpose"] == (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2
                                                                  + [ctypes.c_float, ctypes.c_void_p])
    assert f(null, one, 2, 3, 1.0, null) == -1 and f(one, null, 2, 3, 1.0, null) == -1
    for R, S in ((0, 3), (2, 0), (-1, 3), (2, -5)):
        assert f(one, one, R, S, 1.0, null) == -2, (R, S)
    assert f(odd, one, 2, 3, 1.0, null) == -2 and f(one, odd, 2, 3, 1.0, null) == -2
    assert f(one, one, 1 << 15, 1 << 15, 1.0, null) == -5


def test_wrapper_refuses_what_the_kernel_does_not_take():
    from sivae_hip import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv3x3_flip_transpose(torch.zeros(2, 3, 3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv3x3_flip_transpose(torch.zeros(2, 3, 3, 3), 0.25, out=torch.zeros(3, 2, 3, 3))


def T(w):
    return w.transpose(0, 1).flip(2, 3)


def test_the_identities_the_layers_rest_on():
    """float64, CPU: the reference's two stride-2 forms against the 3x3 convolution around a nearest-2x upsample with the
    flip-transposed weight: outputs, data gradients and weight gradients (Cl != Cf, h != w)"""
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    up2 = lambda t: t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)  # noqa: E731
    B, Cl, Cf, h, w = 2, 5, 3, 4, 6
    x, wu = r(B, Cl, h, w).requires_grad_(True), r(Cl, Cf, 3, 3).requires_grad_(True)
    gy = r(B, Cf, 2 * h, 2 * w)
    a = F.conv_transpose2d(x, O._shifted_sum(wu), stride=2, padding=1)
    b = F.conv2d(up2(x), T(wu), padding=1)
    ga, gb = torch.autograd.grad(a, (x, wu), gy), torch.autograd.grad(b, (x, wu), gy)
    assert max(O.nerr(b, a), O.nerr(gb[0], ga[0]), O.nerr(gb[1], ga[1])) <= 1e-13
    x, wd = r(B, Cf, 2 * h, 2 * w).requires_grad_(True), r(Cl, Cf, 3, 3).requires_grad_(True)
    gy = r(B, Cl, h, w)
    a = F.conv2d(x, O._shifted_sum(wd) * 0.25, stride=2, padding=1)
    z = torch.zeros(B, Cl, h, w, dtype=torch.float64, requires_grad=True)
    b, = torch.autograd.grad(F.conv2d(up2(z), 0.25 * T(wd), padding=1), z, x, create_graph=True)  # (the adjoint, linear in x)
    ga, gb = torch.autograd.grad(a, (x, wd), gy), torch.autograd.grad(b, (x, wd), gy)
    assert max(O.nerr(b, a), O.nerr(gb[0], ga[0]), O.nerr(gb[1], ga[1])) <= 1e-13
    assert O.nerr(F.avg_pool2d(F.conv2d(x, wd, padding=1), 2), a) <= 1e-13


@pytest.mark.parametrize("scale", ["up", "down"])
def test_cpu_tensors_take_the_torch_lines(blocks, monkeypatch, scale):
    """CPU tensors: what _Conv3x3 gives today, bit for bit, forward and both gradients, without touching the library"""
    from sivae_hip import functional as SF

    def never(*a, **k):
        raise AssertionError("the HIP path was entered for a CPU tensor")

    monkeypatch.setattr(SF, "conv_upscale", never)
    monkeypatch.setattr(SF, "conv_downscale", never)
    assert blocks.SCALE_CONV is True  # (default on)
    torch.manual_seed(1)
    m = blocks._Conv3x3(8, 6, scale)
    assert tuple(m.weight.shape) == ((8, 6, 3, 3) if scale == "up" else (6, 8, 3, 3))
    x = torch.randn(2, 8, 8, 16, requires_grad=True)
    y = m(x)
    w2 = m.weight.detach().clone().requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    s = F.pad(w2, (1, 1, 1, 1))
    s = s[:, :, 1:, 1:] + s[:, :, :-1, 1:] + s[:, :, 1:, :-1] + s[:, :, :-1, :-1]
    want = (F.conv_transpose2d(x2, s, None, stride=2, padding=1) if scale == "up"
            else F.conv2d(x2, s * 0.25, None, stride=2, padding=1))
    assert torch.equal(y, want) and tuple(y.shape) == ((2, 6, 16, 32) if scale == "up" else (2, 6, 4, 8))
    gy = torch.randn_like(y)
    y.backward(gy)
    want.backward(gy)
    assert torch.equal(x.grad, x2.grad) and torch.equal(m.weight.grad, w2.grad)
    assert list(m.state_dict()) == ["weight"] and float(m.weight.lr_equalization_coef) == float(np.sqrt(2.0) / np.sqrt(72))
    for other in (x.detach().double(), x.detach().half()):  # (other dtypes never reach the kernels either)
        assert not m._on_kernels(other)


def test_switch_reads_the_environment(monkeypatch):
    """a second copy of the module under another name, so that the one the other tests hold is left alone"""
    import importlib.util
    for value, want in (("0", False), ("1", True), (None, True)):
        if value is None:
            monkeypatch.delenv("SIVAE_STYLE_SCALE_CONV", raising=False)
        else:
            monkeypatch.setenv("SIVAE_STYLE_SCALE_CONV", value)
        spec = importlib.util.spec_from_file_location("blocks_switch_probe", os.path.join(BLOCKS_DIR, "blocks.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.SCALE_CONV is want, value


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "style_scale_blocks.npz"))


def group(fx, prefix):
    return {k[len(prefix):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(prefix)}


def test_fixture_is_small_and_says_what_it_should(fx):
    size = os.path.getsize(os.path.join(HERE, "golden", "style_scale_blocks.npz"))
    assert size < os.path.getsize(os.path.join(HERE, "golden", "style_blocks.npz")) and size < (1 << 20)
    assert sorted({k.split("/")[0] for k in fx.files}) == sorted(SCALE_CASES)
    for case in SCALE_CASES:
        meta = json.loads(str(fx[case + "/meta"]))
        assert meta["kwargs"]["fused_scale"] is True
        for k, v in list(group(fx, case + "/in/").items()) + [("g0", torch.from_numpy(fx[case + "/g0"]))]:
            assert v.dtype == torch.float64 and torch.equal(v.float().double(), v), (case, k)  # (exact in float32)
        G = group(fx, case + "/grad/")
        assert ("conv_1.weight" if meta["block"] == "DecodeBlock" else "conv_2.weight") in G
        assert all(float(v.abs().max()) > 0 for v in G.values())
    assert tuple(fx["dec_fused_up/in/x"].shape) == (2, 8, 8, 16) and tuple(fx["dec_fused_up/out0"].shape) == (2, 6, 16, 32)
    assert tuple(fx["dec_fused_up/param/conv_1.weight"].shape) == (8, 6, 3, 3)
    assert tuple(fx["enc_fused_down/in/x"].shape) == (2, 6, 16, 32) and tuple(fx["enc_fused_down/out0"].shape) == (2, 8, 8, 16)
    assert tuple(fx["enc_fused_down/param/conv_2.weight"].shape) == (8, 6, 3, 3)


@pytest.mark.parametrize("case", SCALE_CASES)
def test_oracle_reproduces_the_recorded_blocks(fx, case):
    """tests/style_oracle.py (which the GPU tests' float64 formulas are) against the reference's recorded run"""
    meta = json.loads(str(fx[case + "/meta"]))
    P = {k: v.clone().requires_grad_(True) for k, v in group(fx, case + "/param/").items() if k != "blur.weight"}
    ins = {k: v.clone().requires_grad_(True) for k, v in group(fx, case + "/in/").items()}
    kw = meta["kwargs"]
    if meta["block"] == "DecodeBlock":
        noises = [torch.from_numpy(fx["%s/noise%d" % (case, i)]) for i in range(2)]
        outs = (O.decode_block(P, ins["x"], ins["s1"], ins["s2"], meta["noise"], noises, True, True, kw["layer"]),)
    else:
        outs = O.encode_block(P, ins["x"], False, True)
    sum((o * torch.from_numpy(fx["%s/g%d" % (case, i)])).sum() for i, o in enumerate(outs)).backward()
    worst = max(O.nerr(o, torch.from_numpy(fx["%s/out%d" % (case, i)])) for i, o in enumerate(outs))
    want = group(fx, case + "/grad/")
    got = {k: v.grad for k, v in list(ins.items()) + list(P.items()) if v.grad is not None}
    assert set(got) == set(want)
    worst = max([worst] + [O.nerr(got[k], v) for k, v in want.items()])
    print("%s: oracle against the reference, worst relative error %.3e" % (case, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("case", SCALE_CASES)
def test_constructors_give_the_reference_state(fx, blocks, case):
    meta = json.loads(str(fx[case + "/meta"]))
    cls = getattr(blocks, meta["block"])
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = cls(**meta["kwargs"])
        want = group(fx, "%s/init%d/" % (case, seed))
        sd = m.state_dict()
        assert list(sd) == list(want)  # (the keys, in order)
        for k, v in want.items():
            assert sd[k].dtype == v.dtype == torch.float32 and torch.equal(sd[k], v), (seed, k)
    coef = {k: float(fx[kk]) for kk in fx.files if kk.startswith(case + "/coef/") for k in [kk[len(case) + 6:]]}
    got = {k: float(p.lr_equalization_coef) for k, p in m.named_parameters() if hasattr(p, "lr_equalization_coef")}
    assert got == coef and len(coef) >= 6  # (two linears with biases and two convolutions)
