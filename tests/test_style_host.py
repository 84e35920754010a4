"""CPU-side checks of the style variant's layers (csrc/style.hip, sivae_hip.ops.style_*, sivae_hip.style,
style_soft_intro_vae/blocks.py): the float64 oracle tests/style_oracle.py against the fixture recorded from the
reference's net.py (tests/golden/style_blocks.npz), the blocks' constructors against the fixture's state dicts, the
argument validation of the five entry points (every call returns before any launch) and the Python surface."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import style_oracle as O
from sivae_hip import lib

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS_DIR = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd", "style_soft_intro_vae")
CASES = ("dec_per_sample", "dec_batch_constant", "dec_no_noise", "dec_no_first_conv", "enc", "enc_last")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "style_blocks.npz"))


@pytest.fixture(scope="module")
def blocks():
    sys.path.insert(0, BLOCKS_DIR)
    try:
        import blocks as B
    finally:
        sys.path.remove(BLOCKS_DIR)
    return B


def group(fx, prefix):
    """{key without the prefix: tensor}, in the fixture's order"""
    return {k[len(prefix):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(prefix)}


def oracle_run(fx, case):
    """the oracle on the fixture's inputs -> (outputs, {name: gradient}) in float64"""
    meta = json.loads(str(fx[case + "/meta"]))
    P = {k: v.clone().requires_grad_(True) for k, v in group(fx, case + "/param/").items() if k != "blur.weight"}
    ins = {k: v.clone().requires_grad_(True) for k, v in group(fx, case + "/in/").items()}
    kw = meta["kwargs"]
    if meta["block"] == "DecodeBlock":
        noises = [torch.from_numpy(fx["%s/noise%d" % (case, i)]) for i in range(2)] if meta["noise"] else None
        outs = (O.decode_block(P, ins["x"], ins["s1"], ins["s2"], meta["noise"], noises, kw["has_first_conv"],
                               kw["fused_scale"], kw["layer"]),)
    else:
        outs = O.encode_block(P, ins["x"], kw["last"], kw["fused_scale"])
    sum((o * torch.from_numpy(fx["%s/g%d" % (case, i)])).sum() for i, o in enumerate(outs)).backward()
    grads = {k: v.grad for k, v in list(ins.items()) + list(P.items()) if v.grad is not None}
    return [o.detach() for o in outs], grads


@pytest.mark.parametrize("case", CASES)
def test_oracle_reproduces_the_reference(fx, case):
    outs, grads = oracle_run(fx, case)
    worst = max(O.nerr(o, torch.from_numpy(fx["%s/out%d" % (case, i)])) for i, o in enumerate(outs))
    want = group(fx, case + "/grad/")
    assert set(grads) == set(want), (sorted(grads), sorted(want))
    for k, v in want.items():
        assert float(v.abs().max()) > 0, k  # (every recorded gradient says something)
        worst = max(worst, O.nerr(grads[k], v))
    print("%s: oracle against the reference, worst relative error %.3e" % (case, worst))
    assert worst <= 1e-12


def test_fixture_covers_what_it_should(fx):
    for case in CASES:
        meta = json.loads(str(fx[case + "/meta"]))
        P, G = group(fx, case + "/param/"), group(fx, case + "/grad/")
        for k, v in P.items():
            if k.startswith(("noise_weight_", "bias_")):
                assert float(v.abs().min()) > 0, (case, k)
        if meta["block"] == "DecodeBlock":
            assert {"x", "s1", "s2", "bias_1", "bias_2", "conv_2.weight", "style_1.weight", "style_2.bias"} <= set(G)
            assert ("noise_weight_1" in G) == bool(meta["noise"]) and ("noise_weight_2" in G) == bool(meta["noise"])
            assert ("conv_1.weight" in P) == meta["kwargs"]["has_first_conv"]
            if meta["noise"]:
                n0, n1 = fx[case + "/noise0"], fx[case + "/noise1"]
                assert n0.shape == n1.shape == ((1 if meta["noise"] == "batch_constant" else 2), 1) + fx[case + "/out0"].shape[2:]
                assert not np.array_equal(n0, n1)
        else:
            assert {"x", "bias_1", "conv_1.weight", "style_1.weight", "style_2.weight"} <= set(G)
            assert ("dense.weight" in P) == meta["kwargs"]["last"] and ("conv_2.weight" in P) != meta["kwargs"]["last"]


def test_oracle_ops_agree_with_torch_modules():
    """the restated ops against torch's own InstanceNorm2d / LeakyReLU / conv2d on one odd shape"""
    d = O.dec_inputs((3, 5, 5, 7), 1)
    C = 5
    t = torch.nn.functional.leaky_relu(d["x"] + d["noise_weight"].view(1, C, 1, 1) * d["noise"] + d["bias"].view(1, C, 1, 1), 0.2)
    st = d["style"].view(3, 2, C, 1, 1)
    ref = torch.addcmul(st[:, 1], torch.nn.InstanceNorm2d(C, eps=1e-8).double()(t), st[:, 0] + 1)
    assert O.nerr(O.style_layer(d["x"], d["noise_weight"], d["bias"], d["style"], d["noise"], 1), ref) <= 1e-14
    e = O.enc_inputs((3, 5, 5, 7))
    t = torch.nn.functional.leaky_relu(e["x"] + e["bias"].view(1, C, 1, 1), 0.2)
    xn, m, std = O.stat_norm(e["x"], e["bias"])
    assert O.nerr(xn, torch.nn.InstanceNorm2d(C).double()(t)) <= 1e-14
    assert O.nerr(m, t.mean((2, 3))) <= 1e-15 and O.nerr(std, t.var((2, 3), unbiased=False).sqrt()) <= 1e-14


# ------------------------------------------------------------------------------------------------ the blocks' constructors
@pytest.mark.parametrize("case", CASES)
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
    assert got == coef and len(coef) >= 5  # (two linears with biases and at least one convolution)
    assert "blur.weight" in sd and "blur.weight" not in dict(m.named_parameters())
    # positional arguments as the reference's networks pass them
    args = list(meta["kwargs"].values())
    torch.manual_seed(0)
    assert all(torch.equal(a, b) for a, b in zip(cls(*args).state_dict().values(),
                                                 group(fx, case + "/init0/").values()))


def test_blocks_surface(blocks):
    import inspect
    for name in ("Blur", "EncodeBlock", "DecodeBlock", "style_mod", "pixel_norm", "upscale2d", "downscale2d"):
        assert hasattr(blocks, name), name
    assert list(inspect.signature(blocks.DecodeBlock.forward).parameters) == ["self", "x", "s1", "s2", "noise"]
    assert list(inspect.signature(blocks.EncodeBlock.forward).parameters) == ["self", "x"]
    assert list(inspect.signature(blocks.DecodeBlock.__init__).parameters) == [
        "self", "inputs", "outputs", "latent_size", "has_first_conv", "fused_scale", "layer"]
    assert list(inspect.signature(blocks.EncodeBlock.__init__).parameters) == [
        "self", "inputs", "outputs", "latent_size", "last", "fused_scale"]
    x = torch.randn(2, 3, 4, 6, dtype=torch.float64)
    st = torch.randn(2, 6, dtype=torch.float64)
    assert torch.equal(blocks.upscale2d(x), x.reshape(2, 3, 4, 1, 6, 1).repeat(1, 1, 1, 2, 1, 2).reshape(2, 3, 8, 12))
    assert torch.equal(blocks.downscale2d(x), torch.nn.functional.avg_pool2d(x, 2, 2))
    assert O.nerr(blocks.style_mod(x, st), x * (st[:, :3, None, None] + 1) + st[:, 3:, None, None]) <= 1e-15
    assert O.nerr(blocks.pixel_norm(x), x / torch.sqrt((x * x).mean(1, keepdim=True) + 1e-8)) <= 1e-15
    m = blocks.DecodeBlock(4, 4, 8, True, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, 4, 4), torch.zeros(1, 8), torch.zeros(1, 8), True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        blocks.EncodeBlock(4, 4, 8, False, False)(torch.zeros(1, 4, 8, 8))


# ------------------------------------------------------------------------------------------------ the entry points
P, I, F32, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t


def test_prototypes_parse_from_the_header():
    protos = lib.parse_header()
    assert protos["sivae_style_dec_fwd"] == (I, [P] * 8 + [I] * 6 + [F32, P])
    assert protos["sivae_style_dec_bwd"] == (I, [P] * 12 + [I] * 6 + [P, SZ, P])
    assert protos["sivae_style_enc_fwd"] == (I, [P] * 5 + [I] * 4 + [F32, P])
    assert protos["sivae_style_enc_bwd"] == (I, [P] * 9 + [I] * 4 + [F32, P, SZ, P])
    assert protos["sivae_style_blur"] == (I, [P, P, I, I, I, I, P])
    assert protos["sivae_style_dec_bwd_workspace_bytes"] == (SZ, [I, I])
    assert protos["sivae_style_enc_bwd_workspace_bytes"] == (SZ, [I, I])
    text = open(lib.HEADER_PATH).read()
    doc = text[text.index("the style variant's non-conv layers"):text.index("int sivae_style_blur")]
    for said in ("net.py:169-185", "net.py:94-101", "net.py:49-60", "No atomics", "bit-identical", "DROPS the dstd term",
                 "'batch_constant'", "its own adjoint"):
        assert said in doc, said


def _caller(f, ok):
    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])
    return call


def test_entry_points_validate_arguments():
    """null pointers, H W < 2, non-positive sizes, a bad mode, sizes beyond 32-bit plane counts, pointers that are not
    4-byte aligned, a missing workspace: the documented codes, all before any launch (the pointers are not memory)"""
    L = lib.load()
    null, one, odd = None, ctypes.c_void_p(64), ctypes.c_void_p(66)
    shape = dict(B=2, C=3, H=4, W=4)
    dec = _caller(L.sivae_style_dec_fwd, dict(x=one, noise=one, nw=one, bias=one, style=one, y=one, mean=one, rstd=one,
                                              **shape, mode=1, layer=0, eps=1e-8, stream=null))
    for k in ("x", "bias", "style", "y", "mean", "rstd", "noise", "nw"):
        assert dec(**{k: null}) == -1, k
    assert dec(mode=0, noise=null, nw=null, B=0) == -2   # (mode 0 needs neither; the refusal is the shape's)
    assert dec(mode=3) == -6 and dec(mode=-1) == -6
    for k in ("B", "C", "H", "W"):
        assert dec(**{k: 0}) == -2 and dec(**{k: -2}) == -2, k
    assert dec(H=1, W=1) == -2 and dec(H=1, W=2, B=0) == -2
    assert dec(layer=-1) == -2 and dec(eps=-1.0) == -2 and dec(eps=float("nan")) == -2
    assert dec(B=65536, C=65536) == -5 and dec(H=32768, W=32768) == -5
    assert dec(x=odd) == -2 and dec(y=odd) == -2

    bwd = _caller(L.sivae_style_dec_bwd, dict(dy=one, x=one, noise=one, nw=one, bias=one, style=one, mean=one, rstd=one,
                                              dx=one, dnw=one, dbias=one, dstyle=one, **shape, mode=1, layer=0, ws=one,
                                              ws_bytes=1 << 20, stream=null))
    for k in ("dy", "x", "bias", "style", "mean", "rstd", "noise", "nw"):
        assert bwd(**{k: null}) == -1, k
    assert bwd(mode=5) == -6 and bwd(mode=0) == -6       # (mode 0 with a dnoise_weight)
    assert bwd(H=1, W=1) == -2 and bwd(C=0) == -2 and bwd(layer=-3) == -2 and bwd(dx=odd) == -2
    assert bwd(ws=null) == -4 and bwd(ws_bytes=2 * 6 * 8 - 1) == -4 and bwd(dnw=null, ws=null) == -4
    assert bwd(dx=null, dnw=null, dbias=null, dstyle=null, ws=null) == 0   # (nothing asked for: nothing launched)
    assert L.sivae_style_dec_bwd_workspace_bytes(2, 3) == 96 and L.sivae_style_dec_bwd_workspace_bytes(0, 3) == 0

    enc = _caller(L.sivae_style_enc_fwd, dict(x=one, bias=one, xn=one, mean=one, std=one, **shape, eps=1e-5, stream=null))
    for k in ("x", "bias", "xn", "mean", "std"):
        assert enc(**{k: null}) == -1, k
    assert enc(H=1, W=1) == -2 and enc(B=-1) == -2 and enc(eps=-1.0) == -2 and enc(B=65536, C=65536) == -5

    ebw = _caller(L.sivae_style_enc_bwd, dict(dxn=one, dmean=one, dstd=one, x=one, bias=one, mean=one, std=one, dx=one,
                                              dbias=one, **shape, eps=1e-5, ws=one, ws_bytes=1 << 20, stream=null))
    for k in ("x", "bias", "mean", "std"):
        assert ebw(**{k: null}) == -1, k
    assert ebw(H=1, W=1) == -2 and ebw(W=0) == -2 and ebw(dxn=odd) == -2
    assert ebw(ws=null) == -4 and ebw(ws_bytes=47) == -4
    assert ebw(dx=null, dbias=null, ws=null) == 0
    assert L.sivae_style_enc_bwd_workspace_bytes(2, 3) == 48

    blur = _caller(L.sivae_style_blur, dict(x=one, y=one, **shape, stream=null))
    assert blur(x=null) == -1 and blur(y=null) == -1 and blur(H=0) == -2 and blur(B=-1) == -2 and blur(y=odd) == -2
    assert L.sivae_abi_version() == 1


# ------------------------------------------------------------------------------------------------ the Python surface
def test_wrappers_refuse_cpu_tensors():
    from sivae_hip import ops, style
    x, b, st, nz, v = torch.zeros(2, 3, 4, 4), torch.zeros(3), torch.zeros(2, 6), torch.zeros(2, 1, 4, 4), torch.zeros(2, 3)
    calls = (lambda: ops.style_dec_fwd(x, nz, b, b, st, 1), lambda: ops.style_dec_fwd(x, None, None, b, st, 0),
             lambda: ops.style_dec_bwd(x, x, nz, b, b, st, v, v, 1), lambda: ops.style_enc_fwd(x, b),
             lambda: ops.style_enc_bwd(x, v, v, x, b, v, v), lambda: ops.style_blur(x),
             lambda: style.style_layer(x, b, b, st, nz, True), lambda: style.style_layer(x, b, b, st),
             lambda: style.stat_norm(x, b), lambda: style.blur(x))
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()
    for fn in (style.StyleLayerFn, style.StatNormFn, style.BlurFn):
        assert issubclass(fn, torch.autograd.Function)
    assert [style.noise_mode(m) for m in (None, False, 0, True, "per_sample", "anything", "batch_constant", 2)] == \
        [0, 0, 0, 1, 1, 1, 2, 2]
    with pytest.raises(ValueError, match="needs the noise tensor"):
        style.style_layer(x, b, b, st, None, True)
