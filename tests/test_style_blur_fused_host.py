"""CPU-side checks of the blur folded into the style chains (csrc/style.hip's *_blur_* kernels, the `blur=` keyword of
sivae_hip.ops.style_* and sivae_hip.style, blocks.FUSE_BLUR): the new prototypes, their argument validation (every call
returns before any launch), the workspace sizes, the Python surface, and the LDS bound of the decoder backward, which is
read out of the source and held against the query, against ST_MAX_HELD_BWD and against the cases of
tests/test_style_blur_fused_gpu.py."""
import ctypes
import importlib.util
import inspect
import os
import re
import sys

import pytest
import torch

from sivae_hip import lib

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd")
BLOCKS_DIR = os.path.join(PKG, "style_soft_intro_vae")
P, I, F32, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t


@pytest.fixture(scope="module")
def blocks():
    sys.path.insert(0, BLOCKS_DIR)
    try:
        import blocks as B
    finally:
        sys.path.remove(BLOCKS_DIR)
    return B


def source_defines():
    with open(os.path.join(PKG, "csrc", "style.hip")) as f:
        return {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\b", f.read(), re.M)}


# ------------------------------------------------------------------------------------------------ the entry points
def test_prototypes_parse_from_the_header():
    protos = lib.parse_header()
    for plain, fused in (("sivae_style_dec_fwd", "sivae_style_dec_blur_fwd"), ("sivae_style_dec_bwd", "sivae_style_dec_blur_bwd"),
                         ("sivae_style_enc_fwd", "sivae_style_enc_blur_fwd"), ("sivae_style_enc_bwd", "sivae_style_enc_blur_bwd"),
                         ("sivae_style_dec_bwd_workspace_bytes", "sivae_style_dec_blur_bwd_workspace_bytes"),
                         ("sivae_style_enc_bwd_workspace_bytes", "sivae_style_enc_blur_bwd_workspace_bytes")):
        assert protos[fused] == protos[plain], fused  # (the argument conventions of the entry point it stands beside)
    assert protos["sivae_style_dec_blur_fwd"] == (I, [P] * 8 + [I] * 6 + [F32, P])
    assert protos["sivae_style_dec_blur_bwd"] == (I, [P] * 12 + [I] * 6 + [P, SZ, P])
    assert protos["sivae_style_enc_blur_fwd"] == (I, [P] * 5 + [I] * 4 + [F32, P])
    assert protos["sivae_style_enc_blur_bwd"] == (I, [P] * 9 + [I] * 4 + [F32, P, SZ, P])
    assert protos["sivae_style_dec_blur_bwd_fused"] == (I, [I, I])
    text = open(lib.HEADER_PATH).read()
    doc = text[text.index("int sivae_style_blur"):text.index("the style variant's RGB layers")]
    assert text.index("int sivae_style_dec_blur_fwd") > text.index("int sivae_style_blur")  # (behind it, not in its block)
    for said in ("net.py:49-60 with :166-185", "net.py:94-101 with :110", "bit for bit", "UNBLURRED", "its own adjoint",
                 "sivae_style_dec_blur_bwd_fused"):
        assert said in doc, said


def _caller(f, ok):
    def call(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])
    return call


def test_entry_points_validate_arguments():
    """the refusals of the plain entry points, all before any launch (the pointers are not memory)"""
    L = lib.load()
    null, one, odd = None, ctypes.c_void_p(64), ctypes.c_void_p(66)
    shape = dict(B=2, C=3, H=4, W=4)
    dec = _caller(L.sivae_style_dec_blur_fwd, dict(x=one, noise=one, nw=one, bias=one, style=one, y=one, mean=one, rstd=one,
                                                   **shape, mode=1, layer=0, eps=1e-8, stream=null))
    for k in ("x", "bias", "style", "y", "mean", "rstd", "noise", "nw"):
        assert dec(**{k: null}) == -1, k
    assert dec(mode=0, noise=null, nw=null, B=0) == -2
    assert dec(mode=3) == -6 and dec(mode=-1) == -6
    for k in ("B", "C", "H", "W"):
        assert dec(**{k: 0}) == -2 and dec(**{k: -2}) == -2, k
    assert dec(H=1, W=1) == -2 and dec(layer=-1) == -2 and dec(eps=-1.0) == -2 and dec(eps=float("nan")) == -2
    assert dec(B=65536, C=65536) == -5 and dec(H=32768, W=32768) == -5
    assert dec(x=odd) == -2 and dec(y=odd) == -2

    bwd = _caller(L.sivae_style_dec_blur_bwd, dict(dy=one, x=one, noise=one, nw=one, bias=one, style=one, mean=one, rstd=one,
                                                   dx=one, dnw=one, dbias=one, dstyle=one, **shape, mode=1, layer=0, ws=one,
                                                   ws_bytes=1 << 20, stream=null))
    for k in ("dy", "x", "bias", "style", "mean", "rstd", "noise", "nw"):
        assert bwd(**{k: null}) == -1, k
    assert bwd(mode=5) == -6 and bwd(mode=0) == -6
    assert bwd(H=1, W=1) == -2 and bwd(C=0) == -2 and bwd(layer=-3) == -2 and bwd(dx=odd) == -2
    assert bwd(H=32768, W=32768) == -5
    assert bwd(ws=null) == -4 and bwd(ws_bytes=2 * 6 * 8 - 1) == -4 and bwd(dnw=null, ws=null) == -4
    assert bwd(dx=null, dnw=null, dbias=null, dstyle=null, ws=null) == 0   # (nothing asked for: nothing launched)

    enc = _caller(L.sivae_style_enc_blur_fwd, dict(x=one, bias=one, bxn=one, mean=one, std=one, **shape, eps=1e-5,
                                                   stream=null))
    for k in ("x", "bias", "bxn", "mean", "std"):
        assert enc(**{k: null}) == -1, k
    assert enc(H=1, W=1) == -2 and enc(B=-1) == -2 and enc(eps=-1.0) == -2 and enc(B=65536, C=65536) == -5
    assert enc(bxn=odd) == -2

    ebw = _caller(L.sivae_style_enc_blur_bwd, dict(dbxn=one, dmean=one, dstd=one, x=one, bias=one, mean=one, std=one, dx=one,
                                                   dbias=one, **shape, eps=1e-5, ws=one, ws_bytes=1 << 20, stream=null))
    for k in ("x", "bias", "mean", "std"):
        assert ebw(**{k: null}) == -1, k
    assert ebw(H=1, W=1) == -2 and ebw(W=0) == -2 and ebw(dbxn=odd) == -2 and ebw(H=32768, W=32768) == -5
    assert ebw(ws=null) == -4 and ebw(ws_bytes=47) == -4
    assert ebw(dx=null, dbias=null, ws=null) == 0


def test_workspace_sizes_are_what_the_wrappers_allocate(monkeypatch):
    """2 B C and B C doubles, and the wrappers ask ops.workspace for exactly that (the call is stopped there)"""
    from sivae_hip import ops
    L = lib.load()
    assert L.sivae_style_dec_blur_bwd_workspace_bytes(2, 3) == 96 and L.sivae_style_dec_blur_bwd_workspace_bytes(0, 3) == 0
    assert L.sivae_style_enc_blur_bwd_workspace_bytes(2, 3) == 48 and L.sivae_style_enc_blur_bwd_workspace_bytes(2, -1) == 0
    asked = []

    class Stop(Exception):
        pass

    def workspace(nbytes, device):
        asked.append(nbytes)
        raise Stop

    monkeypatch.setattr(ops, "workspace", workspace)
    monkeypatch.setattr(ops, "_style_f32", lambda *a: None)  # (the device check: this test stops before any launch)
    x, b, st, nz, v = torch.zeros(5, 7, 4, 4), torch.zeros(7), torch.zeros(5, 14), torch.zeros(5, 1, 4, 4), torch.zeros(5, 7)
    with pytest.raises(Stop):
        ops.style_dec_bwd(x, x, nz, b, b, st, v, v, 1, blur=True)
    with pytest.raises(Stop):
        ops.style_enc_bwd(x, v, v, x, b, v, v, blur=True)
    assert asked == [L.sivae_style_dec_blur_bwd_workspace_bytes(5, 7), L.sivae_style_enc_blur_bwd_workspace_bytes(5, 7)]
    assert asked == [2 * 35 * 8, 35 * 8]


# ------------------------------------------------------------------------------------------------ the Python surface
def test_wrappers_refuse_cpu_tensors():
    from sivae_hip import ops, style
    x, b, st, nz, v = torch.zeros(2, 3, 4, 4), torch.zeros(3), torch.zeros(2, 6), torch.zeros(2, 1, 4, 4), torch.zeros(2, 3)
    calls = (lambda: ops.style_dec_fwd(x, nz, b, b, st, 1, blur=True), lambda: ops.style_dec_fwd(x, None, None, b, st, 0, blur=True),
             lambda: ops.style_dec_bwd(x, x, nz, b, b, st, v, v, 1, blur=True), lambda: ops.style_enc_fwd(x, b, blur=True),
             lambda: ops.style_enc_bwd(x, v, v, x, b, v, v, blur=True),
             lambda: style.style_layer(x, b, b, st, nz, True, blur=True), lambda: style.style_layer(x, b, b, st, blur=True),
             lambda: style.stat_norm(x, b, blur=True))
    for f in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_the_keyword_goes_last_and_defaults_to_off():
    from sivae_hip import ops, style
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(style.style_layer) == ["x", "noise_weight", "bias", "style", "noise", "mode", "layer", "eps", "blur"]
    assert sig(style.stat_norm) == ["x", "bias", "eps", "blur"]
    assert sig(ops.style_dec_fwd)[:8] == ["x", "noise", "noise_weight", "bias", "style", "mode", "layer", "eps"]
    assert sig(ops.style_dec_bwd)[:14] == ["dy", "x", "noise", "noise_weight", "bias", "style", "mean", "rstd", "mode", "layer",
                                           "want_dx", "want_dnw", "want_dbias", "want_dstyle"]
    assert sig(ops.style_enc_fwd)[:3] == ["x", "bias", "eps"]
    assert sig(ops.style_enc_bwd)[:10] == ["dxn", "dmean", "dstd", "x", "bias", "mean", "std", "eps", "want_dx", "want_dbias"]
    for f in (style.style_layer, style.stat_norm, ops.style_dec_fwd, ops.style_dec_bwd, ops.style_enc_fwd, ops.style_enc_bwd):
        p = inspect.signature(f).parameters
        assert list(p)[-1] == "blur" and p["blur"].default is False, f.__name__
    assert inspect.signature(style.style_layer).parameters["eps"].default == 1e-8
    assert inspect.signature(style.stat_norm).parameters["eps"].default == 1e-5


# ------------------------------------------------------------------------------------------------ the LDS bound
def test_the_lds_bound(blocks):
    from sivae_hip import ops
    d = source_defines()
    bound = d["ST_BLUR_LDS_MAX"]
    assert blocks.FUSE_BLUR_DEC_MAX_HW == bound  # (the decoder's size test is the two-launch class, which measured as a loss)
    assert bound <= d["ST_MAX_HELD_BWD"] and bound % 4 == 0 and 4 * bound <= 64 * 1024
    L = lib.load()
    for H, W, want in ((1, bound, 1), (bound, 1, 1), (1, bound + 1, 0), (2, bound // 2, 1), (2, bound // 2 + 1, 0), (1, 2, 1),
                       (0, 4, 0), (4, -1, 0), (65536, 65536, 0)):
        assert L.sivae_style_dec_blur_bwd_fused(H, W) == want, (H, W)
    assert ops.style_dec_blur_bwd_fused(1, bound) is True and ops.style_dec_blur_bwd_fused(1, bound + 1) is False


def test_the_gpu_cases_stand_on_both_sides_of_the_bound():
    import test_style_blur_fused_gpu as G
    bound = source_defines()["ST_BLUR_LDS_MAX"]
    cases = G.bound_cases(bound)
    hw = {k: c[2] * c[3] for k, c in cases.items()}
    assert hw["at"] == bound, "no plane AT the LDS bound of the decoder backward (%d elements)" % bound
    assert hw["below"] == bound - 1, "no plane just BELOW the LDS bound of the decoder backward"
    assert hw["above"] == bound + 1, "no plane just ABOVE the LDS bound of the decoder backward"
    for k, c in cases.items():
        assert c[3] % 4 != 0 and c[3] >= 1 and c[2] >= 1, "the plane %s the bound has a W that is a multiple of 4" % k
        assert c[2] * c[3] <= max(a[2] * a[3] for a in G.O.CASES + G.O.EDGE_CASES)  # (no larger than the existing lists')


# ------------------------------------------------------------------------------------------------ the blocks
def test_the_switch_follows_the_environment(blocks, monkeypatch):
    """the module read afresh under a private name (the one the other tests hold stays as it is)"""
    def fresh():
        spec = importlib.util.spec_from_file_location("_blocks_fresh", os.path.join(BLOCKS_DIR, "blocks.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        return m.FUSE_BLUR

    monkeypatch.delenv("SIVAE_STYLE_FUSE_BLUR", raising=False)
    assert fresh() is True  # (default: on)
    for value, want in (("1", True), ("0", False), ("", True)):
        monkeypatch.setenv("SIVAE_STYLE_FUSE_BLUR", value)
        assert fresh() is want, value
    assert isinstance(blocks.FUSE_BLUR, bool)


def test_state_dict_keys_are_unchanged(blocks):
    dec = blocks.DecodeBlock(8, 6, 16, True, False, 1)
    assert list(dec.state_dict()) == ["noise_weight_1", "bias_1", "noise_weight_2", "bias_2", "conv_1.weight", "blur.weight",
                                      "style_1.weight", "style_1.bias", "conv_2.weight", "style_2.weight", "style_2.bias"]
    enc = blocks.EncodeBlock(6, 8, 16, False, False)
    assert list(enc.state_dict()) == ["bias_1", "bias_2", "conv_1.weight", "blur.weight", "conv_2.weight", "style_1.weight",
                                      "style_1.bias", "style_2.weight", "style_2.bias"]
    assert tuple(dec.blur.weight.shape) == (6, 1, 3, 3) and tuple(enc.blur.weight.shape) == (6, 1, 3, 3)
    assert isinstance(dec.blur, blocks.Blur) and isinstance(enc.blur, blocks.Blur)


def test_the_fused_calls_keep_their_shape(blocks, monkeypatch):
    """what the blocks pass to style.style_layer / stat_norm with the switch on and off, recorded by spies that stop the
    call (CPU tensors: nothing is launched)"""
    from sivae_hip import style

    class Stop(Exception):
        pass

    seen = []

    def spy(name):
        def call(*a, **kw):
            seen.append((name, len(a), dict(kw)))
            raise Stop
        return call

    monkeypatch.setattr(style, "style_layer", spy("style_layer"))
    monkeypatch.setattr(style, "stat_norm", spy("stat_norm"))
    monkeypatch.setattr(style, "blur", spy("blur"))
    # (neither the convolution, 4 -> 4 channels, nor the style's linear is the point; both refuse CPU tensors)
    monkeypatch.setattr(blocks._Conv3x3, "forward", lambda self, x: x)
    monkeypatch.setattr(blocks._Linear, "forward", lambda self, x: x)
    dec, enc = blocks.DecodeBlock(4, 4, 8, True, False), blocks.EncodeBlock(4, 4, 8, False, False)
    x, s = torch.zeros(1, 4, 4, 4), torch.zeros(1, 8)
    for on, want in ((True, [("style_layer", 7, {"blur": True}), ("stat_norm", 2, {"blur": True})]),
                     (False, [("blur", 1, {}), ("stat_norm", 2, {})])):
        monkeypatch.setattr(blocks, "FUSE_BLUR", on)
        del seen[:]
        for run in (lambda: dec(x, s, s, True), lambda: enc(x)):
            with pytest.raises(Stop):
                run()
        assert seen == want, (on, seen)
