"""CPU-side checks of the style variant's network classes (style_soft_intro_vae/net.py) and RGB-layer entry points: the
drop-in surface against the fixture recorded from the reference (tests/golden/style_net.npz), the oracle
(tests/style_rgb_oracle.py) against the fixture's RGB-layer sub-results, the check inputs' distance from the activation's
kink, and the argument validation of the C entry points and of sivae_hip.ops.style_*rgb* (no launch happens)."""
import ctypes
import hashlib
import inspect

import numpy as np
import pytest
import torch

import style_net_fixture as X
import style_rgb_oracle as R

CLASSES = list(X.ENCODERS) + ["Generator"] + X.MAPPING_CASES


@pytest.fixture(scope="module")
def fx():
    return X.Fixture()


@pytest.fixture(scope="module")
def net():
    return X.import_net()


def test_fixture_is_smaller_than_the_largest_committed_one():
    import os
    gold = os.path.join(X.HERE, "golden")
    assert os.path.getsize(os.path.join(gold, "style_net.npz")) < os.path.getsize(os.path.join(gold, "lreq_adam.npz"))


def test_names_registries_and_signatures(fx, net):
    names = fx.json("names")
    for reg, entries in names["registries"].items():
        have = getattr(net, reg)
        for key, cls in entries.items():
            assert have[key].__name__ == cls and have[key] is getattr(net, cls), (reg, key)
    for cls, sig in names["signatures"].items():
        c = getattr(net, cls)
        assert str(inspect.signature(c.__init__)) == sig["init"], cls
        assert str(inspect.signature(c.forward)) == sig["forward"], cls
    for name in ("torch", "nn", "F", "MAPPINGS", "GENERATORS", "ENCODERS", "Blur", "EncodeBlock", "DecodeBlock"):
        assert hasattr(net, name), name  # (what model.py reaches through `from net import *`)
    assert net.torch is torch and not any(k.startswith("DCGAN") for r in ("ENCODERS", "GENERATORS") for k in getattr(net, r))


@pytest.mark.parametrize("cls", CLASSES)
def test_constructor_reproduces_the_reference(fx, net, cls):
    """state dict bit for bit per seed in the recorded key order, every lr_equalization_coef and .std"""
    keys = fx.json(cls + "/keys")
    for seed in (0, 1):
        torch.manual_seed(seed)
        m = X.make(net, cls, fx)
        sd = m.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == keys
        flat = np.concatenate([v.numpy().ravel() for v in sd.values()])
        assert flat.dtype == np.float32
        if seed == 0:
            assert np.array_equal(flat, fx[cls + "/init0"])
        else:
            assert hashlib.sha256(flat.tobytes()).hexdigest() == fx[cls + "/init1_sha256"]
    coef = {k: float(p.lr_equalization_coef) for k, p in m.named_parameters() if hasattr(p, "lr_equalization_coef")}
    assert coef == fx.json(cls + "/coef")
    std = {k: float(mod.std) for k, mod in m.named_modules() if isinstance(getattr(mod, "std", None), (float, np.floating))}
    assert std == fx.json(cls + "/std")


def test_statistics_and_attributes(net):
    torch.manual_seed(0)
    g, e = net.Generator(**X.CFG), net.Encoder_old(**X.CFG)
    assert g.layer_to_resolution == [4, 8, 16] and g.style_sizes == [16, 16, 16, 16, 16, 8]
    for m in (g, e):
        rgb, layers = m.get_statistics(1)
        assert rgb > 0 and len(layers) == 2 and all(len(p) == 2 and p[1] > 0 for p in layers)
    assert g.get_statistics(0)[1][0][0] == 1.0  # (the first block has no first convolution)


@pytest.mark.parametrize("run", X.RUNS)
def test_oracle_reproduces_the_reference_rgb_layers(fx, run):
    """the float64 restatement of the header's formulas against what the reference's net.py computed around its RGB
    layers (to_rgb / interpolate / lerp in the generator; from_rgb / leaky_relu / avg_pool2d / lerp in the encoder)"""
    meta = fx.json("Generator/%s/meta" % run)
    lod, blend = meta["lod"], meta["blend"]
    P = fx.state("Generator")
    w, b = P["to_rgb.%d.to_rgb.weight" % lod].flatten(1), P["to_rgb.%d.to_rgb.bias" % lod]
    pre = "Generator/%s/rgb/" % run
    prev = fx.tensor(pre + "prev") if blend != 1 else None
    assert (pre + "prev" in fx) == (blend != 1)
    y = R.to_rgb(fx.tensor(pre + "x"), w, b, prev, blend)
    assert R.nerr(y, fx.tensor(pre + "y")) <= 1e-13
    assert R.nerr(fx.tensor(pre + "y"), fx.tensor("Generator/%s/out0" % run)[:1]) <= 2.0 ** -23  # (out0 is stored as float32)
    P = fx.state("Encoder")
    first = X.CFG["layer_count"] - lod - 1
    img = fx.tensor("encoders/%s/in/x" % run)[:1]
    pre = "Encoder/%s/rgb/" % run
    if blend == 1:
        w, b = P["from_rgb.%d.from_rgb.weight" % first].flatten(1), P["from_rgb.%d.from_rgb.bias" % first]
        y = R.from_rgb(img, w, b)
    else:
        w, b = P["from_rgb.%d.from_rgb.weight" % (first + 1)].flatten(1), P["from_rgb.%d.from_rgb.bias" % (first + 1)]
        y = R.from_rgb(img, w, b, True, fx.tensor(pre + "other"), blend)
    assert R.nerr(y, fx.tensor(pre + "y")) <= 1e-13


def test_oracle_lerp_is_torchs():
    g = torch.Generator().manual_seed(3)
    a, b = (torch.randn(64, generator=g, dtype=torch.float64) for _ in range(2))
    for w in (0.0, 0.25, 0.49, 0.5, 0.75, 1.0):
        assert R.nerr(R.lerp(a, b, w), torch.lerp(a, b, w)) <= 1e-15, w  # (torch may fuse the multiply-add)
    p = torch.randn(2, 3, 3, 5, generator=g, dtype=torch.float64)
    assert torch.equal(R.up2(p), torch.nn.functional.interpolate(p, size=(6, 10)))
    assert R.nerr(R.avg2(R.up2(p)), p) <= 1e-15
    assert R.nerr(R.avg2(R.up2(p) + 0), torch.nn.functional.avg_pool2d(R.up2(p), 2, 2)) <= 1e-15


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_check_inputs_stay_away_from_the_kink(case):
    """every pre-activation of every from_rgb check keeps 2^-18 of the sum of its terms' magnitudes away from 0, and the
    inputs are exact in float32"""
    assert R.variants(case) == ((None,) + R.BLENDS if case[2] % 2 == 0 and case[3] % 2 == 0 else (None,))
    for blend in R.variants(case):
        d = R.from_inputs(case, blend)
        assert R.kink_margin(d) >= R.KINK_MARGIN and d["seed"] < 4
        for t in list(d.values()) + list(R.to_inputs(case, blend).values()):
            if isinstance(t, torch.Tensor):
                assert t.dtype == torch.float64 and torch.equal(t.float().double(), t)


def test_rgb_entry_points_validate_arguments():
    """documented codes, before any launch (the pointers are never dereferenced)"""
    from sivae_hip import lib
    L = lib.load()
    null, one, odd = None, ctypes.c_void_p(16), ctypes.c_void_p(18)
    tf, tb, ff, fb = L.sivae_to_rgb_fwd, L.sivae_to_rgb_bwd, L.sivae_from_rgb_fwd, L.sivae_from_rgb_bwd
    big = 1 << 30
    # to_rgb forward: x, w, bias, prev, blend, y, B, C, H, W, K
    assert tf(null, one, one, null, 1.0, one, 1, 4, 4, 4, 3, null) == -1
    assert tf(one, one, one, null, 1.0, null, 1, 4, 4, 4, 3, null) == -1
    assert tf(one, one, one, null, 1.0, one, 1, 4, 4, 4, 0, null) == -2 and tf(one, one, one, null, 1.0, one, 1, 4, 4, 4, 5, null) == -2
    assert tf(one, one, one, null, 1.0, one, 0, 4, 4, 4, 3, null) == -2
    assert tf(one, one, one, one, 0.5, one, 1, 4, 5, 4, 3, null) == -2 and tf(one, one, one, one, 0.5, one, 1, 4, 4, 3, 3, null) == -2
    assert tf(one, one, one, null, 1.0, odd, 1, 4, 4, 4, 3, null) == -2           # 4-byte alignment
    assert tf(one, one, one, null, 1.0, one, 70000, 4, 4, 4, 3, null) == -5
    # to_rgb backward: dy, x, w, has_prev, blend, dx, dw, dbias, dprev, B, C, H, W, K, workspace, bytes
    need = L.sivae_to_rgb_bwd_workspace_bytes(2, 5, 6, 10, 3)
    assert need == (5 + 1) * 2 * 1 * 4 * 4 and L.sivae_to_rgb_bwd_workspace_bytes(2, 5, 6, 10, 5) == 0
    assert L.sivae_to_rgb_bwd_workspace_bytes(1, 64, 256, 256, 3) == 65 * 256 * 16
    assert tb(null, one, one, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 3, one, big, null) == -1
    assert tb(one, null, one, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 3, one, big, null) == -1   # dw needs x
    assert tb(one, one, one, 2, 1.0, one, one, one, null, 2, 5, 6, 10, 3, one, big, null) == -6
    assert tb(one, one, one, 0, 1.0, one, one, one, one, 2, 5, 6, 10, 3, one, big, null) == -6     # dprev without prev
    assert tb(one, one, one, 1, 0.5, one, one, one, one, 2, 5, 5, 10, 3, one, big, null) == -2     # odd H with prev
    assert tb(one, one, one, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 6, one, big, null) == -2
    assert tb(one, one, one, 0, 1.0, one, one, null, null, 2, 5, 6, 10, 3, null, 0, null) == -4
    assert tb(one, one, one, 0, 1.0, one, null, one, null, 2, 5, 6, 10, 3, one, need - 1, null) == -4
    assert tb(one, one, one, 0, 1.0, null, null, null, null, 2, 5, 6, 10, 3, null, 0, null) == 0   # nothing asked for
    # from_rgb forward: img, w, bias, pool, other, blend, y, B, C, H, W, K
    assert ff(one, null, one, 0, null, 1.0, one, 1, 4, 4, 4, 3, null) == -1
    assert ff(one, one, one, 2, null, 1.0, one, 1, 4, 4, 4, 3, null) == -6
    assert ff(one, one, one, 1, one, 0.5, one, 1, 4, 4, 6, 3 + 2, null) == -2
    assert ff(one, one, one, 1, one, 0.5, one, 1, 4, 3, 6, 3, null) == -2 and ff(one, one, one, 1, null, 1.0, one, 1, 4, 4, 7, 3, null) == -2
    assert ff(one, one, one, 0, null, 1.0, one, 1, 0, 4, 4, 3, null) == -2
    # from_rgb backward: dy, img, w, bias, pool, has_other, blend, dimg, dw, dbias, dother, B, C, H, W, K, workspace, bytes
    wb = L.sivae_from_rgb_bwd_workspace_bytes
    assert wb(2, 5, 6, 10, 3, 0) == 5 * 2 * 4 * 4 and wb(2, 5, 6, 10, 4, 1) == 5 * 2 * 8 * 4 and wb(2, 5, 5, 10, 3, 1) == 0
    assert wb(1, 64, 512, 512, 3, 1) == wb(1, 64, 256, 256, 3, 0) == 64 * 256 * 16
    assert fb(one, null, one, one, 0, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 3, one, big, null) == -1
    assert fb(one, one, one, null, 0, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 3, one, big, null) == -1
    assert fb(one, one, one, one, 0, 3, 1.0, one, one, one, null, 2, 5, 6, 10, 3, one, big, null) == -6
    assert fb(one, one, one, one, 0, 0, 1.0, one, one, one, one, 2, 5, 6, 10, 3, one, big, null) == -6    # dother without other
    assert fb(one, one, one, one, 1, 1, 0.5, one, one, one, one, 2, 5, 6, 9, 3, one, big, null) == -2     # odd W with pooling
    assert fb(one, one, one, one, 0, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 0, one, big, null) == -2
    assert fb(one, one, one, one, 0, 0, 1.0, one, one, null, null, 2, 5, 6, 10, 3, null, 0, null) == -4
    assert fb(one, one, one, one, 0, 0, 1.0, one, null, one, null, 2, 5, 6, 10, 3, one, wb(2, 5, 6, 10, 3, 0) - 1, null) == -4
    assert fb(one, one, one, one, 0, 0, 1.0, one, one, one, null, 2, 5, 6, 10, 3, odd, big, null) == -4   # 16-byte aligned
    assert fb(one, one, one, one, 0, 0, 1.0, null, null, null, null, 2, 5, 6, 10, 3, null, 0, null) == 0


def test_ops_refuse_cpu_tensors_wrong_dtypes_and_k5():
    from sivae_hip import ops, style
    x, w, b = torch.zeros(1, 4, 4, 4), torch.zeros(3, 4), torch.zeros(3)
    img, wf, bf = torch.zeros(1, 3, 4, 4), torch.zeros(4, 3), torch.zeros(4)
    calls = {"to_fwd": lambda c: ops.style_to_rgb_fwd(c(x), c(w), c(b)),
             "to_bwd": lambda c: ops.style_to_rgb_bwd(c(img), c(x), c(w)),
             "from_fwd": lambda c: ops.style_from_rgb_fwd(c(img), c(wf), c(bf)),
             "from_bwd": lambda c: ops.style_from_rgb_bwd(c(x), c(img), c(wf), c(bf))}
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="ROCm device"):
            call(lambda t: t)
        with pytest.raises(TypeError, match="float32"):
            call(lambda t: t.double())
        with pytest.raises(TypeError, match="float32"):
            call(lambda t: t.half())
    with pytest.raises(RuntimeError, match="ROCm device"):
        style.to_rgb(x, w.view(3, 4, 1, 1), b)
    with pytest.raises(RuntimeError, match="ROCm device"):
        style.from_rgb(img, wf.view(4, 3, 1, 1), bf, pool=True)
    with pytest.raises(ValueError, match="K <= 4"):
        ops.style_to_rgb_fwd(x, torch.zeros(5, 4), torch.zeros(5))
    with pytest.raises(ValueError, match="K <= 4"):
        ops.style_to_rgb_bwd(torch.zeros(1, 5, 4, 4), x, torch.zeros(5, 4))
    with pytest.raises(ValueError, match="K <= 4"):
        ops.style_from_rgb_fwd(torch.zeros(1, 5, 4, 4), torch.zeros(4, 5), bf)
    with pytest.raises(ValueError, match="K <= 4"):
        ops.style_from_rgb_bwd(x, torch.zeros(1, 5, 4, 4), torch.zeros(4, 5), bf)
    with pytest.raises(ValueError, match="even"):
        ops.style_from_rgb_fwd(torch.zeros(1, 3, 5, 4), wf, bf, pool=True)
