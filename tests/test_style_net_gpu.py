"""GPU checks of the style variant's RGB layers and network classes: the kernels of csrc/rgb.hip through
sivae_hip.ops.style_*rgb*, the autograd Functions sivae_hip.style.to_rgb / from_rgb and the drop-in classes of
style_soft_intro_vae/net.py, against the float64 oracle tests/style_rgb_oracle.py and the fixture recorded from the
reference (tests/golden/style_net.npz).

Tolerances.  Forward outputs: the project's element-wise criterion |a - ref| <= 1e-4 |ref| + 1e-5 max |ref| (O.viol).
Gradients of the ops: the normalised error O.nerr is held to GRAD_GATE, which comes from what a float32 torch restatement
of the same formulas loses on the CPU against the float64 one over the same cases and the edge cases of
tests/test_style_edges_gpu.py (O.CASES and O.EDGE_CASES), NOT from the kernels' own error:

    cd tests && python style_rgb_oracle.py
    float32 restatement vs float64 over CASES and EDGE_CASES: forward 3.115e-07, gradients 1.286e-06

The gate is 4 x that figure for the different summation order of a parallel reduction, and never looser than 1e-4.
Classes chain convolutions, blocks and these layers: their gradients are held to the project's fp32 figure 1e-4
(test_e2e_gpu.TOL, test_style_gpu.BLOCK_GRAD_GATE)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import style_net_fixture as X
import style_rgb_oracle as O

pytestmark = pytest.mark.gpu

FP32_GRAD_LOSS = 1.286e-06                      # measured, see above
GRAD_GATE = min(4 * FP32_GRAD_LOSS, 1e-4)       # = 5.144e-06
CLASS_GRAD_GATE = 1e-4
DEV = "cuda:0"
VARIANTS = [(c, b) for c in O.CASES for b in O.variants(c)]
VID = lambda v: "%s-%s" % (O.case_id(v[0]), "plain" if v[1] is None else "blend%s" % v[1])  # noqa: E731
TO_KEYS, FROM_KEYS = ("y",) + O.TO_GRADS, ("y",) + O.FROM_GRADS


def put(t):
    return None if t is None else t.float().to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def to_case(case, blend):
    """(inputs, float64 reference), computed once and shared"""
    d = O.to_inputs(case, blend)
    return d, O.to_reference(d)


@functools.lru_cache(maxsize=None)
def from_case(case, blend):
    d = O.from_inputs(case, blend)
    return d, O.from_reference(d)


def run_to(d, wants=(True, True, True, True), place=put):
    from sivae_hip import ops
    x, w, b, p, g = (place(d[k]) for k in ("x", "w", "bias", "prev", "g"))
    blend = 1.0 if d["blend"] is None else d["blend"]
    y = ops.style_to_rgb_fwd(x, w, b, p, blend)
    return dict(zip(TO_KEYS, (y,) + ops.style_to_rgb_bwd(g, x, w, p is not None, blend, *wants)))


def run_from(d, wants=(True, True, True, True), place=put):
    from sivae_hip import ops
    img, w, b, o, g = (place(d[k]) for k in ("img", "w", "bias", "other", "g"))
    blend, pool = (1.0, False) if d["blend"] is None else (d["blend"], True)
    y = ops.style_from_rgb_fwd(img, w, b, pool, o, blend)
    return dict(zip(FROM_KEYS, (y,) + ops.style_from_rgb_bwd(g, img, w, b, pool, o is not None, blend, *wants)))


RUN = {"to": (to_case, run_to, TO_KEYS, ("x", "w", "bias", "prev", "g")),
       "from": (from_case, run_from, FROM_KEYS, ("img", "w", "bias", "other", "g"))}


def same(a, b, keys, what=""):
    for k in keys:
        if b[k] is None:
            assert a[k] is None, (what, k)
        else:
            assert torch.equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------ the ops against the oracle
@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", VARIANTS, ids=VID)
def test_ops_against_the_oracle(variant, op):
    case_fn, run, keys, _ = RUN[op]
    d, ref = case_fn(*variant)
    got = run(d)
    v = O.viol(got["y"], ref["y"])
    errs = {k: O.nerr(got[k], ref[k]) for k in keys[1:] if ref[k] is not None}
    print("%s_rgb %s: y %.3f of the criterion; %s (gate %.2e)"
          % (op, VID(variant), v, ", ".join("%s %.2e" % kv for kv in errs.items()), GRAD_GATE))
    assert v <= 1.0
    for k in keys[1:]:
        assert (got[k] is None) == (ref[k] is None), k
        assert got[k] is None or got[k].shape == ref[k].shape, k
    for k, e in errs.items():
        assert e <= GRAD_GATE, (k, e)


# ------------------------------------------------------------------------------------------------ bit-identity
ALIGN_VARIANTS = [((3, 5, 6, 10, 3), 0.25), ((2, 16, 8, 8, 3), None), ((2, 16, 8, 8, 3), 0.75), ((1, 2, 128, 128, 4), 0.25)]


@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", ALIGN_VARIANTS, ids=VID)
def test_alignment_changes_no_bit(variant, op):
    """every output with each input in turn one, two and three elements behind a 512-byte aligned base (the scalar
    instantiation), the others staying aligned, against all of them aligned (the 16-byte one where H W allows)"""
    case_fn, run, keys, names = RUN[op]
    d, _ = case_fn(*variant)
    base = run(d)

    def shifted(t, off):
        buf = torch.empty(t.numel() + off, dtype=torch.float32, device=DEV)
        v = buf[off:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
        return v

    for name in names:
        if d[name] is None:
            continue
        for off in (1, 2, 3):
            moved = {k: (shifted(put(v), off) if k == name else v) for k, v in d.items()}
            got = run(moved, place=lambda t: None if t is None else (t if t.is_cuda else put(t)))
            same(got, base, keys, (name, off))


@pytest.mark.parametrize("case", [(3, 5, 6, 10, 3), (3, 5, 5, 7, 3), (4, 130, 4, 4, 3), (2, 3, 64, 64, 3)], ids=O.case_id)
def test_a_sample_does_not_depend_on_the_batch(case):
    """the forward output of sample 1 inside its batch against the same sample run alone"""
    from sivae_hip import ops
    for blend in O.variants(case):
        d = O.to_inputs(case, blend)
        x, w, b, p = (put(d[k]) for k in ("x", "w", "bias", "prev"))
        bl = 1.0 if blend is None else blend
        whole = ops.style_to_rgb_fwd(x, w, b, p, bl)
        alone = ops.style_to_rgb_fwd(x[1:2].contiguous(), w, b, None if p is None else p[1:2].contiguous(), bl)
        assert torch.equal(whole[1:2], alone)
        d = O.from_inputs(case, blend)
        img, w, b, o = (put(d[k]) for k in ("img", "w", "bias", "other"))
        whole = ops.style_from_rgb_fwd(img, w, b, blend is not None, o, bl)
        alone = ops.style_from_rgb_fwd(img[1:2].contiguous(), w, b, blend is not None,
                                       None if o is None else o[1:2].contiguous(), bl)
        assert torch.equal(whole[1:2], alone)


@pytest.mark.parametrize("case", [(3, 5, 6, 10, 3), (2, 16, 8, 8, 3), (1, 2, 128, 128, 4)], ids=O.case_id)
def test_blend_one_is_the_plain_form(case):
    from sivae_hip import ops
    d = O.to_inputs(case, 0.25)
    x, w, b, p = (put(d[k]) for k in ("x", "w", "bias", "prev"))
    plain = ops.style_to_rgb_fwd(x, w, b)
    assert torch.equal(ops.style_to_rgb_fwd(x, w, b, p, 1.0), plain)
    assert not torch.equal(ops.style_to_rgb_fwd(x, w, b, p, 0.75), plain)
    # from_rgb: at blend 1 the result is `other`, at blend 0 the pooled layer alone; without pooling the plain form
    d = O.from_inputs(case, 0.25)
    img, w, b, o = (put(d[k]) for k in ("img", "w", "bias", "other"))
    pooled = ops.style_from_rgb_fwd(img, w, b, True)
    assert torch.equal(ops.style_from_rgb_fwd(img, w, b, True, o, 1.0), o)
    assert torch.equal(ops.style_from_rgb_fwd(img, w, b, True, o, 0.0), pooled)
    assert O.viol(pooled, O.from_rgb(d["img"], d["w"], d["bias"], True)) <= 1.0
    small = F.avg_pool2d(img, 2, 2)  # (exact inputs, but the average is rounded: compare with the kernel's own pooling)
    assert O.viol(ops.style_from_rgb_fwd(small, w, b), pooled) <= 1.0
    plain = ops.style_from_rgb_fwd(small, w, b)
    assert torch.equal(ops.style_from_rgb_fwd(small, w, b, False, plain.clone(), 0.75), plain)  # lerp(a, a, .) = a


def test_two_runs_are_bit_identical():
    for variant in (((3, 5, 6, 10, 3), 0.25), ((1, 1, 256, 256, 3), None), ((4, 130, 4, 4, 3), 0.75)):
        for op in ("to", "from"):
            case_fn, run, keys, _ = RUN[op]
            d, _ = case_fn(*variant)
            same(run(d), run(d), keys, (op, variant))


# ------------------------------------------------------------------------------------------------ flags
def wanted_alone(variant, op):
    """each gradient wanted alone, two together and none, against the run that wants them all, bit for bit"""
    case_fn, run, keys, _ = RUN[op]
    d, ref = case_fn(*variant)
    full = run(d)
    for bits in (1, 2, 4, 8, 6, 0):
        wants = tuple(bool(bits >> i & 1) for i in range(4))
        got = run(d, wants)
        for k, w in zip(keys[1:], wants):
            if w and ref[k] is not None:
                assert torch.equal(got[k], full[k]), (variant, wants, k)
            else:
                assert got[k] is None, (variant, wants, k)


@pytest.mark.parametrize("op", ["to", "from"])
def test_each_wanted_gradient_alone(op):
    for variant in (((3, 5, 6, 10, 3), 0.25), ((3, 5, 5, 7, 3), None), ((1, 2, 128, 128, 4), 0.75)):
        wanted_alone(variant, op)


# ------------------------------------------------------------------------------------------------ guarded
def guarded_variant(variant, op):
    """one op at one shape on guarded, poisoned outputs and workspaces of exactly the reported size, the inputs placed at an
    aligned base and one element behind it: nothing written outside a tensor, no element left at the poison value, the
    unguarded results"""
    from sivae_hip import ops
    from support.guard import describe, guarded
    case_fn, run, keys, _ = RUN[op]
    d, _ = case_fn(*variant)
    base = run(d)
    for off in (0, 1):
        with guarded(ops) as g:
            got = run(d, place=lambda t: None if t is None else g.place(put(t), offset_elems=off))
            damage = g.verify()
            assert not damage, "guard damage (%s, %s, offset %d):\n%s" % (op, variant, off, describe(damage))
        for k in keys:
            if base[k] is None:
                assert got[k] is None
            else:
                assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], base[k]), (op, variant, off, k)


def test_guarded():
    for variant in (((3, 5, 5, 7, 3), None), ((3, 5, 6, 10, 3), 0.25), ((2, 3, 2, 2, 3), 0.75), ((4, 130, 4, 4, 3), 0.25),
                    ((1, 2, 128, 128, 4), 0.75), ((1, 2, 128, 128, 4), None)):
        for op in ("to", "from"):
            guarded_variant(variant, op)


# ------------------------------------------------------------------------------------------------ autograd
@pytest.mark.parametrize("blend", [None, 0.25, 0.75])
def test_autograd_against_the_oracle(blend):
    """style.to_rgb and style.from_rgb through torch.autograd with the reference's parameter shapes, the gradients of prev
    and other included"""
    from sivae_hip import style
    case = (3, 5, 6, 10, 3)
    bl = 1.0 if blend is None else blend
    d, ref = to_case(case, blend)
    x, w, b, p = (None if d[k] is None else put(d[k]).requires_grad_(True) for k in ("x", "w", "bias", "prev"))
    w4 = w.detach().view(3, 5, 1, 1).requires_grad_(True)
    y = style.to_rgb(x, w4, b, p, bl)
    (y * put(d["g"])).sum().backward()
    assert O.viol(y, ref["y"]) <= 1.0 and w4.grad.shape == w4.shape
    for k, t in (("dx", x), ("dw", w4), ("dbias", b), ("dprev", p)):
        assert (t is None) or O.nerr(t.grad.reshape(ref[k].shape), ref[k]) <= GRAD_GATE, k
    d, ref = from_case(case, blend)
    img, w, b, o = (None if d[k] is None else put(d[k]).requires_grad_(True) for k in ("img", "w", "bias", "other"))
    w4 = w.detach().view(5, 3, 1, 1).requires_grad_(True)
    y = style.from_rgb(img, w4, b, blend is not None, o, bl)
    (y * put(d["g"])).sum().backward()
    assert O.viol(y, ref["y"]) <= 1.0
    for k, t in (("dimg", img), ("dw", w4), ("dbias", b), ("dother", o)):
        assert (t is None) or O.nerr(t.grad.reshape(ref[k].shape), ref[k]) <= GRAD_GATE, k


def test_autograd_with_inputs_that_need_no_gradient():
    from sivae_hip import style
    d, ref = from_case((3, 5, 6, 10, 3), 0.25)
    img, w, b, o = (put(d[k]) for k in ("img", "w", "bias", "other"))
    w.requires_grad_(True)
    y = style.from_rgb(img, w.view(5, 3, 1, 1), b, True, o, 0.25)  # (an image and a block output without gradients)
    (y * put(d["g"])).sum().backward()
    assert img.grad is None and b.grad is None and o.grad is None and O.nerr(w.grad, ref["dw"]) <= GRAD_GATE
    d, ref = to_case((3, 5, 6, 10, 3), 0.75)
    x, w, b, p = (put(d[k]) for k in ("x", "w", "bias", "prev"))
    p.requires_grad_(True)
    y = style.to_rgb(x, w.view(3, 5, 1, 1), b, p, 0.75)
    (y * put(d["g"])).sum().backward()
    assert x.grad is None and w.grad is None and O.nerr(p.grad, ref["dprev"]) <= GRAD_GATE
    with torch.no_grad():
        assert torch.equal(style.to_rgb(x, w.view(3, 5, 1, 1), b, p, 0.75), y)


# ------------------------------------------------------------------------------------------------ the classes
@pytest.fixture(scope="module")
def fx():
    return X.Fixture()


@pytest.fixture(scope="module")
def net():
    return X.import_net()


def load(net, fx, cls):
    m = X.make(net, cls, fx)
    sd = fx.state(cls)
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    return m.to(DEV), {k: v.shape for k, v in sd.items()}


def check_run(fx, m, shapes, pre, ins, outs, leads={}):
    outs = outs if isinstance(outs, tuple) else (outs,)
    sum((o * put(fx.tensor("%s/g%d" % (pre, i)))).sum() for i, o in enumerate(outs)).backward()
    worst_v = max(O.viol(o, fx.tensor("%s/out%d" % (pre, i))) for i, o in enumerate(outs))
    params = dict(m.named_parameters())
    want = fx.grads(pre, shapes)
    errs = {k: O.nerr(params[k].grad, g, leads.get(k, 0.0)) for k, g in want.items()}
    errs.update({"in/" + k: O.nerr(v.grad, fx.tensor("%s/grad/%s" % (pre, k))) for k, v in ins.items()})
    print("%s: outputs %.3f of the criterion, gradients worst %.2e (%s; gate %.1e)"
          % (pre, worst_v, max(errs.values()), max(errs, key=errs.get), CLASS_GRAD_GATE))
    assert worst_v <= 1.0
    assert max(errs.values()) <= CLASS_GRAD_GATE, errs
    for k, p in params.items():  # (a parameter the reference gave no gradient gets none here)
        assert (p.grad is not None) == (k in want), k


@pytest.mark.parametrize("run", X.RUNS)
@pytest.mark.parametrize("cls", X.ENCODERS + ("Generator",))
def test_networks_against_the_reference(fx, net, monkeypatch, cls, run):
    m, shapes = load(net, fx, cls)
    pre = "%s/%s" % (cls, run)
    meta = fx.json(pre + "/meta")
    leads = {}
    if cls == "Generator":
        # The first layer normalises the constant plane: its variance is 0, r = 1 / sqrt(eps) = 1e4, and the layer's
        # dbias = sum r (style + 1) (dy - mean dy) is exactly 0 (the norm removes what the bias adds; the reference records
        # float64 round-off).  It is measured as test_style_gpu measures the layer's dbias (style_oracle.nerr): against the
        # size of the terms of that difference, lead = max |r (style + 1)| max |dy|, taken from the layer's own call.
        from sivae_hip import style
        seen = []

        def spy(x, noise_weight, bias, st, *a, **k):
            y = style_layer(x, noise_weight, bias, st, *a, **k)
            if not seen:
                seen.append(float((st.detach()[:, :x.shape[1]] + 1).abs().max()) / 1e-8 ** 0.5)
                y.register_hook(lambda g: leads.update({"decode_block.0.bias_1": seen[0] * float(g.abs().max())}))
            return y

        style_layer = style.style_layer
        monkeypatch.setattr(style, "style_layer", spy)
        ins = {"styles": put(fx.tensor(pre + "/in/styles")).requires_grad_(True)}
        outs = m(ins["styles"], meta["lod"], meta["blend"], meta["noise"])
    else:
        ins = {"x": put(fx.tensor("encoders/%s/in/x" % run)).requires_grad_(True)}
        outs = m(ins["x"], meta["lod"], meta["blend"])
    check_run(fx, m, shapes, pre, ins, outs, leads)
    assert (cls == "Generator") == bool(leads)


@pytest.mark.parametrize("cls", X.MAPPING_CASES)
def test_mappings_against_the_reference(fx, net, cls):
    m, shapes = load(net, fx, cls)
    ins = {"x": put(fx.tensor(cls + "/run/in/x")).requires_grad_(True)}
    check_run(fx, m, shapes, cls + "/run", ins, m(ins["x"]))


@pytest.mark.parametrize("noise", [True, "batch_constant"])
def test_generator_with_noise(fx, net, noise):
    m, _ = load(net, fx, "Generator")
    styles = put(fx.tensor("Generator/lod2_blend0p25/in/styles"))
    with torch.no_grad():
        a, b = m(styles, 2, 0.25, noise), m(styles, 2, 0.25, noise)
    assert a.shape == (styles.shape[0], 3, 16, 16) and bool(torch.isfinite(a).all()) and not torch.equal(a, b)


def test_more_than_four_image_channels_take_the_torch_chain(net, monkeypatch):
    from sivae_hip import style
    for name in ("to_rgb", "from_rgb"):
        monkeypatch.setattr(style, name, lambda *a, **k: pytest.fail("the fused layer was called"))
    torch.manual_seed(0)
    t, f = net.ToRGB(6, 5).to(DEV), net.FromRGB(5, 6).to(DEV)
    with torch.no_grad():
        t.to_rgb.bias.normal_()
        f.from_rgb.bias.normal_()
    x, prev = torch.randn(2, 6, 8, 8, device=DEV), torch.randn(2, 5, 4, 4, device=DEV)
    conv = F.conv2d(x, t.to_rgb.weight, t.to_rgb.bias)
    assert torch.equal(t(x), conv)
    assert torch.equal(t.blended(x, prev, 0.25), torch.lerp(F.interpolate(prev, size=8), conv, 0.25))
    img, other = torch.randn(2, 5, 8, 8, device=DEV), torch.randn(2, 6, 4, 4, device=DEV)
    lr = lambda v: F.leaky_relu(v, 0.2)  # noqa: E731
    assert torch.equal(f.encode_input(img), lr(lr(F.conv2d(img, f.from_rgb.weight, f.from_rgb.bias))))
    a = lr(lr(F.conv2d(F.avg_pool2d(img, 2, 2), f.from_rgb.weight, f.from_rgb.bias)))
    assert torch.equal(f.encode_input(img, True, other, 0.75), torch.lerp(a, other, 0.75))
    # ... and a float64 tensor does too, while three channels in float32 do not
    t3 = net.ToRGB(6, 3).to(DEV)
    assert t3.double()(x.double()).dtype == torch.float64
    with pytest.raises(BaseException, match="fused layer"):
        t3.float()(x)


def test_fused_layers_are_the_torch_chain(net):
    """ToRGB / FromRGB on the kernels against the chain the classes fall back to, on the device"""
    torch.manual_seed(1)
    t, f = net.ToRGB(6, 3).to(DEV), net.FromRGB(3, 6).to(DEV)
    x, prev = torch.randn(2, 6, 8, 8, device=DEV), torch.randn(2, 3, 4, 4, device=DEV)
    conv = F.conv2d(x.double(), t.to_rgb.weight.double(), t.to_rgb.bias.double())
    assert O.viol(t.blended(x, prev, 0.25), torch.lerp(F.interpolate(prev.double(), size=8), conv, 0.25)) <= 1.0
    img = torch.randn(2, 3, 8, 8, device=DEV)
    one = F.leaky_relu(F.conv2d(img.double(), f.from_rgb.weight.double(), f.from_rgb.bias.double()), 0.2)
    assert O.viol(f(img), one) <= 1.0 and O.viol(f.encode_input(img), F.leaky_relu(one, 0.2)) <= 1.0


def test_one_introspective_round_trip_and_an_optimizer_step(net):
    """Generator -> Encoder -> MappingToLatent -> a loss -> backward -> LREQAdam over all parameters: everything finite,
    every parameter with a gradient moved, and a second forward sees the new weights (the kernels write through raw
    pointers: the packed convolution operands must follow)"""
    from sivae_hip.lreq_adam import LREQAdam
    torch.manual_seed(0)
    gen, enc = net.Generator(**X.CFG).to(DEV), net.Encoder(**X.CFG).to(DEV)
    mtl = net.VAEMappingToLatent_old(mapping_layers=3, latent_size=8, dlatent_size=8, mapping_fmaps=8).to(DEV)
    mfl = net.VAEMappingFromLatent(num_layers=6, mapping_layers=3, latent_size=8, dlatent_size=8, mapping_fmaps=8).to(DEV)
    params = [p for m in (gen, enc, mtl, mfl) for p in m.parameters()]
    opt = LREQAdam(params, lr=0.05)
    z = torch.randn(4, 8, device=DEV)

    def forward():
        img = gen(mfl(z), 2, 0.75, False)
        lat = mtl(enc(img, 2, 0.75))
        return img, lat

    img0, lat0 = forward()
    assert img0.shape == (4, 3, 16, 16) and lat0.shape == (4, 2, 8)
    loss = lat0.square().mean() + img0.square().mean()
    loss.backward()
    before = [p.detach().clone() for p in params]
    with_grad = [p.grad is not None for p in params]
    assert sum(with_grad) > len(params) // 2 and all(bool(torch.isfinite(p.grad).all()) for p in params if p.grad is not None)
    opt.step()
    for p, old, had in zip(params, before, with_grad):
        assert bool(torch.isfinite(p).all())
        assert torch.equal(p, old) != (had and bool((p.grad != 0).any())), "a parameter with a gradient did not move"
    img1, lat1 = forward()
    assert bool(torch.isfinite(img1).all()) and bool(torch.isfinite(lat1).all())
    assert not torch.equal(img1, img0) and not torch.equal(lat1, lat0)
    # the second forward is what fresh modules holding the new state compute
    twin_g, twin_e = net.Generator(**X.CFG).to(DEV), net.Encoder(**X.CFG).to(DEV)
    twin_g.load_state_dict(gen.state_dict())
    twin_e.load_state_dict(enc.state_dict())
    img2 = twin_g(mfl(z), 2, 0.75, False)
    assert torch.equal(img2, img1) and torch.equal(mtl(twin_e(img2, 2, 0.75)), lat1)
