"""GPU checks of the style variant's mapping networks, style assembly and model class: the kernels of csrc/mapping.hip and
the LeakyReLU epilogue of csrc/linear.hip through sivae_hip.ops, the autograd Functions sivae_hip.style.mapping / styles,
the `map` methods of the drop-in net.py and the drop-in model.py, against the float64 oracle tests/style_model_oracle.py
and the fixture recorded from the reference's model.py (tests/golden/style_model.npz).

Tolerances.  Forward outputs: the project's element-wise criterion |a - ref| <= 1e-4 |ref| + 1e-5 max |ref| (O.viol <= 1).
Gradients of the ops: the normalised error O.nerr is held to GRAD_GATE, which comes from what a float32 torch restatement
of the same formulas loses on the CPU against the float64 one over O.CASES and O.EDGE_CASES, NOT from the kernels:

    cd tests && python style_model_oracle.py
    float32 restatement against float64 over 119 cases: forward viol 0.0327, gradient nerr 1.91e-07 -> gradient gate 7.65e-07

The gate is 4 x that figure for the different summation order of a parallel reduction, and never looser than 1e-4.  The
gradients that cancel are measured against the size of their terms (nerr's lead): the pixel-norm dx (lead = max r max |dy|,
a row of one element cancels to the order of eps), dbias, ds and ds2 (lead = max |dy|).  dz is compared where the kernel's
output and the oracle's pre-activation have the same sign (it follows the sign by design) and bit for bit against torch's
LeakyReLU backward everywhere.  The model chains convolutions, blocks and these ops: its gradients are held to the
project's fp32 figure 1e-4 (CLASS_GRAD_GATE, as test_style_net_gpu), its losses to test_e2e_gpu.TOL.

One identity the ops cannot have: style.mapping's output is torch.equal to the per-layer chain only behind the pixel-norm,
because torch's mean over a row and the kernel's add in different orders.  The classes with a pixel-norm are therefore
compared bit for bit from the normalised rows on, and by the criterion as a whole."""
import functools

import pytest
import torch
import torch.nn.functional as F

import style_model_fixture as MF
import style_model_oracle as O
import style_net_fixture as NF

pytestmark = pytest.mark.gpu

FP32_GRAD_LOSS = 1.91e-07                       # measured, see above
GRAD_GATE = min(4 * FP32_GRAD_LOSS, 1e-4)       # = 7.64e-07
CLASS_GRAD_GATE = 1e-4
TOL = 1e-4                                      # test_e2e_gpu.TOL
DEV = "cuda:0"
B = 2


def put(t):
    return None if t is None else t.float().to(DEV).contiguous()


def shifted(t, off):
    """t copied `off` elements behind a 512-byte aligned base"""
    buf = torch.empty(t.numel() + off, dtype=torch.float32, device=DEV)
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
    return v


@functools.lru_cache(maxsize=None)
def pn_case(B_, Z):
    return O.pn_case(B_, Z)


@functools.lru_cache(maxsize=None)
def lin_case(B_, K, N):
    return O.lin_case(B_, K, N)


@functools.lru_cache(maxsize=None)
def st_case(shape, var):
    return O.st_case(shape, var)


def vid(v):
    return "x".join(str(i) for i in v)


def stid(c):
    (shape, (cut, tcut, beta)) = c
    return "%s-mix%s-trunc%s-beta%s" % (vid(shape), cut, tcut, beta)


# ------------------------------------------------------------------------------------------------ pixel-norm
def run_pn(d, off=(0, 0)):
    from sivae_hip import ops
    x, g = (put(d[k]) if o == 0 else shifted(put(d[k]), o) for k, o in zip(("x", "g"), off))
    y, r = ops.pixel_norm_fwd(x)
    return y, r, ops.pixel_norm_bwd(g, x, r)


@pytest.mark.parametrize("case", O.PN_CASES, ids=vid)
def test_pixel_norm_against_the_oracle(case):
    d = pn_case(*case)
    y, r, dx = run_pn(d)
    v, e = O.viol(y, d["y"]), O.nerr(dx, d["dx"], lead=d["lead"])
    print("pixel_norm %s: y %.3f of the criterion, dx %.2e (gate %.2e)" % (vid(case), v, e, GRAD_GATE))
    assert v <= 1.0 and e <= GRAD_GATE
    assert r.shape == (case[0],)


@pytest.mark.parametrize("Z", [1, 3, 8, 255, 256, 257, 1027, 4100])
def test_pixel_norm_zero_and_planted_rows(Z):
    """a row of zeros gives y = 0 and a finite dx = dy / sqrt(eps); a single large element at the LAST position among tiny
    ones: a row sum that drops its tail misses the criterion by orders of magnitude"""
    from sivae_hip import ops
    x64 = torch.cat([O.planted_rows(Z), torch.zeros(1, Z, dtype=torch.float64)]).requires_grad_(True)
    g64 = O.rand(4, Z, seed=Z)
    y64 = O.pixel_norm(x64)
    (dx64,) = torch.autograd.grad((y64 * g64).sum(), x64)
    x, g = put(x64.detach()), put(g64)
    y, r = ops.pixel_norm_fwd(x)
    dx = ops.pixel_norm_bwd(g, x, r)
    assert torch.equal(y[3], torch.zeros(Z, device=DEV)) and bool(torch.isfinite(dx).all())
    assert O.viol(dx[3], g64[3] * 1e4) <= 1.0
    r64 = torch.rsqrt(x64.detach().pow(2).mean(1) + O.EPS)
    for row in range(3):
        assert O.viol(y[row], y64[row].detach()) <= 1.0, row
        assert O.nerr(dx[row], dx64[row], lead=float(r64[row] * g64[row].abs().max())) <= GRAD_GATE, row


@pytest.mark.parametrize("case", [(3, 8), (3, 65), (5, 256), (2, 1027)], ids=vid)
def test_pixel_norm_alignment_and_batch_change_no_bit(case):
    d = pn_case(*case)
    base = run_pn(d)
    for off in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3)):
        got = run_pn(d, off=off)
        assert all(torch.equal(a, b) for a, b in zip(got, base)), off
    one = {k: (v[1:2] if isinstance(v, torch.Tensor) else v) for k, v in d.items()}
    alone = run_pn(one)
    assert all(torch.equal(a[0], b[1]) for a, b in zip(alone, base))


# ------------------------------------------------------------------------------------------------ linear + LeakyReLU
def split_for(tiles, contraction):
    """linear.hip's contraction split restated: about 1024 waves per call, slices of at least 64 in multiples of 16"""
    S = max(1, min(-(-1024 // tiles), max(contraction // 64, 1), 64))
    length = -(-(-(-contraction // S)) // 16) * 16
    return -(-contraction // length)


# the site of the LeakyReLU: inside linear_fwd_kernel (S == 1) or inside linear_reduce_kernel (S > 1)
LIN_SIDE = {(1, 8, 12): "gemm", (2, 12, 8): "gemm", (2, 64, 32): "gemm", (2, 128, 36): "reduce", (33, 512, 512): "reduce",
            (130, 512, 1024): "reduce", (257, 128, 64): "reduce"}


@pytest.mark.parametrize("case", O.LIN_CASES, ids=vid)
def test_linear_lrelu_against_the_oracle_and_torch(case):
    from sivae_hip import functional as SF
    from sivae_hip import lib, ops
    B_, K, N = case
    # which side of the split the shape is on: the exact workspace query is max(S_f B N, S_d B K) floats (+ 16 bytes), a
    # direction with S == 1 needing none
    s_f, s_d = split_for(-(-N // 32), K), split_for(-(-K // 32), N)
    want = max(s_f * B_ * N if s_f > 1 else 0, s_d * B_ * K if s_d > 1 else 0) * 4 + 16
    assert lib.load().sivae_linear_workspace_bytes(B_, K, N) == want
    side = "gemm" if s_f == 1 else "reduce"
    assert side == LIN_SIDE[case] and (s_f == 1) == (K < 128)
    d = lin_case(*case)
    x, w, b, g = (put(d[k]) for k in ("x", "w", "b", "g"))
    y = ops.linear_lrelu_fwd(x, w, b, O.SLOPE)
    dz, db = ops.lrelu_bias_bwd(g, y, O.SLOPE)
    # bit-identities: the chain it replaces, and torch's LeakyReLU backward
    pre = SF.linear(x, w, b)
    assert torch.equal(y, F.leaky_relu(pre, O.SLOPE))
    pre_t = pre.detach().clone().requires_grad_(True)
    (dz_t,) = torch.autograd.grad(F.leaky_relu(pre_t, O.SLOPE), pre_t, g)
    assert torch.equal(dz, dz_t)
    assert torch.equal(ops.linear_fwd(x, w, b), pre) and torch.equal(ops.linear_fwd(x, w, b, relu=True), F.relu(pre))
    same = ((y > 0).cpu() == (d["y"] > 0))
    v = O.viol(y, d["y"])
    e_dz = O.nerr(dz.cpu() * same, d["dz"] * same)
    # (dbias adds every dz: where the signs differ the kernel's own dz is the reference's summand)
    db_ref = torch.where(same, d["dz"], dz.cpu().double()).sum(0)
    e_db = O.nerr(db, db_ref, lead=float(d["g"].abs().max()))
    print("linear_lrelu %s (%s): y %.3f of the criterion, dz %.2e, dbias %.2e (gate %.2e), %d sign flips"
          % (vid(case), side, v, e_dz, e_db, GRAD_GATE, int((~same).sum())))
    assert v <= 1.0 and e_dz <= GRAD_GATE and e_db <= GRAD_GATE
    # a sample inside its batch against the same sample alone
    i = B_ // 2
    assert torch.equal(ops.linear_lrelu_fwd(x[i:i + 1].contiguous(), w, b, O.SLOPE)[0], y[i])


@pytest.mark.parametrize("case", [(2, 64, 32), (2, 128, 36), (33, 512, 512)], ids=vid)
def test_linear_lrelu_alignment_changes_no_bit(case):
    from sivae_hip import ops
    d = lin_case(*case)
    x, w, b, g = (put(d[k]) for k in ("x", "w", "b", "g"))
    y = ops.linear_lrelu_fwd(x, w, b, O.SLOPE)
    dz, db = ops.lrelu_bias_bwd(g, y, O.SLOPE)
    for off in (1, 2, 3):
        # (the GEMM's 16-byte operand loads need aligned x and w: the bias and the backward's tensors move)
        assert torch.equal(ops.linear_lrelu_fwd(x, w, shifted(b, off), O.SLOPE), y)
        for which in range(2):
            a = [g, y]
            a[which] = shifted(a[which], off)
            dz2, db2 = ops.lrelu_bias_bwd(a[0], a[1], O.SLOPE)
            assert torch.equal(dz2, dz) and torch.equal(db2, db), (off, which)
        db3 = ops.lrelu_bias_bwd(g, y, O.SLOPE, want_dz=False, out=shifted(torch.zeros_like(db), off))[1]
        assert torch.equal(db3, db)


def test_lrelu_slope_at_zero_and_plain_layers():
    """a zero input row with a zero bias gives pre-activations of exactly 0: the backward applies `slope` there (torch's
    rule); a layer without activation passes dy through and only sums the bias gradient"""
    from sivae_hip import ops
    d = lin_case(2, 64, 32)
    x, w, g = put(d["x"]), put(d["w"]), put(d["g"])
    x[1].zero_()
    y = ops.linear_lrelu_fwd(x, w, torch.zeros(32, device=DEV), O.SLOPE)
    assert torch.equal(y[1], torch.zeros(32, device=DEV))
    dz, db = ops.lrelu_bias_bwd(g, y, O.SLOPE)
    assert torch.equal(dz[1], g[1] * O.SLOPE)
    dz2, db2 = ops.lrelu_bias_bwd(g, None)
    assert dz2 is g and O.nerr(db2, d["g"].sum(0), lead=float(d["g"].abs().max())) <= GRAD_GATE
    assert ops.lrelu_bias_bwd(g, y, want_dz=False, want_dbias=False) == (None, None)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="slope"):
            ops.linear_lrelu_fwd(x, w, None, bad)


# ------------------------------------------------------------------------------------------------ styles
def run_st(d, shape, var, offs=(0, 0, 0, 0)):
    from sivae_hip import ops
    (B_, L, Z), (cut, tcut, beta) = shape, var
    mv = lambda t, o: None if t is None else (put(t) if o == 0 else shifted(put(t), o))  # noqa: E731
    s, s2, avg, g = (mv(d[k], o) for k, o in zip(("s", "s2", "avg", "g"), offs))
    psi = O.PSI if tcut is not None else None
    out = ops.styles_fwd(s, L, s2, cut, avg, beta, psi, tcut)
    ds, ds2 = ops.styles_bwd(g, s2 is not None, cut, psi, tcut)
    return dict(out=out, avg_out=avg, ds=ds, ds2=ds2)


@pytest.mark.parametrize("case", O.ST_CASES, ids=stid)
def test_styles_against_the_oracle(case):
    shape, var = case
    d = st_case(shape, var)
    got = run_st(d, shape, var)
    lead = float(d["g"].abs().max())
    v = O.viol(got["out"], d["out"])
    errs = {"ds": O.nerr(got["ds"], d["ds"], lead=lead)}
    if d["ds2"] is not None:
        errs["ds2"] = O.nerr(got["ds2"], d["ds2"], lead=lead)
    else:
        assert got["ds2"] is None
    if d["avg_out"] is not None:
        v = max(v, O.viol(got["avg_out"], d["avg_out"]))
    print("styles %s: out / avg %.3f of the criterion; %s (gate %.2e)"
          % (stid(case), v, ", ".join("%s %.2e" % kv for kv in errs.items()), GRAD_GATE))
    assert v <= 1.0 and max(errs.values()) <= GRAD_GATE, errs
    if var == (None, None, None):  # the plain output is the broadcast, bit for bit
        assert torch.equal(got["out"], put(d["s"]).unsqueeze(1).expand(-1, shape[1], -1))
    if var[2] is None and d["avg"] is not None:  # no update: the average is as it was
        assert torch.equal(got["avg_out"], put(d["avg"]))


@pytest.mark.parametrize("case", [((3, 6, 7), (3, 3, 0.0)), ((2, 6, 8), (3, 3, 0.995)), ((4, 14, 512), (7, 7, 0.0)),
                                  ((2, 6, 1027), (1, 6, 0.995))], ids=stid)
def test_styles_alignment_changes_no_bit(case):
    shape, var = case
    d = st_case(shape, var)
    base = run_st(d, shape, var)
    for which in range(4):
        for off in (1, 2, 3):
            offs = [0, 0, 0, 0]
            offs[which] = off
            got = run_st(d, shape, var, offs)
            assert all(torch.equal(got[k], base[k]) for k in base), (which, off)


@pytest.mark.parametrize("case", [((3, 6, 7), (3, 3, None)), ((130, 18, 512), (9, 9, None)), ((4, 14, 512), (None, None, None))],
                         ids=stid)
def test_a_sample_of_styles_does_not_depend_on_its_batch(case):
    shape, var = case
    d = st_case(shape, var)
    base = run_st(d, shape, var)
    i = shape[0] // 2
    one = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) and k != "avg" else v) for k, v in d.items()}
    alone = run_st(one, (1,) + shape[1:], var)
    for k in ("out", "ds", "ds2"):
        assert (base[k] is None and alone[k] is None) or torch.equal(alone[k][0], base[k][i]), k


def test_styles_function_updates_the_average_in_place_without_a_gradient():
    from sivae_hip import style
    shape, var = (3, 6, 7), (3, 3, 0.0)
    d = st_case(shape, var)
    s, s2, avg, g = put(d["s"]).requires_grad_(True), put(d["s2"]).requires_grad_(True), put(d["avg"]), put(d["g"])
    out = style.styles(s, 6, s2=s2, cutoff=3, avg=avg, beta=0.0, psi=O.PSI, trunc_cutoff=3)
    (out * g).sum().backward()
    assert O.viol(out, d["out"]) <= 1.0 and O.viol(avg, d["avg_out"]) <= 1.0 and not avg.requires_grad
    lead = float(d["g"].abs().max())
    assert O.nerr(s.grad, d["ds"], lead=lead) <= GRAD_GATE and O.nerr(s2.grad, d["ds2"], lead=lead) <= GRAD_GATE
    s.grad = None
    s2f = put(d["s2"])
    (style.styles(s, 6, s2=s2f, cutoff=3) * g).sum().backward()
    assert s2f.grad is None and s.grad is not None
    with pytest.raises(ValueError, match="no gradient"):
        style.styles(s, 6, avg=avg.clone().requires_grad_(True), beta=0.5)


# ------------------------------------------------------------------------------------------------ guarded
def test_nothing_outside_the_tensors_is_written():
    """all four ops on guarded, poisoned outputs and exact workspaces, at shapes with a scalar tail and several blocks"""
    from sivae_hip import ops
    from support.guard import describe, guarded
    for off in (0, 1):
        with guarded(ops) as gd:
            d = pn_case(5, 255)
            x, g = gd.place(put(d["x"]), offset_elems=off), put(d["g"])
            y, r = ops.pixel_norm_fwd(x)
            dx = ops.pixel_norm_bwd(g, x, r)
            assert O.viol(y, d["y"]) <= 1.0 and O.nerr(dx, d["dx"], lead=d["lead"]) <= GRAD_GATE
            for case in ((2, 12, 8), (2, 128, 36), (33, 512, 512)):
                c = lin_case(*case)
                xx, w, b, gg = (put(c[k]) for k in ("x", "w", "b", "g"))
                yy = ops.linear_lrelu_fwd(xx, w, b, O.SLOPE)
                dz, db = ops.lrelu_bias_bwd(gd.place(gg, offset_elems=off), yy, O.SLOPE,
                                            out=gd.place(torch.zeros(case[2], device=DEV), offset_elems=off))
                assert O.viol(yy, c["y"]) <= 1.0 and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(db).all())
            for shape, var in (((3, 6, 7), (3, 3, 0.0)), ((2, 6, 1027), (1, 6, 0.995)), ((130, 18, 512), (9, 9, 0.0))):
                c = st_case(shape, var)
                s, s2, g3 = (gd.place(put(c[k]), offset_elems=off) for k in ("s", "s2", "g"))
                avg = gd.place(put(c["avg"]), offset_elems=off)
                out = ops.styles_fwd(s, shape[1], s2, var[0], avg, var[2], O.PSI, var[1])
                ds, ds2 = ops.styles_bwd(g3, True, var[0], O.PSI, var[1])
                assert O.viol(out, c["out"]) <= 1.0 and O.viol(avg, c["avg_out"]) <= 1.0
                assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(ds2).all())
            damage = gd.verify()
            assert not damage, "guard damage at offset %d:\n%s" % (off, describe(damage))


# ------------------------------------------------------------------------------------------------ style.mapping and the classes
@pytest.fixture(scope="module")
def net():
    return NF.import_net()


@pytest.fixture(scope="module")
def nfx():
    return NF.Fixture()


def load_mapping(net, nfx, cls):
    m = NF.make(net, cls, nfx)
    m.load_state_dict({k: v.float() for k, v in nfx.state(cls).items()}, strict=True)
    return m.to(DEV)


@pytest.mark.parametrize("cls", NF.MAPPING_CASES)
def test_mapping_is_the_per_layer_chain(net, nfx, cls):
    """style.mapping (one node) against the chain it replaces: outputs torch.equal (from the normalised rows on where the
    class has a pixel-norm, see the module docstring), parameter and input gradients within the gradient gate"""
    from sivae_hip import ops
    m = load_mapping(net, nfx, cls)
    x0 = put(nfx.tensor(cls + "/run/in/x"))
    rows = x0.reshape(-1, x0.shape[-1])
    gsum = None
    res = {}
    for fused in (True, False):
        for p in m.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        y = m.map(x, fused=fused)
        gsum = torch.randn(y.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) if gsum is None else gsum
        (y * gsum).sum().backward()
        res[fused] = (y.detach(), x.grad, {k: p.grad.clone() for k, p in m.named_parameters()})
    normalise = getattr(m, "normalise", cls.startswith("Mapping"))
    if not normalise:
        assert torch.equal(res[True][0], res[False][0])
    else:
        assert O.viol(res[True][0], res[False][0]) <= 1.0
        fcs = [getattr(b, "fc", b) for b in (m.map_blocks if hasattr(m, "map_blocks") else
                                             [getattr(m, "block_%d" % (i + 1)) for i in range(m.mapping_layers)])]
        ws, bs = [f.weight for f in fcs], [f.bias for f in fcs]
        from sivae_hip import style
        with torch.no_grad():
            normed = ops.pixel_norm_fwd(rows)[0]
            assert torch.equal(res[True][0], style.mapping_chain(normed, ws, bs, False, 0.2, True))
    errs = {"x": O.nerr(res[True][1], res[False][1], lead=float(res[False][1].abs().max()))}
    for k, g in res[False][2].items():
        errs[k] = O.nerr(res[True][2][k], g)
    print("mapping %s: gradients worst %.2e (%s; gate %.2e)" % (cls, max(errs.values()), max(errs, key=errs.get), GRAD_GATE))
    assert max(errs.values()) <= GRAD_GATE, errs
    # forward is map followed by the class's view / repeat
    out = m(x0)
    assert out.shape == tuple(nfx[cls + "/run/out0"].shape) and O.viol(out, nfx.tensor(cls + "/run/out0")) <= 1.0


def test_mapping_wanted_gradient_combinations(net, nfx, monkeypatch):
    """frozen parameters give None and launch no weight gradient; an input without a gradient stops the data gradients"""
    from sivae_hip import ops, style
    m = load_mapping(net, nfx, "VAEMappingFromLatent5")
    fcs = [b.fc for b in m.map_blocks]
    ws, bs = [f.weight for f in fcs], [f.bias for f in fcs]
    calls = {"wgrad": 0, "dgrad": 0}
    wgrad, dgrad = ops.linear_wgrad, ops.linear_dgrad
    monkeypatch.setattr(ops, "linear_wgrad", lambda *a, **k: (calls.__setitem__("wgrad", calls["wgrad"] + 1), wgrad(*a, **k))[1])
    monkeypatch.setattr(ops, "linear_dgrad", lambda *a, **k: (calls.__setitem__("dgrad", calls["dgrad"] + 1), dgrad(*a, **k))[1])
    x = torch.randn(4, 8, device=DEV, requires_grad=True)

    def run():
        for p in m.parameters():
            p.grad = None
        x.grad = None
        calls.update(wgrad=0, dgrad=0)
        style.mapping(x, ws, bs, True).square().sum().backward()
    run()
    full = (x.grad.clone(), [p.grad.clone() for p in m.parameters()])
    assert calls == {"wgrad": 5, "dgrad": 5}
    for p in m.parameters():  # the E-step and the D-step freeze whole mapping networks
        p.requires_grad_(False)
    run()
    assert calls == {"wgrad": 0, "dgrad": 5} and all(p.grad is None for p in m.parameters())
    assert torch.equal(x.grad, full[0])
    for p in m.parameters():
        p.requires_grad_(True)
    ws[0].requires_grad_(False)
    bs[3].requires_grad_(False)
    run()
    assert calls == {"wgrad": 4, "dgrad": 5} and ws[0].grad is None and bs[3].grad is None
    assert all(torch.equal(p.grad, g) for p, g in zip(m.parameters(), full[1]) if p.grad is not None)
    ws[0].requires_grad_(True)
    bs[3].requires_grad_(True)
    for p in (ws[0], bs[0], ws[1], bs[1]):
        p.requires_grad_(False)
    x2 = x.detach()
    for p in m.parameters():
        p.grad = None
    calls.update(wgrad=0, dgrad=0)
    style.mapping(x2, ws, bs, True).square().sum().backward()
    # nothing in front of layer 2 wants a gradient: its data gradient and everything before it is not computed
    assert calls == {"wgrad": 3, "dgrad": 2}
    assert all(torch.equal(p.grad, g) for p, g in zip(m.parameters(), full[1]) if p.grad is not None)
    with torch.no_grad():
        assert not style.mapping(x, ws, bs, True).requires_grad


@pytest.mark.parametrize("slope,last", [(0.2, False), (None, True), (0.0, True), (1.0, True)])
def test_mapping_epilogue_variants_are_the_chain(slope, last):
    """the last layer without activation, no activation at all (VAEMappingToLatentNoStyle), and the ends of the slope range"""
    from sivae_hip import style
    torch.manual_seed(2)
    x = torch.randn(5, 8, device=DEV)
    ws = [torch.randn(12, 8, device=DEV, requires_grad=True), torch.randn(128, 12, device=DEV, requires_grad=True),
          torch.randn(8, 128, device=DEV, requires_grad=True)]
    bs = [torch.randn(n, device=DEV, requires_grad=True) for n in (12, 128, 8)]
    res = []
    for run in (style.mapping, style.mapping_chain):
        for p in ws + bs:
            p.grad = None
        y = run(x, ws, bs, False, slope, last)
        y.square().sum().backward()
        res.append((y.detach(), [p.grad.clone() for p in ws + bs]))
    assert torch.equal(res[0][0], res[1][0])
    assert max(O.nerr(a, b) for a, b in zip(res[0][1], res[1][1])) <= GRAD_GATE


def test_refused_shapes_and_other_dtypes_take_the_chain(monkeypatch):
    from sivae_hip import style
    monkeypatch.setattr(style.MappingFn, "forward", lambda *a, **k: pytest.fail("the fused node was called"))
    torch.manual_seed(0)
    x = torch.randn(3, 6, device=DEV)  # K = 6 is no multiple of 4: ops.linear_supported refuses it
    ws, bs = [torch.randn(8, 6, device=DEV), torch.randn(8, 8, device=DEV)], [torch.randn(8, device=DEV) for _ in range(2)]
    y = style.mapping(x, ws, bs, True, 0.2, False)
    ref = O.pixel_norm(x.double().cpu())
    ref = F.leaky_relu(ref @ ws[0].double().cpu().t() + bs[0].double().cpu(), 0.2) @ ws[1].double().cpu().t() + bs[1].double().cpu()
    assert O.viol(y, ref) <= 1.0


# ------------------------------------------------------------------------------------------------ the model against the fixture
@pytest.fixture(scope="module")
def fx():
    return MF.Fixture()


@pytest.fixture(scope="module")
def model():
    return MF.import_model()


def build(model, fx, kw_key):
    m = model.SoftIntroVAEModelTL(**fx.json(kw_key))
    sd = fx.state("model")
    sd["dlatent_avg.buff"] = fx.tensor("model/buff_in")
    m.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    for k in MF.LAST:
        setattr(m, k, torch.tensor(MF.LAST_IN.get(k, 0.0)))
    return m.to(DEV), {k: v.shape for k, v in sd.items()}


def rel(a, ref):
    return abs(float(a) - ref) / max(abs(ref), 1e-30)


def check_grads(fx, run, m, shapes, meta, x=None):
    params = dict(m.named_parameters())
    want = fx.grads(run, shapes)
    assert [k for k, p in params.items() if p.grad is not None] == meta["grad_keys"]
    top = max(float(g.abs().max()) for g in want.values())
    errs = {k: O.nerr(params[k].grad, g, lead=top if k in meta["zero_grad_keys"] else 0.0) for k, g in want.items()}
    if x is not None:
        errs["x"] = O.nerr(x.grad, fx.tensor(run + "/grad_x"))
    return errs


BRANCH_SETS = {"vae": ("last_rec_loss", "last_real_kl"), "d_train": ("last_rec_loss", "last_fake_kl"),
               "e_train": ("last_rec_loss", "last_real_kl", "last_expelbo_fake", "last_expelbo_rec")}
FORWARD_RUNS = MF.Fixture().runs("forward")
GENERATE_RUNS = MF.Fixture().runs("generate")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("run", FORWARD_RUNS)
def test_forward_branches_against_the_reference(fx, model, monkeypatch, run, fused):
    """the three branches of forward at three (lod, blend) on the reference's replayed draws, with model.FUSED on and off"""
    monkeypatch.setattr(model, "FUSED", fused)
    meta = fx.json(run + "/meta")
    m, shapes = build(model, fx, "model/kwargs")
    x = put(fx.tensor(run + "/x")).requires_grad_(True)
    with MF.replay(fx.draws(run), meta["seed"], B):
        loss = m(x, meta["lod"], meta["blend"], meta["branch"] == "d_train", meta["branch"] == "e_train")
    loss.backward()
    scal = {"loss": rel(loss, meta["loss"])}
    for k in MF.LAST:
        t = getattr(m, k)
        assert t.dim() == 0 and not t.requires_grad, k
        if k in BRANCH_SETS[meta["branch"]]:  # (what the branch takes from its losses; the others are as they were)
            assert t.is_cuda, k
        scal[k] = rel(t, meta[k]) if meta[k] != 0.0 else abs(float(t))
    v_buff = O.viol(m.dlatent_avg.buff, fx.tensor(run + "/buff"))
    errs = check_grads(fx, run, m, shapes, meta, x)
    print("%s [%s]: scalars worst %.2e (%s; TOL %.0e), buff %.3f of the criterion, gradients worst %.2e (%s; gate %.0e)"
          % (run, "fused" if fused else "torch", max(scal.values()), max(scal, key=scal.get), TOL, v_buff,
             max(errs.values()), max(errs, key=errs.get), CLASS_GRAD_GATE))
    assert max(scal.values()) <= TOL, scal
    assert v_buff <= 1.0
    assert max(errs.values()) <= CLASS_GRAD_GATE, errs
    assert [k for k, p in m.named_parameters() if p.requires_grad] == meta["requires_grad"]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("run", GENERATE_RUNS)
def test_generate_with_average_truncation_and_mixing(fx, model, monkeypatch, run, fused):
    """direct generate runs with dlatent_avg_beta=0.995, truncation_psi=0.7, truncation_cutoff=4, mixing taken and not"""
    monkeypatch.setattr(model, "FUSED", fused)
    meta = fx.json(run + "/meta")
    m, shapes = build(model, fx, "model/gen_kwargs")
    assert (m.truncation_psi, m.truncation_cutoff, m.dlatent_avg_beta) == (0.7, 4, 0.995)
    with MF.replay(fx.draws(run), meta["seed"], B):
        img = m.generate(meta["lod"], meta["blend"], count=B, mixing=True, noise=True)
    (img * put(fx.tensor(run + "/g"))).sum().backward()
    v, v_buff = O.viol(img, fx.tensor(run + "/out")), O.viol(m.dlatent_avg.buff, fx.tensor(run + "/buff"))
    errs = check_grads(fx, run, m, shapes, meta)
    print("%s [%s]: image %.3f, buff %.3f of the criterion, gradients worst %.2e (%s; gate %.0e), mixing %s"
          % (run, "fused" if fused else "torch", v, v_buff, max(errs.values()), max(errs, key=errs.get), CLASS_GRAD_GATE,
             meta["mixing"]))
    assert v <= 1.0 and v_buff <= 1.0 and max(errs.values()) <= CLASS_GRAD_GATE, errs


def test_forward_synchronises_nowhere_and_lerp_leaves_the_buffer(fx, model):
    """last_* are device scalars the training script's .data.cpu() still works on; lerp averages parameters only"""
    run = FORWARD_RUNS[1]
    meta = fx.json(run + "/meta")
    m, _ = build(model, fx, "model/kwargs")
    other, _ = build(model, fx, "model/kwargs")
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
        other.dlatent_avg.buff.add_(1.0)
    x = put(fx.tensor(run + "/x"))
    with MF.replay(fx.draws(run), meta["seed"], B):
        m(x, meta["lod"], meta["blend"], meta["branch"] == "d_train", meta["branch"] == "e_train")
    assert m.last_rec_loss.is_cuda and m.last_rec_loss.data.cpu().shape == ()
    before = [p.detach().clone() for p in m.parameters()]
    buff = m.dlatent_avg.buff.clone()
    m.lerp(other, 0.75)
    for p, old, q in zip(m.parameters(), before, other.parameters()):
        assert O.viol(p, torch.lerp(old.double(), q.double(), 0.25)) <= 1.0
    assert torch.equal(m.dlatent_avg.buff, buff)
