"""GPU checks of the style variant's optimizer: the multi-tensor kernels of csrc/multi_tensor.hip through
sivae_hip.ops.mt_lreq_adam / mt_lerp_ and the class sivae_hip.lreq_adam.LREQAdam, against the float64 oracle
tests/lreq_adam_oracle.py and the trajectory recorded from the reference (tests/golden/lreq_adam.npz).  Shapes come from
the library's own limits (T tensors, K chunks of C elements per launch), not from a workload.

Bounds of one step, from the operation order in the header of multi_tensor.hip, with u = 2^-24 (one fp32 rounding, relative)
and the oracle fed the device's fp32 state from before the step and the DOUBLE scalars the host formed:

  v' = fl(fl(b2' v) + fl(w2' fl(g g))), b2' and w2' the fp32 images of beta2 and 1 - beta2.  Both terms are >= 0, so the
       sum's relative error is the worse term's (3 roundings: image, g g, product) plus the addition's: 4 roundings,
       |dv'| <= 5 u v'  (one unit of slack for the second-order terms)
  U  = fl(s' fl(g / fl(fl(sqrt(v')) + eps'))): v' carries 4 u, its square root half of that, 2 u, plus the root's own
       rounding: 3 u; eps' (the image of eps) carries 1 u and both summands are >= 0: the worse, 3 u, plus the addition's:
       4 u; the division: 5 u; s' (the image of the step size): 6 u; the product: 7 u.  7 roundings where the issue that
       asked for this test counted 8, so the gate is 8 u |U| (one unit of slack), tighter than its 10 u |U|
  p' = fl(p - U): 1 rounding, |dp'| <= u |p'| + 8 u |U|

The average, d = fl(q - p), |w| < 0.5: fl(p + fl(w' d)): d carries u |d|, the image of w and the product one each:
|w d| 3 u <= 1.5 u (|p| + |q|), and the addition u |p'| <= u (|p| + |q|): 2.5 u (|p| + |q|).  Otherwise fl(q - fl(d om)),
om = fl(1 - w') exact (Sterbenz) but w' off by u w: |d| (u (1 - w) + u w + u (1 - w)) = (2 - w) u |d| <= 1.5 u (|p| + |q|)
for 0.5 <= w <= 1, and the subtraction's u (|p| + |q|): 2.5 u (|p| + |q|).  Gate: 3 u (|p| + |q|) on both branches.

Trajectory gate: 4 x the deviation of the reference's own float32 run from its float64 run, recorded in the fixture
(p 1.932e-07, v 1.689e-07), per tensor and max-norm.  Measured through the fused path on an MI355X: p 1.932e-07,
v 1.724e-07 (gates 7.728e-07 and 6.758e-07)."""
import copy
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import lreq_adam_oracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BLOCKS_DIR = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd", "style_soft_intro_vae")
DEV = "cuda:0"
U = 2.0 ** -24
BETA2, EPS = 0.99, 1e-8
WEIGHTS = (1.0 - 0.5 ** (32 / (10 * 1000.0)), 0.75)  # the training script's value (< 0.5) and one on the other branch


@functools.lru_cache(maxsize=None)
def limits():
    from sivae_hip import lib
    L = lib.load()
    return L.sivae_mt_max_tensors(), L.sivae_mt_max_chunks(), L.sivae_mt_chunk_elems()


def sizes_all():
    T, K, C = limits()
    return [0, 1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3, K * C + C + 5]  # (the last: more chunks than a launch has)


def size_lists():
    """name -> element counts: 1, T and T + 1 tensors, every size (the large tensor is cut between two launches), and a
    list whose chunks pass K in the middle of a tensor that would fit a launch of its own"""
    T, K, C = limits()
    small = [1, 3, 4, 5, 64, 257, 1023, C - 1, C, C + 1, 2 * C + 3]
    return {"one": [2 * C + 3], "T": [small[i % len(small)] for i in range(T)],
            "T+1": [small[(i + 3) % len(small)] for i in range(T + 1)], "sizes": sizes_all(),
            "cut": [3, C + 1, (K - 2) * C - 7, 5]}


@functools.lru_cache(maxsize=None)
def case(name):
    """(p, g, v, q) lists of float32 device tensors and the step sizes (doubles), made once and never written"""
    sizes = size_lists()[name]
    gen = torch.Generator(device=DEV).manual_seed(len(sizes) * 7919 + sum(sizes) % 1000)
    rn = lambda n: torch.randn(n, device=DEV, generator=gen)  # noqa: E731
    p, g, v, q, s = [], [], [], [], []
    for t, n in enumerate(sizes):
        scale = 10.0 ** (torch.rand(n, device=DEV, generator=gen) * 4.0 - 3.0)  # gradient magnitudes 1e-3 .. 10
        p.append(rn(n))
        g.append(rn(n) * scale)
        v.append((rn(n) * scale).square() * 0.5)
        q.append(rn(n))
        s.append(1.5e-3 * math.sqrt(1.0 - BETA2 ** (1 + t % 7)) * (1.0, 0.0721, 2.5, 0.0147)[t % 4])
    return p, g, v, q, s


def clones(ts):
    return [t.clone() for t in ts]


def fused_step(p, g, v, s):
    from sivae_hip import ops
    p, v = clones(p), clones(v)
    n = ops.mt_lreq_adam(p, g, v, s, BETA2, EPS)
    return p, v, n


def fused_lerp(p, q, w):
    from sivae_hip import ops
    p = clones(p)
    n = ops.mt_lerp_(p, q, w)
    return p, n


def step_ratio(p0, g, v0, s, p1, v1):
    """the worst |error| / bound over the elements of one tensor -> (p, v), from the float64 oracle evaluated on the device"""
    if p0.numel() == 0:
        return 0.0, 0.0
    P, V, Ud = O.step_tensor(p0.double(), v0.double(), g.double(), s, BETA2, EPS, xp=torch)
    rv = ((v1.double() - V).abs() / (5 * U * V)).max()
    rp = ((p1.double() - P).abs() / (U * P.abs() + 8 * U * Ud.abs())).max()
    return float(rp), float(rv)


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("name", ["one", "T", "T+1", "sizes", "cut"])
def test_step_against_the_oracle(name):
    from sivae_hip import ops
    p0, g, v0, _, s = case(name)
    g_before = clones(g)
    p1, v1, launches = fused_step(p0, g, v0, s)
    worst = [max(r) for r in zip(*(step_ratio(*ts) for ts in zip(p0, g, v0, s, p1, v1)))]
    print("step %s: %d tensors in %d launch(es), worst error / bound: p %.3f, v %.3f" % (name, len(p0), launches, *worst))
    assert worst[0] <= 1.0 and worst[1] <= 1.0
    assert all(torch.equal(a, b) for a, b in zip(g, g_before))
    assert launches == ops.mt_launches([t.numel() for t in p0]) == {"one": 1, "T": 1, "T+1": 2, "sizes": 2, "cut": 2}[name]
    assert any(not torch.equal(a, b) for a, b in zip(p0, p1))


@pytest.mark.parametrize("w", WEIGHTS, ids=["small", "large"])
@pytest.mark.parametrize("name", ["T+1", "sizes"])
def test_lerp_against_the_oracle(name, w):
    p0, _, _, q, _ = case(name)
    q_before = clones(q)
    p1, launches = fused_lerp(p0, q, w)
    worst = 0.0
    for a, b, r in zip(p0, q, p1):
        if a.numel():
            ref = O.lerp(a.double(), b.double(), w, xp=torch)
            worst = max(worst, float(((r.double() - ref).abs() / (3 * U * (a.double().abs() + b.double().abs()))).max()))
    print("lerp %s w %.6f: %d launch(es), worst error / bound %.3f" % (name, w, launches, worst))
    assert worst <= 1.0 and launches == 2
    assert all(torch.equal(a, b) for a, b in zip(q, q_before))


# ------------------------------------------------------------------------------------------------ the class
@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "lreq_adam.npz"))


def test_recorded_trajectory_through_the_fused_path(fx):
    """the fixture's 12 steps (None gradients, the second group's changing lr, the state reset) on device tensors, every
    step fused; gate and measured figures: the module's docstring"""
    from sivae_hip.lreq_adam import LREQAdam
    nt = len(O.SIZES)
    params = [fx["p0/%d" % t] for t in range(nt)]
    base = [[fx["g%d/%d" % (i, t)] for t in range(nt)] for i in range(2)]
    seen = []

    def after_step(k, opt):
        seen.append(k)
        want = sum(O.has_grad(k, t) for t in range(nt))
        assert opt.last_step == {"fused": want, "fallback": 0, "launches": 1}, (k, opt.last_step)

    out, _, _ = O.run_class(LREQAdam, params, base, torch.float32, device=DEV, after_step=after_step)
    assert seen == list(range(1, O.STEPS + 1))
    gate = 4 * float(fx["f32_dev_p"]), 4 * float(fx["f32_dev_v"])
    worst = [0.0, 0.0]
    for k in O.SNAPSHOTS:
        assert out[k][2] == [int(s) for s in fx["steps%d" % k]]
        for t in range(nt):
            for j, key in enumerate("pv"):
                worst[j] = max(worst[j], O.rel_dev(out[k][j][t], fx["%s%d/%d" % (key, k, t)]))
    print("trajectory through the fused path: p %.3e (gate %.3e), v %.3e (gate %.3e)" % (worst[0], gate[0], worst[1], gate[1]))
    assert worst[0] <= gate[0] and worst[1] <= gate[1]


# ------------------------------------------------------------------------------------------------ independence
def test_a_tensor_does_not_depend_on_the_rest_of_the_list():
    """alone, as the first, the 38th and the last of T + 1, and twice in a row: bit-identical; the average too"""
    T, K, C = limits()
    p, g, v, q, s = case("T+1")
    n = 2 * C + 3
    own = [x[0] for x in case("one")]  # (p, g, v, q, s of the tensor followed through the lists)
    alone = fused_step([own[0]], [own[1]], [own[2]], [own[4]])
    again = fused_step([own[0]], [own[1]], [own[2]], [own[4]])
    assert torch.equal(alone[0][0], again[0][0]) and torch.equal(alone[1][0], again[1][0])
    alone_l = {w: fused_lerp([own[0]], [own[3]], w)[0][0] for w in WEIGHTS}
    for at in (0, 37, T):
        ins = [list(x) for x in (p, g, v, q, s)]
        for lst, x in zip(ins, own):
            lst[at] = x
        assert ins[0][at].numel() == n
        p1, v1, _ = fused_step(*ins[:3], ins[4])
        assert torch.equal(p1[at], alone[0][0]) and torch.equal(v1[at], alone[1][0]), at
        for w in WEIGHTS:
            assert torch.equal(fused_lerp(ins[0], ins[3], w)[0][at], alone_l[w]), (at, w)
    full = fused_step(p, g, v, s), fused_step(p, g, v, s)
    assert all(torch.equal(a, b) for j in range(2) for a, b in zip(full[0][j], full[1][j]))


@pytest.mark.parametrize("offs", [(1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 0, 0), (0, 2, 0), (0, 0, 3), (4, 4, 4)])
def test_alignment_changes_no_bit(offs):
    """a tensor in a fresh allocation against the same values as a view 1, 2 or 3 elements into a larger buffer (every
    pointer, and each pointer alone, so that the scalar walk meets the 16-byte walk); 4: aligned again"""
    own = [x[0] for x in case("one")]
    n = own[0].numel()
    alone = fused_step([own[0]], [own[1]], [own[2]], [own[4]])

    def view(t, off):
        buf = torch.zeros(n + 8, device=DEV)
        buf[off:off + n] = t
        return buf, buf[off:off + n]

    (bp, p), (bg, g), (bv, v) = (view(t, o) for t, o in zip(own[:3], offs))
    from sivae_hip import ops
    ops.mt_lreq_adam([p], [g], [v], [own[4]], BETA2, EPS)
    assert torch.equal(p, alone[0][0]) and torch.equal(v, alone[1][0]) and torch.equal(g, own[1])
    for buf, off in ((bp, offs[0]), (bv, offs[2])):  # nothing next to the views was written
        assert float(buf[:off].abs().sum()) == 0.0 and float(buf[off + n:].abs().sum()) == 0.0
    for w in WEIGHTS:
        (bp, p), (bq, q) = view(own[0], offs[0]), view(own[3], offs[1])
        ops.mt_lerp_([p], [q], w)
        assert torch.equal(p, fused_lerp([own[0]], [own[3]], w)[0][0]) and torch.equal(q, own[3])
        assert float(bp[:offs[0]].abs().sum()) == 0.0 and float(bp[offs[0] + n:].abs().sum()) == 0.0


def test_non_finite_gradients_stay_in_their_elements():
    p, g, v, q, s = case("T")
    T, K, C = limits()
    at = max(range(len(p)), key=lambda t: p[t].numel())
    n = p[at].numel()
    bad = clones(g)
    bad[at][1] = float("inf")
    bad[at][n - 2] = float("nan")
    clean, dirty = fused_step(p, g, v, s), fused_step(p, bad, v, s)
    for j in range(2):
        for t, (a, b) in enumerate(zip(clean[j], dirty[j])):
            if t != at:
                assert torch.equal(a, b)
                continue
            finite = torch.isfinite(b)
            assert (~finite).nonzero().flatten().tolist() == [1, n - 2]
            assert torch.equal(a[finite], b[finite]) and bool(torch.isfinite(a).all())


# ------------------------------------------------------------------------------------------------ guarded
def test_nothing_outside_the_tensors_is_written():
    """parameters, states and gradients of every size placed 0 .. 3 elements behind a guarded base (0xFF on both sides):
    no guard byte changes, the gradients keep their bits, the results are those of the plain allocations"""
    from sivae_hip import ops
    from support.guard import describe, guarded
    p, g, v, q, s = case("sizes")
    want_p, want_v, _ = fused_step(p, g, v, s)
    want_l = fused_lerp(p, q, WEIGHTS[0])[0]
    for offs in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (1, 2, 3)):
        with guarded(ops) as gd:
            pp, pg, pv = ([gd.place(t, offset_elems=o) for t in ts] for ts, o in zip((p, g, v), offs))
            lp, lq = ([gd.place(t, offset_elems=o) for t in ts] for ts, o in zip((p, q), offs))
            ops.mt_lreq_adam(pp, pg, pv, s, BETA2, EPS)
            ops.mt_lerp_(lp, lq, WEIGHTS[0])
            damage = gd.verify()
            assert not damage, "guard damage at offsets %s:\n%s" % (offs, describe(damage))
        for got, want in ((pp, want_p), (pv, want_v), (pg, g), (lp, want_l), (lq, q)):
            assert all(torch.equal(a, b) for a, b in zip(got, want)), offs


# ------------------------------------------------------------------------------------------------ last_step, fallback
def _params(sizes, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ps = []
    for t, n in enumerate(sizes):
        p = torch.nn.Parameter(torch.randn(n, device=DEV, generator=gen))
        p.grad = torch.randn(n, device=DEV, generator=gen)
        if t % 2:
            p.lr_equalization_coef = 0.25
        ps.append(p)
    return ps


def test_last_step_reports_what_ran():
    from sivae_hip.lreq_adam import LREQAdam
    T, K, C = limits()
    for count, launches in ((T, 1), (T + 1, 2)):
        ps = _params([5 + t for t in range(count)])
        half = len(ps) // 2
        opt = LREQAdam([{"params": ps[:half], "lr": 2e-3}, {"params": ps[half:]}], lr=1e-3)  # (two groups, ONE call)
        opt.step()
        assert opt.last_step == {"fused": count, "fallback": 0, "launches": launches}
        ps[3].grad = None
        opt.step()
        assert opt.last_step == {"fused": count - 1, "fallback": 0, "launches": 1}
        assert opt.state[ps[3]]["step"] == 1 and opt.state[ps[4]]["step"] == 2


def test_a_non_contiguous_parameter_takes_the_torch_path(fx):
    """... and still matches the oracle: that path is torch's arithmetic, not the kernels', so its gate is the trajectory
    gate (4 x the reference's own float32 loss), not the kernels' rounding count"""
    from sivae_hip.lreq_adam import LREQAdam
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = torch.nn.Parameter(torch.randn(6, 9, device=DEV, generator=gen).t())
    b = torch.nn.Parameter(torch.randn(6, 9, device=DEV, generator=gen))
    c = torch.nn.Parameter(torch.randn(6, 9, device=DEV, generator=gen).double())
    assert not a.is_contiguous()
    for t in (a, b, c):
        t.grad = torch.randn(t.shape, device=DEV, generator=gen).to(t.dtype)
    before = [t.detach().double().cpu().numpy().copy() for t in (a, b, c)]
    opt = LREQAdam([a, b, c], lr=1e-2)
    opt.step()
    assert opt.last_step == {"fused": 1, "fallback": 2, "launches": 1}
    gate = 4 * max(float(fx["f32_dev_p"]), float(fx["f32_dev_v"]))
    for t, p0 in zip((a, b, c), before):
        want, v, _ = O.step_tensor(p0, np.zeros_like(p0), t.grad.double().cpu().numpy(), O.step_size(1e-2, 0.99, 1))
        assert O.rel_dev(t.detach().cpu().numpy(), want) <= gate
        assert O.rel_dev(opt.state[t]["exp_avg_sq"].cpu().numpy(), v) <= gate
    # a non-contiguous gradient of a contiguous parameter falls back too
    b.grad = torch.randn(9, 6, device=DEV, generator=gen).t()
    a.grad = c.grad = None
    opt.step()
    assert opt.last_step == {"fused": 0, "fallback": 1, "launches": 0}


# ------------------------------------------------------------------------------------------------ the blocks
@pytest.fixture(scope="module")
def blocks():
    sys.path.insert(0, BLOCKS_DIR)
    try:
        import blocks as B
    finally:
        sys.path.remove(BLOCKS_DIR)
    return B


def test_packed_weights_follow_a_fused_step_and_the_average(blocks):
    """the kernels write through raw pointers: without the generation bump the convolution would run on the operand
    packed from the old weight"""
    from sivae_hip import functional as SF
    from sivae_hip.lreq_adam import LREQAdam, lerp_parameters
    torch.manual_seed(0)
    conv = blocks._Conv3x3(16, 16).to(DEV)
    w = conv.weight
    x = torch.randn(2, 16, 8, 8, device=DEV)

    def fresh():
        return SF.conv_bias(x, torch.nn.Parameter(w.detach().clone()), None).detach()

    y0 = SF.conv_bias(x, w, None).detach()  # (packs and caches the operand)
    assert torch.equal(y0, fresh())
    w.grad = torch.randn_like(w)
    opt = LREQAdam([w], lr=0.1)
    opt.step()
    assert opt.last_step["fused"] == 1
    y1 = SF.conv_bias(x, w, None).detach()
    assert torch.equal(y1, fresh()) and not torch.equal(y1, y0)
    r = lerp_parameters([w], [torch.randn_like(w)], 0.5)
    assert r == {"fused": 1, "fallback": 0, "launches": 1}
    y2 = SF.conv_bias(x, w, None).detach()
    assert torch.equal(y2, fresh()) and not torch.equal(y2, y1)


def eager_step(params, state, lr, beta_2=0.99, eps=1e-8):
    """the five element-wise operations per tensor the fused step replaces, on .data as the reference's loop"""
    for p in params:
        if p.grad is None:
            continue
        st = state.setdefault(p, {"step": 0, "exp_avg_sq": torch.zeros_like(p.data)})
        st["step"] += 1
        v, g = st["exp_avg_sq"], p.grad.data
        v.mul_(beta_2).addcmul_(g, g, value=1 - beta_2)
        denom = v.sqrt().add_(eps)
        p.data.addcdiv_(g, denom, value=-lr * math.sqrt(1 - beta_2 ** st["step"]) * getattr(p, "lr_equalization_coef", 1.0))


def test_two_steps_of_an_encoder_and_a_decoder_block(blocks, fx):
    """EncodeBlock and DecodeBlock at 8 x 8 with 16 channels: two steps of the class against two steps of the eager loop
    on a deep copy, within the trajectory gate"""
    from sivae_hip import functional as SF
    from sivae_hip.lreq_adam import LREQAdam
    torch.manual_seed(3)
    enc = blocks.EncodeBlock(16, 16, 32, last=False, fused_scale=False).to(DEV)
    dec = blocks.DecodeBlock(16, 16, 32, has_first_conv=True, fused_scale=False, layer=0).to(DEV)
    nets = torch.nn.ModuleList([enc, dec])
    with torch.no_grad():  # (the constructors leave biases and noise weights at 0, which would hide them)
        for k, p in nets.named_parameters():
            if "bias" in k or "noise_weight" in k:
                p.normal_(0.0, 0.5)
    twin = copy.deepcopy(nets)
    for a, b in zip(nets.parameters(), twin.parameters()):
        b.__dict__.pop("_sivae_pack", None)
        if hasattr(a, "lr_equalization_coef"):
            b.lr_equalization_coef = a.lr_equalization_coef
    x = torch.randn(2, 16, 8, 8, device=DEV)
    gy = [torch.randn(2, 16, 4, 4, device=DEV), torch.randn(2, 32, device=DEV), torch.randn(2, 32, device=DEV),
          torch.randn(2, 16, 8, 8, device=DEV)]

    def backward(m):
        torch.manual_seed(11)  # (the decoder block draws its noise)
        for p in m.parameters():
            p.grad = None
        h, w1, w2 = m[0](x)
        y = m[1](h, w1, w2, True)
        ((h * gy[0]).sum() + (w1 * gy[1]).sum() + (w2 * gy[2]).sum() + (y * gy[3]).sum()).backward()

    opt = LREQAdam([{"params": list(enc.parameters())}, {"params": list(dec.parameters()), "lr": 2e-3}], lr=1.5e-3)
    state = {}
    for _ in range(2):
        backward(nets)
        opt.step()
        assert opt.last_step["fallback"] == 0 and opt.last_step["fused"] == sum(p.grad is not None for p in nets.parameters())
        backward(twin)
        eager_step(list(twin[0].parameters()), state, 1.5e-3)
        eager_step(list(twin[1].parameters()), state, 2e-3)
        SF.bump_generation(twin.parameters())  # (.data writes move no version counter either)
    gate = 4 * float(fx["f32_dev_p"])
    names = [k for k, _ in nets.named_parameters()]
    devs = {k: O.rel_dev(a.detach().cpu().numpy(), b.detach().cpu().numpy())
            for k, a, b in zip(names, nets.parameters(), twin.parameters())}
    print("two steps, fused against eager: worst %.3e (%s; gate %.3e)" % (max(devs.values()), max(devs, key=devs.get), gate))
    assert opt.last_step["fused"] > 0 and max(devs.values()) <= gate, devs
