"""Host checks of the style variant's optimizer (no GPU): the float64 oracle tests/lreq_adam_oracle.py and the class
sivae_hip.lreq_adam.LREQAdam on CPU tensors (its torch path) against the trajectory recorded from the reference
(tests/golden/lreq_adam.npz), the rules the training loop relies on, and the C entry points' argument validation."""
import collections
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

import lreq_adam_oracle as O
from sivae_hip import lib
from sivae_hip.lreq_adam import LREQAdam, lerp_parameters

HERE = os.path.dirname(os.path.abspath(__file__))
DROPIN_DIR = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd", "style_soft_intro_vae")
EXACT = 1e-13  # float64 against float64: the same operations in the same order, up to the order of the scalar products
NT = len(O.SIZES)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "lreq_adam.npz"))


def inputs(fx):
    return [fx["p0/%d" % t] for t in range(NT)], [[fx["g%d/%d" % (i, t)] for t in range(NT)] for i in range(2)]


def recorded(fx, k):
    return ([fx["p%d/%d" % (k, t)] for t in range(NT)], [fx["v%d/%d" % (k, t)] for t in range(NT)],
            [int(s) for s in fx["steps%d" % k]])


def worst(got, want):
    """the worst per-tensor max-norm relative deviation -> (params, exp_avg_sq)"""
    return tuple(max(O.rel_dev(a, b) for a, b in zip(got[j], want[j])) for j in range(2))


def test_fixture_is_what_the_oracle_module_describes(fx):
    params, base = inputs(fx)
    p2, b2 = O.make_inputs()
    assert all(np.array_equal(a, b) for a, b in zip(params, p2))
    assert all(np.array_equal(a, b) for i in range(2) for a, b in zip(base[i], b2[i]))
    assert tuple(a.size for a in params) == O.SIZES and min(O.SIZES) == 1 and max(O.SIZES) == 8193
    mags = np.abs(np.concatenate([g for i in range(2) for g in base[i]]))
    assert np.quantile(mags, 0.05) < 1e-3 and mags.max() > 10.0
    assert any(c is None for c in O.COEFS) and any(c is not None for c in O.COEFS)
    for t in range(NT):  # every tensor misses a gradient at some step and has one at another
        assert {O.has_grad(k, t) for k in range(1, O.STEPS + 1)} == {True, False}
    assert 1 < O.RESET_BEFORE < O.STEPS and len({O.lr1(k) for k in range(1, O.STEPS + 1)}) == O.STEPS
    assert 0 < float(fx["f32_dev_p"]) < 1e-6 and 0 < float(fx["f32_dev_v"]) < 1e-6
    w = fx["lerp_w"]
    assert w[0] == 1.0 - 0.5 ** (32 / (10 * 1000.0)) and w[0] < 0.5 <= w[1]
    assert os.path.getsize(os.path.join(HERE, "golden", "lreq_adam.npz")) < 1 << 20


def test_oracle_reproduces_the_reference(fx):
    params, base = inputs(fx)
    tr = O.trajectory(params, base)
    for k in O.SNAPSHOTS:
        want = recorded(fx, k)
        dp, dv = worst(tr[k], want)
        print("oracle against the reference after step %d: p %.2e, v %.2e" % (k, dp, dv))
        assert dp <= EXACT and dv <= EXACT
        assert tr[k][2] == want[2]
    for i, w in enumerate(fx["lerp_w"]):
        assert O.rel_dev(O.lerp(fx["lerp_p"], fx["lerp_q"], float(w)), fx["lerp_out%d" % i]) <= EXACT


def test_class_reproduces_the_reference_in_float64(fx):
    params, base = inputs(fx)
    out, opt, _ = O.run_class(LREQAdam, params, base, torch.float64)
    for k in O.SNAPSHOTS:
        want = recorded(fx, k)
        dp, dv = worst(out[k], want)
        assert dp <= EXACT and dv <= EXACT, (k, dp, dv)
        assert out[k][2] == want[2]
    assert opt.last_step["fused"] == 0 and opt.last_step["launches"] == 0 and opt.last_step["fallback"] > 0


def test_class_in_float32_stays_within_the_references_own_float32_loss(fx):
    params, base = inputs(fx)
    out, _, _ = O.run_class(LREQAdam, params, base, torch.float32)
    gate_p, gate_v = 4 * float(fx["f32_dev_p"]), 4 * float(fx["f32_dev_v"])
    for k in O.SNAPSHOTS:
        dp, dv = worst(out[k], recorded(fx, k))
        print("float32 class after step %d: p %.3e (gate %.3e), v %.3e (gate %.3e)" % (k, dp, gate_p, dv, gate_v))
        assert dp <= gate_p and dv <= gate_v


def test_state_dict_round_trip_continues_the_recorded_trajectory(fx):
    """the reference's float64 state after step 6 goes in through load_state_dict, steps 7 .. 12 end at its step-12 state"""
    params, base = inputs(fx)
    out, opt, _ = O.run_class(LREQAdam, params, base, torch.float64, first=7, resume=recorded(fx, 6))
    want = recorded(fx, 12)
    dp, dv = worst(out[12], want)
    assert dp <= EXACT and dv <= EXACT, (dp, dv)
    assert out[12][2] == want[2]
    sd = opt.state_dict()
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(["lr", "beta_2", "eps", "weight_decay", "params"])] * 2
    assert all(sorted(s) == ["exp_avg_sq", "step"] and isinstance(s["step"], int) for s in sd["state"].values())


def _one(n=5, coef=None, dtype=torch.float64):
    p = torch.nn.Parameter(torch.linspace(-1.0, 1.0, n, dtype=dtype))
    if coef is not None:
        p.lr_equalization_coef = coef
    return p


def _grad(n=5, dtype=torch.float64):
    return torch.linspace(0.5, 2.0, n, dtype=dtype)


def test_none_gradients_keep_their_step_and_state():
    a, b = _one(), _one()
    opt = LREQAdam([a, b], lr=1e-2)
    a.grad = _grad()
    opt.step()
    assert opt.state[a]["step"] == 1 and len(opt.state[b]) == 0
    assert opt.last_step == {"fused": 0, "fallback": 1, "launches": 0}
    b0 = b.detach().clone()
    a.grad, b.grad = None, _grad()
    a1 = a.detach().clone()
    opt.step()
    assert opt.state[a]["step"] == 1 and opt.state[b]["step"] == 1
    assert torch.equal(a.detach(), a1) and not torch.equal(b.detach(), b0)


def test_state_reset_starts_over():
    a = _one()
    opt = LREQAdam([a], lr=1e-2)
    for _ in range(3):
        a.grad = _grad()
        opt.step()
    assert opt.state[a]["step"] == 3
    opt.state = collections.defaultdict(dict)  # (lod_driver.set_epoch)
    before = a.detach().double().numpy().copy()
    a.grad = _grad()
    opt.step()
    assert opt.state[a]["step"] == 1
    want, v, _ = O.step_tensor(before, np.zeros(5), _grad().numpy(), O.step_size(1e-2, 0.99, 1))
    assert O.rel_dev(a.detach().numpy(), want) <= EXACT and O.rel_dev(opt.state[a]["exp_avg_sq"].numpy(), v) <= EXACT


def test_lr_is_read_per_call_and_per_group_and_a_missing_coefficient_is_one():
    a, b, c = _one(coef=0.25), _one(), _one(coef=1.0)
    opt = LREQAdam([{"params": [a], "lr": 1e-2}, {"params": [b, c]}], lr=1e-3)
    start = a.detach().numpy().copy()
    for t in (a, b, c):
        t.grad = _grad()
    opt.step()
    moved = [np.abs(t.detach().numpy() - start) for t in (a, b, c)]
    assert np.allclose(moved[0], moved[1] * 10 * 0.25, rtol=1e-12) and np.array_equal(moved[1], moved[2])
    opt.param_groups[1]["lr"] = 0.0  # (the scheduler rewrites it)
    b1 = b.detach().clone()
    a1 = a.detach().clone()
    opt.step()
    assert torch.equal(b.detach(), b1) and not torch.equal(a.detach(), a1)


def test_constructor_signature_and_errors():
    sig = inspect.signature(LREQAdam.__init__)
    assert list(sig.parameters) == ["self", "params", "lr", "betas", "eps", "weight_decay"]
    assert [sig.parameters[k].default for k in ("lr", "betas", "eps", "weight_decay")] == [1e-3, (0.0, 0.99), 1e-8, 0]
    assert issubclass(LREQAdam, torch.optim.Optimizer)
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(0.9, 0.99)), dict(betas=(0.0, 1.0)), dict(betas=(0.0, -0.1))):
        with pytest.raises(ValueError):
            LREQAdam([_one()], **kw)
    with pytest.raises(NotImplementedError):
        LREQAdam([_one()], weight_decay=1e-4)
    opt = LREQAdam([_one()])
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == dict(lr=1e-3, beta_2=0.99, eps=1e-8,
                                                                                     weight_decay=0)


def test_sparse_gradient_is_refused():
    a = _one()
    opt = LREQAdam([a])
    a.grad = _grad().to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        opt.step()


def test_closure_is_evaluated():
    a = _one()
    opt = LREQAdam([a])

    def closure():
        loss = (a * a).sum()
        loss.backward()
        return loss.detach()

    assert float(opt.step(closure)) > 0 and opt.state[a]["step"] == 1


def test_lerp_parameters_on_cpu_tensors(fx):
    for i, w in enumerate(fx["lerp_w"]):
        p = [torch.nn.Parameter(torch.from_numpy(fx["lerp_p"]).double()), torch.nn.Parameter(torch.zeros(0))]
        q = [torch.from_numpy(fx["lerp_q"]).double(), torch.zeros(0)]
        r = lerp_parameters(p, q, float(w))
        assert r == {"fused": 0, "fallback": 2, "launches": 0}
        assert O.rel_dev(p[0].detach().numpy(), fx["lerp_out%d" % i]) <= EXACT
        assert p[0]._sivae_gen == 1
    with pytest.raises(ValueError):
        lerp_parameters([torch.zeros(2)], [], 0.5)


def test_drop_in_module_exports_the_references_names():
    sys.path.insert(0, DROPIN_DIR)
    try:
        import custom_adam
    finally:
        sys.path.remove(DROPIN_DIR)
    assert custom_adam.LREQAdam is LREQAdam and custom_adam.lerp_parameters is lerp_parameters
    assert list(inspect.signature(custom_adam.lerp_parameters).parameters) == ["params", "other_params", "weight"]


# ------------------------------------------------------------------------------------------------ the C entry points
def _arr(values, dtype):
    a = np.array(values, dtype=dtype)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_size_queries_and_the_table():
    L = lib.load()
    T, K, C = L.sivae_mt_max_tensors(), L.sivae_mt_max_chunks(), L.sivae_mt_chunk_elems()
    assert T > 0 and K > 0 and C > 0
    assert C % 1024 == 0          # whole trips of 256 threads x 4 elements; a cut between launches keeps 16-byte alignment
    assert K * C < 2 ** 32        # a launch's share of a tensor is a 32-bit count
    assert 0 < L.sivae_mt_table_bytes() <= 4096
    # three addresses, a count, a step size and a prefix-sum entry per tensor cannot take less
    assert L.sivae_mt_table_bytes() >= T * (3 * 8 + 4 + 4 + 4)


def test_the_list_is_cut_by_tensors_and_by_chunks():
    L = lib.load()
    T, K, C = L.sivae_mt_max_tensors(), L.sivae_mt_max_chunks(), L.sivae_mt_chunk_elems()

    def launches(sizes):
        a, pa = _arr(sizes, np.uintp)
        return L.sivae_mt_launches(pa, len(sizes))

    assert launches([]) == 0 and launches([0, 0]) == 0
    assert launches([1]) == 1 and launches([5] * T) == 1 and launches([5] * (T + 1)) == 2
    assert launches([0] * T + [5] * T) == 1            # empty tensors take no slot
    assert launches([K * C]) == 1 and launches([K * C + 1]) == 2 and launches([2 * K * C + 1]) == 3
    assert launches([C + 1, (K - 2) * C]) == 1 and launches([C + 1, (K - 2) * C + 1]) == 2  # cut in the middle of a tensor
    assert launches([3, (K - 1) * C + 1] + [5] * T) == 3  # ... whose rest shares the next launch with T - 1 others
    assert L.sivae_mt_launches(None, 1) == -1 and launches([1]) == 1 and L.sivae_mt_launches(_arr([1], np.uintp)[1], -1) == -2


def test_entry_points_validate_before_any_launch():
    """every refusal is the documented negative code: a launch on this machine (no device) would give a positive HIP error,
    so the code also shows that the call returned before one; the legal empty calls return 0 for the same reason"""
    L = lib.load()
    NULL, SHAPE, RANGE = -1, -2, -5
    # (the arrays stay referenced until the function ends; the addresses in them are never dereferenced)
    adr, padr = _arr([4096, 8192], np.uint64)
    odd, podd = _arr([4096, 8194], np.uint64)
    zero, pzero = _arr([4096, 0], np.uint64)
    n, pn = _arr([8, 8], np.uintp)
    none, pnone = _arr([0, 0], np.uintp)
    s, ps = _arr([1e-3, 1e-3], np.float32)

    def adam(p=padr, g=padr, v=padr, cnt=pn, steps=ps, nt=2, beta2=0.99, omb=0.01, eps=1e-8):
        return L.sivae_mt_lreq_adam(p, g, v, cnt, steps, nt, beta2, omb, eps, None)

    def lerp(d=padr, q=padr, cnt=pn, nt=2, w=0.25):
        return L.sivae_mt_lerp(d, q, cnt, nt, w, None)

    for kw in (dict(p=None), dict(g=None), dict(v=None), dict(cnt=None), dict(steps=None)):
        assert adam(**kw) == NULL, kw
    for kw in (dict(p=pzero), dict(g=pzero), dict(v=pzero)):  # a null address of a tensor with elements
        assert adam(**kw) == NULL, kw
    assert adam(nt=-1) == SHAPE and adam(g=podd) == SHAPE
    for kw in (dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=float("nan")), dict(eps=-1e-8), dict(eps=float("nan")),
               dict(omb=float("inf"))):
        assert adam(**kw) == RANGE, kw
    for kw in (dict(d=None), dict(q=None), dict(cnt=None), dict(d=pzero), dict(q=pzero)):
        assert lerp(**kw) == NULL, kw
    assert lerp(nt=-1) == SHAPE and lerp(q=podd) == SHAPE
    for w in (float("inf"), float("-inf"), float("nan")):
        assert lerp(w=w) == RANGE
    # legal and launching nothing: no tensors, and tensors without elements (whose addresses may be null)
    assert adam(nt=0) == 0 and lerp(nt=0) == 0
    assert adam(p=pzero, g=pzero, v=pzero, cnt=pnone) == 0 and lerp(d=pzero, q=pzero, cnt=pnone) == 0


def test_wrappers_refuse_what_the_kernels_do_not_take():
    from sivae_hip import ops
    t = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mt_lreq_adam([t], [t], [t], [1e-3], 0.99, 1e-8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mt_lerp_([t], [t], 0.5)
    with pytest.raises(ValueError):
        ops.mt_lreq_adam([t], [t], [t], [], 0.99, 1e-8)
    with pytest.raises(ValueError):
        ops.mt_lerp_([t], [], 0.5)
    assert ops.mt_lreq_adam([], [], [], [], 0.99, 1e-8) == 0 and ops.mt_lerp_([], [], 0.5) == 0
