"""The kernel checks again, on guarded and poisoned outputs with workspaces of exactly the reported size
(tests/support/guard.py): a store outside the returned tensor, an output element no kernel wrote and an under-reported
`*_workspace_bytes()` all pass the plain checks (allocator padding, a recycled block that still holds the previous
answer, a workspace that is never smaller than 1 MiB) and corrupt training.

  a. every check of kernel_checks / kernel_checks16 at its own tolerance, plus intact guards
  b. `out=` / `accumulate=` / `pg_out=` destinations placed 0..3 elements behind an aligned start, the way
     optim.FlatAdam's gradient-slab views sit in their flat buffer: bit-identical to a fresh destination, guards intact
     (one exception, stated at `_up_dgrad_pool_case`: a route that changes kernel with the destination's alignment)
  c. the point-cloud ops on the scalar (N = 131) and the 16-byte (N = 132) paths against their fp64 restatements

No tolerance here is new: (a) and (c) use the ones of the unguarded tests, (b) compares bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import kernel_checks as kc
import kernel_checks16 as kc16
import pc3d_jsd_oracle as JO
import pc3d_oracle as O
from support.guard import describe, guarded
from support.pc import viol

pytestmark = pytest.mark.gpu
DEV = "cuda"
# process-level stress / time-limit checks: not about addressing
NOT_GUARDED = ("store_hazard_stress", "bn_fused_squatter", "bn_fused_timeout")
CHECKS = ([("fp32-" + label, thunk) for label, thunk in kc.all_checks() if label not in NOT_GUARDED]
          + [("bf16-" + label, thunk) for label, thunk in kc16.all_checks()])


def _mods():
    from sivae_hip import ops, ops16, pointcloud
    return ops, ops16, pointcloud


# ------------------------------------------------------------------------------------------------ a. the checks, guarded
def test_the_guard_sees_a_kernel_store_next_to_a_tensor_and_an_unwritten_element():
    """the harness itself on the device: a HIP kernel that is told to write one element more than the tensor has (into
    the guard: allocated memory, nothing faults) is reported with its byte range, and a kernel that is told to write one
    element less leaves NaN behind"""
    ops, ops16, _ = _mods()
    with guarded(ops, ops16) as g:
        import ctypes
        dst = g.place(torch.zeros(5, device=DEV), offset_elems=1)
        ops._lib.call("sivae_randn", ops._p(dst), 6, 1, 0, ops._s())  # (six normals into a tensor of five)
        (d,) = g.verify()
        # (the four bytes behind the 20 of the tensor; a byte of the value may itself be 0xFF)
        assert d["kind"] == "placed" and 20 <= d["first_byte"] <= d["last_byte"] <= 23 and d["damaged_bytes"] >= 3, d
        dst = g.place(torch.zeros(5, device=DEV), offset_elems=1)
        ops._lib.call("sivae_randn", ctypes.c_void_p(dst.data_ptr() - 4), 6, 1, 0, ops._s())  # (starting one element early)
        (d,) = g.verify()
        assert -4 <= d["first_byte"] <= d["last_byte"] <= -1 and d["damaged_bytes"] >= 3, d
        x = torch.ones(2, 3, 4, 4, device=DEV)
        y = ops.relu_fwd(x)  # (written in full)
        short = ops.randn((8,), 1, 0, torch.device(DEV))
        ops._lib.call("sivae_randn", ops._p(short), 7, 1, 0, ops._s())  # (the same draw, one element short)
        assert g.verify() == [] and bool(torch.isfinite(y).all()) and bool(torch.isfinite(short).all())
        fresh = ops.torch.empty(8, dtype=torch.float32, device=DEV)
        ops._lib.call("sivae_randn", ops._p(fresh), 7, 1, 0, ops._s())
        assert bool(torch.isfinite(fresh[:7]).all()) and bool(torch.isnan(fresh[7])) and kc._err(fresh, short) == float("inf")
        assert g.verify() == []


@pytest.mark.parametrize("label,thunk", CHECKS, ids=[c[0] for c in CHECKS])
def test_guarded_check(label, thunk):
    ops, ops16, _ = _mods()
    with guarded(ops, ops16) as g:
        results = thunk()
        damage = g.verify()
    bad = [(n, e, t) for (n, e, t) in results if not e <= t]
    assert not bad and not damage, "parity failures on poisoned outputs: %s\nguard damage:\n%s" % (bad, describe(damage))


# ------------------------------------------------------------------------------------------------ b. slab-view destinations
def _t(*shape, seed):
    return kc._rand(*shape, seed=seed).float().to(DEV)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


class _Switch:
    """ops switches set for one call and put back"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        ops = _mods()[0]
        self.saved = {k: getattr(ops, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(ops, k, v)

    def __exit__(self, *exc):
        ops = _mods()[0]
        for k, v in self.saved.items():
            setattr(ops, k, v)


def _conv_fwd_case(shape, accumulate):
    """the direct implicit-GEMM forward (a direct pack: no other route) into `out`"""
    ops = _mods()[0]
    B, Ci, Co, H, W, ks = shape
    x, w = _t(B, Ci, H, W, seed=1), _t(Co, Ci, ks, ks, seed=2) / math.sqrt(Ci * ks * ks)
    wp = ops.pack_weight(w, 0)
    init = _t(B, Co, H, W, seed=12) if accumulate else _nan(B, Co, H, W)
    return (init,), lambda out: (ops.conv2d_fwd(x, wp, Co, ks, out=out[0], accumulate=accumulate),)


def _conv_wgrad_case(shape, family, upsample=False, **switches):
    ops = _mods()[0]
    B, Ci, Co, H, W, ks = shape
    x = _t(B, Ci, H // 2, W // 2, seed=5) if upsample else _t(B, Ci, H, W, seed=1)
    dy = _t(B, Co, H, W, seed=4)

    def call(out):
        with _Switch(**switches):
            assert ops.conv2d_wgrad_route(B, Ci, Co, H, W, ks, upsample=upsample).family == family
            return (ops.conv2d_wgrad(x, dy, ks, upsample=upsample, out=out[0]),)
    return (_nan(Co, Ci, ks, ks),), call


def _up_dgrad_case(shape, accumulate):
    """the phase-form kernel (conv_wino_up_dgrad.hip); its tile geometry follows Ws >= 32, its K split over wave pairs
    N <= 64, and a destination that is only 4-byte aligned takes the dword-store instantiation of each"""
    ops = _mods()[0]
    B, Ci, Co, H, W, _ = shape
    dy, w = _t(B, Co, H, W, seed=4), _t(Co, Ci, 3, 3, seed=2) / math.sqrt(Ci * 9)
    wp = ops.PackedW(w, 0)
    init = _t(B, Ci, H // 2, W // 2, seed=12) if accumulate else _nan(B, Ci, H // 2, W // 2)

    def call(out):
        assert ops.conv2d_up_dgrad_route(B, Co, Ci, H, W).family == "wino_up_dgrad"  # (no K split: one summation order)
        return (ops.conv2d_up_dgrad(dy, wp, Ci, out=out[0], accumulate=accumulate),)
    return (init,), call


def _up_dgrad_pool_case(shape, accumulate):
    """conv2d_up_dgrad with the mode-1 pack: the F(4x4,3x3) kernel with the block sum in its output transform stores pixel
    PAIRS and takes 8-byte-aligned destinations only, so the route sends a destination at an odd element offset to the
    phase-form kernel: another kernel, another summation order — those offsets are held to the fp64 gradient at
    check_conv_up_dgrad's tolerance instead of to the fresh destination's bits"""
    ops = _mods()[0]
    B, Ci, Co, H, W, _ = shape
    xs = kc._rand(B, Ci, H // 2, W // 2, seed=5).requires_grad_()
    w64 = kc._rand(Co, Ci, 3, 3, seed=2, scale=1.0 / math.sqrt(Ci * 9))
    dy64 = kc._rand(B, Co, H, W, seed=4)
    kc._conv_ref(torch.nn.functional.interpolate(xs, scale_factor=2, mode="nearest"), w64).backward(dy64)
    base = kc._rand(B, Ci, H // 2, W // 2, seed=12)
    ref = xs.grad + base if accumulate else xs.grad
    dy, w = kc._d(dy64), kc._d(w64)
    wp, wp1 = ops.PackedW(w, 0), ops.PackedW(w, 1)
    init = kc._d(base) if accumulate else _nan(B, Ci, H // 2, W // 2)

    def call(out):
        al8 = not (out[0].data_ptr() & 7)
        r = ops.conv2d_up_dgrad_route(B, Co, Ci, H, W, has_wp1=True, dx_al8=al8)
        assert r.family == ("wino4_pool" if al8 else "wino_up_dgrad"), r.family
        return (ops.conv2d_up_dgrad(dy, wp, Ci, out=out[0], accumulate=accumulate, wp1=wp1),)
    return (init,), call, dict(ref=ref, tol=kc.WINO_TOL)


def _conv5_edge_case(shape, small_out):
    ops = _mods()[0]
    B, Cb, Cs, H, W = shape
    Ci, Co = (Cb, Cs) if small_out else (Cs, Cb)
    x, dy = _t(B, Ci, H, W, seed=1), _t(B, Co, H, W, seed=4)
    return (_nan(Co, Ci, 5, 5),), lambda out: (ops.conv5_edge_wgrad(x, dy, out=out[0]),)


def _linear_wgrad_case(shape):
    ops = _mods()[0]
    B, K, N = shape
    x, dy = _t(B, K, seed=1), _t(B, N, seed=4)
    return (_nan(N, K),), lambda out: (ops.linear_wgrad(dy, x, out=out[0]),)


def _bn_inputs(shape):
    ops = _mods()[0]
    B, C, H, W = shape
    x, r, dy = _t(B, C, H, W, seed=1) * 2.0 + 0.7, _t(B, C, H, W, seed=2), _t(B, C, H, W, seed=7)
    gamma, beta = _t(C, seed=3) * 0.5 + 1.0, _t(C, seed=4)
    mean, invstd = ops.bn_stats(x)
    return x, r, dy, gamma, beta, mean, invstd


def _bn_apply_case(shape):
    ops = _mods()[0]
    x, r, dy, gamma, beta, mean, invstd = _bn_inputs(shape)
    return (_nan(*shape),), lambda out: (ops.bn_apply_act(x, r, mean, invstd, gamma, beta, 0.2, out=out[0]),)


def _channel_sum_case(shape):
    ops = _mods()[0]
    x = _t(*shape, seed=1)
    return (_nan(shape[1]),), lambda out: (ops.channel_sum(x, out=out[0]),)


def _bn_bwd_case(shape, op, fused):
    """dgamma / dbeta into pg_out (dx, dz compared too); op: "saved" (sign from y), "recompute" (from x), "dzsum",
    "signmask"; fused: the one-launch persistent kernel where it takes the shape, or the three-launch form"""
    ops = _mods()[0]
    x, r, dy, gamma, beta, mean, invstd = _bn_inputs(shape)
    C = shape[1]
    y = ops.bn_apply_act(x, r, mean, invstd, gamma, beta, 0.2)
    mask = ops.bn_apply_act_signmask(x, r, mean, invstd, gamma, beta, 0.2)[2] if op == "signmask" else None

    def call(out):
        pg = None if out is None else (out[0], out[1])
        with _Switch(BN_FUSED=fused):
            route = ops.bn_bwd_route(*shape, op={"dzsum": "dzsum", "signmask": "signmask"}.get(op, "bn_bwd"))
            assert route.family == ("bn_fused" if fused else "bn_seg"), route.family
            if op == "saved":
                got = ops.bn_bwd(dy, y, x, mean, invstd, gamma, 0.2, want_dz=True, pg_out=pg)
            elif op == "recompute":
                got = ops.bn_bwd(dy, None, x, mean, invstd, gamma, 0.2, beta=beta, act_mode=2, pg_out=pg)
            elif op == "dzsum":
                got = ops.bn_bwd_dzsum(dy, y, x, mean, invstd, gamma, 0.2, pg_out=pg)
            else:
                got = ops.bn_bwd_signmask(dy, mask, x, mean, invstd, gamma, 0.2, pg_out=pg)
        dx, dz, dgamma, dbeta = got
        return (dgamma, dbeta, dx) + (() if dz is None else (dz,))
    return (_nan(C), _nan(C)), call


def _bn_from_partials_case(shape):
    """the BatchNorm backward whose reduction pass ran in the epilogue of the producing data gradient"""
    ops = _mods()[0]
    B, Cm, Co, H, W, _ = shape
    a, dc = _t(B, Cm, H, W, seed=1), _t(B, Co, H, W, seed=4)
    gamma, beta = _t(Cm, seed=8).abs() + 0.5, _t(Cm, seed=9)
    w2 = _t(Co, Cm, 3, 3, seed=2) / math.sqrt(Cm * 9)
    mean, invstd = ops.bn_stats(a)
    dh, part = ops.conv2d_dgrad_bnbwd(dc, ops.PackedW(w2, 1), Cm, a, mean, invstd, gamma, beta, 0.2)

    def call(out):
        da, dg, db = ops.bn_bwd_from_partials(dh, a, mean, invstd, gamma, beta, part, 0.2, pg_out=(out[0], out[1]))
        return dg, db, da
    return (_nan(Cm), _nan(Cm)), call


def _b16(shape, seed):
    return kc16.to_blocked(kc16._r16(kc16._rand(*shape, seed=seed))).to(DEV)


def _bn16_bwd_case(shape, sign, fused, nseg=1):
    """ops16.bn_bwd with dgamma / dbeta into pg_out — functional16 passes FlatAdam's slab views there.  sign: "mask",
    "saved" (the bf16 output) or "recompute" (from x and beta); fused: bf16_bn_fused.hip or the three-launch form, which
    runs a segmented batch as nseg calls and ADDS the later segments' sums onto the destination"""
    ops, ops16, _ = _mods()
    B, C, H, W = shape
    L = ops._lib.load()
    assert L.sivae_bf16_bn_bwd_fused_seg_supported(B, C, H, W, B // nseg) == 1  # (so that the switch decides the form)
    x, r, dy = _b16(shape, 1), _b16(shape, 2), _b16(shape, 3)
    gamma, beta = _t(C, seed=7) * 0.5 + 1.0, _t(C, seed=8) * 0.2
    mean = torch.cat([_t(C, seed=20 + g) * 0.3 for g in range(nseg)])
    invstd = torch.cat([_t(C, seed=30 + g).abs() + 0.5 for g in range(nseg)])
    y, _, mask = ops16.bn_apply_act(x, r, mean, invstd, gamma, beta, C, want_full=True, want_mask=True, nseg=nseg)
    src = {"mask": mask, "saved": y, "recompute": None}[sign]

    def call(out):
        with _Switch(BN_FUSED=fused):
            dx, dz, dg, db = ops16.bn_bwd(dy, src, x, mean, invstd, gamma, beta, C, want_dz=sign != "recompute",
                                          pg_out=(out[0], out[1]), nseg=nseg)
        return (dg, db, dx) + (() if dz is None else (dz,))
    return (_nan(C), _nan(C)), call


def _conv16_case(shape, accumulate, pool):
    """ops16.conv2d / conv2d_pool into a blocked bf16 destination"""
    ops16 = _mods()[1]
    B, Ci, Co, H, W, ks = shape
    w = kc16._rand(Co, Ci, ks, ks, seed=2, scale=1.0 / (Ci * 9) ** 0.5).float().to(DEV)
    if pool:  # the data gradient of a conv of an upsampled input: dy [B, Co] -> 2x2 block sums [B, Ci, H/2, W/2]
        wp, src, oshape = ops16.PackedW16(w, 1), _b16((B, Co, H, W), 4), (B, Ci, H // 2, W // 2)
        run = lambda out: ops16.conv2d_pool(src, wp, Co, Ci, out=out, accumulate=accumulate)  # noqa: E731
    else:
        wp, src, oshape = ops16.PackedW16(w, 0), _b16((B, Ci, H, W), 1), (B, Co, H, W)
        run = lambda out: ops16.conv2d(src, wp, Ci, Co, ks, out=out, accumulate=accumulate)  # noqa: E731
    init = _b16(oshape, 6) if accumulate else _nan(oshape[0], ops16.cblocks(oshape[1]), oshape[2], oshape[3], 8,
                                                    dtype=torch.bfloat16)
    return (init,), lambda out: (run(out[0]),)


def _wgrad16_case(shape):
    ops16 = _mods()[1]
    B, Ci, Co, H, W, ks = shape
    x, dy = _b16((B, Ci, H, W), 1), _b16((B, Co, H, W), 4)
    return (_nan(Co, Ci, ks, ks),), lambda out: (ops16.conv2d_wgrad(x, dy, Ci, Co, ks, out=out[0]),)


DIRECT3, WINO_WG, UP, ONE, FIVE = (5, 16, 32, 8, 8, 3), (2, 8, 8, 12, 20, 3), (2, 8, 16, 20, 36, 3), (3, 100, 40, 8, 8, 1), \
    (2, 20, 130, 8, 8, 5)
EDGE, LINEAR, BF16, BN, BN_EVEN = (2, 40, 3, 12, 20), (7, 100, 36), (2, 24, 16, 12, 20, 3), (3, 7, 7, 7), (3, 8, 8, 16)
# the one-launch BatchNorm backward takes power-of-two maps: one plane set per block (8 x 16) and the persistent
# half-grids with a grid barrier (64 x 64); both from check_bn_bwd_fused's list
BN_P2, BN_P2_BIG, BN16 = (8, 8, 8, 16), (4, 24, 64, 64), (4, 64, 16, 16)
# conv2d_up_dgrad's other three tile / K-split forms: Ws >= 32 with N <= 64, N > 64 with Ws < 32, N > 64 with Ws >= 32
UP_W32, UP_N130, UP_N72_W32 = (2, 64, 128, 16, 64, 3), (2, 130, 20, 16, 32, 3), (1, 72, 8, 16, 64, 3)
UP_POOL = (8, 16, 16, 128, 128, 3)  # (the F(4x4,3x3) pooled data gradient pays from one work item per CU)
SLAB_CASES = {
    "conv2d_fwd direct 3x3": lambda: _conv_fwd_case(DIRECT3, False),
    "conv2d_fwd direct 3x3 accumulate": lambda: _conv_fwd_case(DIRECT3, True),
    "conv2d_fwd 1x1": lambda: _conv_fwd_case(ONE, False),
    "conv2d_fwd 1x1 accumulate": lambda: _conv_fwd_case(ONE, True),
    "conv2d_fwd 5x5": lambda: _conv_fwd_case(FIVE, False),
    "conv2d_wgrad direct 3x3": lambda: _conv_wgrad_case(DIRECT3, "direct_wgrad", WINO_WGRAD=False),
    "conv2d_wgrad F(2x2)": lambda: _conv_wgrad_case(WINO_WG, "wino_wgrad"),
    "conv2d_wgrad F(4x4)": lambda: _conv_wgrad_case((1, 32, 64, 16, 16, 3), "wino4_wgrad", WINO4_FORCE=True),
    "conv2d_wgrad F(4x4) grid": lambda: _conv_wgrad_case((4, 64, 64, 4, 4, 3), "wino4_wgrad", WINO4_FORCE=True),
    "conv2d_wgrad upsample": lambda: _conv_wgrad_case(UP, "wino_up_wgrad", upsample=True),
    "conv2d_wgrad 1x1": lambda: _conv_wgrad_case(ONE, "direct_wgrad"),
    "conv2d_wgrad 5x5": lambda: _conv_wgrad_case(FIVE, "direct_wgrad"),
    "conv2d_up_dgrad": lambda: _up_dgrad_case(UP, False),
    "conv2d_up_dgrad accumulate": lambda: _up_dgrad_case(UP, True),
    "conv2d_up_dgrad Ws32": lambda: _up_dgrad_case(UP_W32, False),
    "conv2d_up_dgrad N130 accumulate": lambda: _up_dgrad_case(UP_N130, True),
    "conv2d_up_dgrad N72 Ws32": lambda: _up_dgrad_case(UP_N72_W32, False),
    "conv2d_up_dgrad wp1": lambda: _up_dgrad_pool_case(UP_POOL, False),
    "conv2d_up_dgrad wp1 accumulate": lambda: _up_dgrad_pool_case(UP_POOL, True),
    "conv5_edge_wgrad small Co": lambda: _conv5_edge_case(EDGE, True),
    "conv5_edge_wgrad small Ci": lambda: _conv5_edge_case(EDGE, False),
    "linear_wgrad": lambda: _linear_wgrad_case(LINEAR),
    "bn_apply_act": lambda: _bn_apply_case(BN),
    "channel_sum": lambda: _channel_sum_case(BN),
    "bn_bwd saved fused": lambda: _bn_bwd_case(BN_P2, "saved", True),
    "bn_bwd saved fused persistent": lambda: _bn_bwd_case(BN_P2_BIG, "saved", True),
    "bn_bwd saved three-launch": lambda: _bn_bwd_case(BN, "saved", False),
    "bn_bwd recompute fused": lambda: _bn_bwd_case(BN_P2, "recompute", True),
    "bn_bwd recompute three-launch": lambda: _bn_bwd_case(BN, "recompute", False),
    "bn_bwd_dzsum fused": lambda: _bn_bwd_case(BN_EVEN, "dzsum", True),
    "bn_bwd_dzsum three-launch": lambda: _bn_bwd_case(BN_EVEN, "dzsum", False),
    "bn_bwd_signmask fused": lambda: _bn_bwd_case(BN_EVEN, "signmask", True),
    "bn_bwd_signmask three-launch": lambda: _bn_bwd_case(BN_EVEN, "signmask", False),
    "bn_bwd_from_partials": lambda: _bn_from_partials_case((2, 24, 16, 12, 20, 3)),
    "ops16.bn_bwd mask fused": lambda: _bn16_bwd_case(BN16, "mask", True),
    "ops16.bn_bwd mask three-launch": lambda: _bn16_bwd_case(BN16, "mask", False),
    "ops16.bn_bwd saved fused": lambda: _bn16_bwd_case(BN16, "saved", True),
    "ops16.bn_bwd saved three-launch": lambda: _bn16_bwd_case(BN16, "saved", False),
    "ops16.bn_bwd recompute fused": lambda: _bn16_bwd_case(BN16, "recompute", True),
    "ops16.bn_bwd recompute three-launch": lambda: _bn16_bwd_case(BN16, "recompute", False),
    "ops16.bn_bwd mask fused nseg2": lambda: _bn16_bwd_case(BN16, "mask", True, nseg=2),
    "ops16.bn_bwd mask three-launch nseg2": lambda: _bn16_bwd_case(BN16, "mask", False, nseg=2),
    "ops16.conv2d": lambda: _conv16_case(BF16, False, False),
    "ops16.conv2d accumulate": lambda: _conv16_case(BF16, True, False),
    "ops16.conv2d_pool": lambda: _conv16_case(BF16, False, True),
    "ops16.conv2d_pool accumulate": lambda: _conv16_case(BF16, True, True),
    "ops16.conv2d_wgrad": lambda: _wgrad16_case(BF16),
}


@pytest.mark.parametrize("name", list(SLAB_CASES), ids=[n.replace(" ", "_") for n in SLAB_CASES])
def test_slab_view_destination(name):
    """the destination 0, 1, 2, 3 elements behind a 512-byte boundary, 0xFF on both sides of it"""
    ops, ops16, _ = _mods()
    with guarded(ops, ops16) as g:
        init, call, other = (SLAB_CASES[name]() + (None,))[:3]
        fresh = call(tuple(t.clone() for t in init))
        assert all(bool(torch.isfinite(t.float()).all()) for t in fresh), "%s: non-finite values in a fresh destination" % name
        problems = []
        for k in range(4):
            dst = tuple(g.place(t, offset_elems=k) for t in init)
            got = call(dst)
            assert all(o.data_ptr() == d.data_ptr() for o, d in zip(got, dst))
            if other is not None and any(d.data_ptr() & 7 for d in dst):
                # (a destination that legitimately takes another kernel: the case's fp64 reference at its check's tolerance)
                err = kc._err(got[0], other["ref"])
                if not err <= other["tol"]:
                    problems.append("offset %d: error %.3e against fp64 over the tolerance %.1e" % (k, err, other["tol"]))
                got = ()
            for i, (a, b) in enumerate(zip(got, fresh)):
                if not torch.equal(a, b):
                    problems.append("offset %d, result %d: differs from the fresh destination (max |diff| %.3e, %d "
                                    "non-finite)" % (k, i, float((a.float() - b.float()).abs().nan_to_num(0.0).max()),
                                                     int((~torch.isfinite(a.float())).sum())))
            damage = g.verify()
            if damage:
                problems.append("offset %d: guard damage\n%s" % (k, describe(damage)))
        assert not problems, "%s:\n%s" % (name, "\n".join(problems))


# ------------------------------------------------------------------------------------------------ c. point clouds
PC_B, PC_M, PC_C = 3, 70, 5
PC_N = [131, 132]  # N & 3 != 0: the scalar kernels; N & 3 == 0 on 16-byte-aligned tensors: the vector ones


def _pc_guard():
    ops, _, pointcloud = _mods()
    return pointcloud, guarded(pointcloud, ops)


def _intact(g):
    damage = g.verify()
    assert not damage, "guard damage:\n%s" % describe(damage)


@pytest.mark.parametrize("N", PC_N)
def test_guarded_chamfer(N):
    PC, ctx = _pc_guard()
    g_ = torch.Generator().manual_seed(N)
    gts = torch.rand(PC_B, N, 3, generator=g_, dtype=torch.float64).float()
    preds = torch.rand(PC_B, PC_M, 3, generator=g_, dtype=torch.float64).float()
    w = torch.rand(PC_B, generator=g_) + 0.5
    P = O.pairwise_sqdist(preds.double(), gts.double())
    want = P.min(dim=1)[0].sum(1) + P.min(dim=2)[0].sum(1)
    with ctx as g:
        p, q = preds.to(DEV), gts.to(DEV)
        loss, idx_p, idx_g = PC.chamfer_fwd(p, q)
        dp, dg = PC.chamfer_bwd(w.to(DEV), p, q, idx_p, idx_g, True, True)
        _intact(g)
    assert bool(torch.isfinite(loss).all()) and float(((loss.double().cpu() - want).abs() / want).max()) <= 1e-5
    ip, ig = idx_p.cpu().long(), idx_g.cpu().long()
    assert ip.min() >= 0 and ip.max() < N and ig.min() >= 0 and ig.max() < PC_M
    d_p, d_g = P.gather(1, ip[:, None, :])[:, 0, :], P.gather(2, ig[:, :, None])[:, :, 0]
    m_p, m_g = P.min(dim=1)[0], P.min(dim=2)[0]
    assert max(float(((d_p - m_p) / m_p.clamp_min(1e-300)).max()), float(((d_g - m_g) / m_g.clamp_min(1e-300)).max())) <= 1e-5
    rp, rg = O.chamfer_grads_from_indices(w.double(), preds.double(), gts.double(), ip, ig)
    for got, ref in ((dp, rp), (dg, rg)):
        assert bool(torch.isfinite(got).all())
        assert float((got.double().cpu() - ref).abs().max() / ref.abs().max()) <= 1e-5


@pytest.mark.parametrize("N", PC_N)
def test_guarded_relu_bn_and_max_points(N):
    PC, ctx = _pc_guard()
    B, C = PC_B, PC_C
    g_ = torch.Generator().manual_seed(100 + N)
    a = torch.randn(B, C, N, generator=g_)
    a[torch.rand(B, C, N, generator=g_) < 0.1] = 0.0
    a[:, 0] = -a[:, 0].abs() - 0.1  # (a channel that is dead everywhere)
    gamma, beta = torch.rand(C, generator=g_) + 0.5, torch.rand(C, generator=g_) - 0.5
    dy = torch.randn(B, C, N, generator=g_)
    rm0, rv0 = torch.rand(C, generator=g_) * 0.2 - 0.1, torch.rand(C, generator=g_) + 0.5
    a64, g64, b64 = (t.double().requires_grad_(True) for t in (a, gamma, beta))
    y64, rm64, rv64 = O.relu_bn(a64, g64, b64, rm0.double(), rv0.double(), True)
    (y64 * dy.double()).sum().backward()
    x = torch.randn(B, C, N, generator=g_)
    x[0, 1] = 0.25           # an all-equal channel: index 0 wins
    x[1, 2, 37] = x[1, 2, 5] = 9.0
    gy = torch.randn(B, C, generator=g_)
    with ctx as g:
        ad, rm, rv = a.to(DEV), rm0.to(DEV), rv0.to(DEV)
        nbt = torch.tensor(3, dtype=torch.int64, device=DEV)
        mean, invstd = PC.relu_bn_stats(ad, rm, rv, nbt)
        y = PC.relu_bn_apply(ad, mean, invstd, gamma.to(DEV), beta.to(DEV))
        da, dgamma, dbeta = PC.relu_bn_bwd(dy.to(DEV), ad, mean, invstd, gamma.to(DEV))
        vals, arg = PC.max_points_fwd(x.to(DEV))
        dx = PC.max_points_bwd(gy.to(DEV), arg, N)
        _intact(g)
    figs = dict(y=viol(y, y64), rm=viol(rm, rm64), rv=viol(rv, rv64), da=viol(da, a64.grad),
                dgamma=viol(dgamma, g64.grad), dbeta=viol(dbeta, b64.grad))
    assert all(v <= 1.0 for v in figs.values()), figs
    assert int(nbt) == 4 and bool((da[ad == 0] == 0).all()) and bool((da[:, 0] == 0).all())
    want = x.max(dim=2)[0]
    first = torch.where(x == want[:, :, None], torch.arange(N)[None, None, :], N).min(dim=2)[0]
    assert torch.equal(vals.cpu(), want) and torch.equal(arg.cpu().long(), first)
    assert torch.equal(dx.cpu(), torch.zeros(B, C, N).scatter_(2, first[:, :, None], gy[:, :, None]))


@pytest.mark.parametrize("N", PC_N)
def test_guarded_pointwise_conv(N):
    PC, ctx = _pc_guard()
    B, Ci, Co = PC_B, PC_C, 7
    g_ = torch.Generator().manual_seed(200 + N)
    x, w = torch.randn(B, Ci, N, generator=g_), torch.randn(Co, Ci, 1, generator=g_) / math.sqrt(Ci)
    b, dy = torch.randn(Co, generator=g_), torch.randn(B, Co, N, generator=g_)
    runs = {}
    for dt in (torch.float64, torch.float32):
        leaves = [t.clone().to(dt).requires_grad_(True) for t in (x, w, b)]
        yr = torch.relu(torch.einsum("oc,bcn->bon", leaves[1][:, :, 0], leaves[0]) + leaves[2][None, :, None])
        (yr * dy.to(dt)).sum().backward()
        runs[dt] = (yr, leaves)
    y64, l64 = runs[torch.float64]
    with ctx as g:
        ld = [t.to(DEV).requires_grad_(True) for t in (x, w, b)]
        y = PC.pointwise_conv(ld[0], ld[1], ld[2], relu=True)
        (y * dy.to(DEV)).sum().backward()
        _intact(g)
    assert viol(y, y64) <= 1.0 and viol(ld[0].grad, l64[0].grad) <= 1.0
    for got, ref, r32 in zip(ld[1:], l64[1:], runs[torch.float32][1][1:]):  # (test_pointcloud_gpu._grad_report's gate)
        assert bool(torch.isfinite(got.grad).all())
        assert O.rel_l2(got.grad, ref.grad) <= max(4 * O.rel_l2(r32.grad, ref.grad), 1e-5)


@pytest.mark.parametrize("N", PC_N)
def test_guarded_jsd_metric(N):
    """counters are integers: equality, on points whose nearest centre float32 can tell from the second nearest"""
    PC, ctx = _pc_guard()
    rng = np.random.Generator(np.random.PCG64(N))
    x = ((rng.random(size=(PC_B, N, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.1)).astype(np.float32)
    for clip in (False, True):
        x[JO.occupancy(x, JO.grid(8, clip)[0])[2] < JO.GAP] = 0.01
    x2 = np.ascontiguousarray(x[::-1] * np.float32(0.7))
    for clip in (False, True):
        for pts in (x, x2):
            assert JO.occupancy(pts, JO.grid(8, clip)[0])[2].min() >= JO.GAP
    with ctx as g:
        xd, x2d = torch.from_numpy(x).to(DEV), torch.from_numpy(x2).to(DEV)
        got = {}
        for clip in (False, True):
            got[clip] = (PC.occupancy_grid(xd, 8, clip), PC.occupancy_grid(x2d, 8, clip, want_bernoulli=False))
        hist = PC.voxel_histogram(xd, 8)
        jsd = PC.js_divergence(got[True][0][0], got[True][1][0])
        jsd_h = PC.js_divergence(hist, PC.voxel_histogram(x2d, 8).double())
        _intact(g)
    for clip in (False, True):
        cells = JO.grid(8, clip)[0]
        c1, b1, _ = JO.occupancy(x, cells)
        (c, b), (c2, none) = got[clip]
        assert none is None and np.array_equal(c.cpu().numpy(), c1) and np.array_equal(b.cpu().numpy(), b1)
        assert np.array_equal(c2.cpu().numpy(), JO.occupancy(x2, cells)[0])
    assert np.array_equal(hist.cpu().numpy(), JO.voxel_distribution(x, 8))
    cells = JO.grid(8, True)[0]
    assert abs(float(jsd) - JO.js_divergence(JO.occupancy(x, cells)[0], JO.occupancy(x2, cells)[0])) <= 1e-10
    assert abs(float(jsd_h) - JO.js_divergence(JO.voxel_distribution(x, 8), JO.voxel_distribution(x2, 8))) <= 1e-10
