"""Characterisation of the fp32 dispatch of sivae_hip.ops, recorded without a GPU.

The public launch functions (conv2d_fwd, conv2d_wgrad, conv2d_up_dgrad, conv2d_dgrad_bnbwd, bn_bwd, bn_bwd_signmask,
bn_bwd_dzsum) are driven with device="meta" tensors while the helpers every launch goes through are replaced:
`ops._lib.call` by a recorder, `ops._require` by a no-op, `ops._p` by "null / non-null", `ops._s` by a constant,
`ops.workspace` / `ops.counters` / `ops.bn_fused_state` by meta-tensor allocators, `ops.TIMER` by a fake timer.  Only
library predicates run (they need no device: without one sivae_num_cus() answers 256, the MI355X's count).

A case's record is, in order: every C entry point called with its scalar arguments and the null ("-") / non-null ("p")
pattern of its pointer arguments, the timer key with `flops` and `executed`, and the shapes of the returned tensors —
or, for a combination the code refuses, the exception type and message (sivae_pack_* calls made before a refusal are
dropped: packing a weight before refusing the call is not behaviour anyone relies on).

The module patches only names that are part of the package's surface, so the same file records any commit:

    python tests/conv_routes.py            # writes tests/golden/conv_routes_fp32.json.gz

The committed fixture was recorded on the commit that folded the per-variant fp32 BatchNorm entry points into the general
ones (bn_bwd_route families bn_fused / bn_sync / bn_seg).
tests/test_conv_routes_host.py replays it in-process and compares with the committed fixture.

The bf16 mode (sivae_hip.ops16: conv2d, conv2d_pool, conv2d_wgrad, bn_bwd) is recorded the same way, under its own switch
variants (ops16.POOL_DGRAD, ops.BN_FUSED, SIVAE_DP_SAME_DEVICE, ops.SYNC_BN), into a second fixture:

    python tests/conv_routes.py --bf16     # writes tests/golden/conv_routes_bf16.json.gz

That fixture was recorded on the last commit whose ops16 launch functions still chose the entry point inline
("pointcloud.hip: one definition per shared ReLU-BatchNorm/max expression"), before ops16 got route functions.
"""
import contextlib
import gzip
import json
import os
import sys

import torch

for _d in (os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "soft-intro-vae-pytorch_amd"),):
    _d = os.path.abspath(_d)
    if _d not in sys.path:
        sys.path.insert(0, _d)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes_fp32.json.gz")

# every switch of the dispatch, set explicitly (the recording must not depend on SIVAE_* variables of the environment)
SWITCHES = dict(WINO=True, WINO_UP=True, WINO4=True, WINO4_B6=False, WINO4_B6_MINC=16, WINO4_B6_PRO=True,
                WINO4_MAXC=512, WINO4_WGRAD=True, WINO4_FORCE=False, WINO4_SPLITK=True, WINO4_SMALL=True,
                WINO4_SMALL_FORCE=False, WINO4_UP_SMALL=True, WINO4_DGRAD_POOL=True, WINO4_PRO=True,
                FUSE_BN_BWD=False, WINO_WGRAD=True, CONV1_STREAM=True, CONV5_K75=True, SIGNMASK=True, BN_FUSED=True,
                BN_FUSED_FINALIZE=False, SYNC_BN=None)


def _sync_stub(sums):
    return 2  # (world size; the sums stay as they are)


# (name, switch overrides, SIVAE_DP_SAME_DEVICE): "default" records the full case table, the others a thinned one
VARIANTS = [("default", {}, "0"), ("WINO=0", dict(WINO=False), "0"),
            ("WINO4=0", dict(WINO4=False, WINO4_WGRAD=False), "0"), ("WINO4_FORCE=1", dict(WINO4_FORCE=True), "0"),
            ("WINO4_SMALL=0", dict(WINO4_SMALL=False), "0"), ("WINO4_SMALL_FORCE=1", dict(WINO4_SMALL_FORCE=True), "0"),
            ("WINO4_UP_SMALL=0", dict(WINO4_UP_SMALL=False), "0"), ("WINO4_SPLITK=0", dict(WINO4_SPLITK=False), "0"),
            ("WINO4_PRO=0", dict(WINO4_PRO=False), "0"), ("WINO4_DGRAD_POOL=0", dict(WINO4_DGRAD_POOL=False), "0"),
            ("WINO4_B6=1", dict(WINO4_B6=True), "0"), ("WINO_UP=0", dict(WINO_UP=False), "0"),
            ("WINO_WGRAD=0", dict(WINO_WGRAD=False), "0"), ("CONV1_STREAM=0", dict(CONV1_STREAM=False), "0"),
            ("CONV5_K75=0", dict(CONV5_K75=False), "0"), ("FUSE_BN_BWD=1", dict(FUSE_BN_BWD=True), "0"),
            ("BN_FUSED=0", dict(BN_FUSED=False), "0"), ("BN_FUSED_FINALIZE=1", dict(BN_FUSED_FINALIZE=True), "0"),
            ("SIVAE_DP_SAME_DEVICE=1", {}, "1"), ("SYNC_BN", dict(SYNC_BN=_sync_stub), "0")]


# ---- recorder --------------------------------------------------------------------------------------------------------
class _Ptr:
    pass


_PTR, _STREAM = _Ptr(), _Ptr()


def _enc(a):
    if a is None:
        return "-"
    if a is _PTR:
        return "p"
    if a is _STREAM:
        return "s"
    if isinstance(a, bool):
        return int(a)
    if isinstance(a, (int, float)):
        return a
    raise TypeError("conv_routes: unexpected argument %r in a C-ABI call" % (a,))


class _FakeTimer:
    def __init__(self, events):
        self.events = events

    def begin(self):
        return self

    def end(self, key, flops, start, executed=None):
        assert start is self
        self.events.append(["timer", key, flops, flops if executed is None else executed])


class _Mask:
    """stands for the uint8 device sign mask bn_apply_act_signmask returns (a meta tensor is not `is_cuda`)"""
    dtype = torch.uint8
    is_cuda = True

    def numel(self):
        return 1 << 40


class _MaskOf(_Mask):
    """_Mask with the size of the meta tensor it stands for (ops16.bn_bwd checks it, and slices it per segment)"""

    def __init__(self, t):
        self.n = t.numel()

    def numel(self):
        return self.n

    def __getitem__(self, sl):
        return self


def M(*shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device="meta")


@contextlib.contextmanager
def recording(switches=None, same_device="0", pool_dgrad=True):
    """patch sivae_hip.ops as the module docstring says, and sivae_hip.ops16 likewise (it binds `_p` / `_s` at import and
    has its own `_req16` and one switch, POOL_DGRAD); yields (ops, events) — `events` is the list the recorder appends
    to (clear it between cases)"""
    from sivae_hip import ops, ops16
    events = []
    saved16 = {n: getattr(ops16, n) for n in ("_p", "_s", "_req16", "POOL_DGRAD")}
    names = list(SWITCHES) + ["_require", "_p", "_s", "workspace", "counters", "bn_fused_state", "TIMER"]
    saved = {n: getattr(ops, n) for n in names}
    saved_call = ops._lib.call
    saved_env = os.environ.get("SIVAE_DP_SAME_DEVICE")
    try:
        for n, v in dict(SWITCHES, **(switches or {})).items():
            setattr(ops, n, v)
        os.environ["SIVAE_DP_SAME_DEVICE"] = same_device
        ops._require = lambda *tensors: None
        ops._p = lambda t: None if t is None else _PTR
        ops._s = lambda t=None: _STREAM
        ops.workspace = lambda nbytes, device: torch.empty(int(nbytes), dtype=torch.uint8, device="meta")
        ops.counters = lambda device: torch.empty(8192, dtype=torch.int32, device="meta")
        ops.bn_fused_state = lambda device: torch.empty(64, dtype=torch.int32, device="meta")
        ops.TIMER = _FakeTimer(events)
        ops._lib.call = lambda name, *args: events.append(["call", name] + [_enc(a) for a in args])
        ops16._p, ops16._s, ops16._req16, ops16.POOL_DGRAD = ops._p, ops._s, ops._require, pool_dgrad
        yield ops, events
    finally:
        ops._lib.call = saved_call
        for n, v in saved16.items():
            setattr(ops16, n, v)
        for n, v in saved.items():
            setattr(ops, n, v)
        if saved_env is None:
            os.environ.pop("SIVAE_DP_SAME_DEVICE", None)
        else:
            os.environ["SIVAE_DP_SAME_DEVICE"] = saved_env


# ---- runners: one public call per case -------------------------------------------------------------------------------
def _pro(C, nseg):
    return (M(nseg * C), M(nseg * C), M(C), M(C), 0.2)


def run_fwd(ops, B, Ci, Co, H, W, ks, packed=True, mode=0, bias=False, pro=False, upsample=False, want_stats=False,
            has_out=False, accumulate=False, nseg=1):
    x = M(B, Ci, H // 2, W // 2) if upsample else M(B, Ci, H, W)
    w = M(Co, Ci, ks, ks) if mode == 0 else M(Ci, Co, ks, ks)
    wp = ops.PackedW(w, mode) if packed else ops.pack_weight(w, mode)
    return ops.conv2d_fwd(x, wp, Co, ks, bias=M(Co) if bias else None, pro=_pro(Ci, nseg) if pro else None,
                          upsample=upsample, want_stats=want_stats, out=M(B, Co, H, W) if has_out else None,
                          accumulate=accumulate, nseg=nseg)


def run_wgrad(ops, B, Ci, Co, H, W, ks, pro=False, upsample=False, has_out=False, nseg=1):
    x = M(B, Ci, H // 2, W // 2) if upsample else M(B, Ci, H, W)
    return ops.conv2d_wgrad(x, M(B, Co, H, W), ks, pro=_pro(Ci, nseg) if pro else None, upsample=upsample,
                            out=M(Co, Ci, ks, ks) if has_out else None, nseg=nseg)


def run_up_dgrad(ops, B, C, N, H, W, has_wp1=False, has_out=False, accumulate=False):
    w = M(C, N, 3, 3)
    return ops.conv2d_up_dgrad(M(B, C, H, W), ops.PackedW(w, 0), N, out=M(B, N, H // 2, W // 2) if has_out else None,
                               accumulate=accumulate, wp1=ops.PackedW(w, 1) if has_wp1 else None)


def run_dgrad_bnbwd(ops, B, Ci, Cm, H, W):
    return ops.conv2d_dgrad_bnbwd(M(B, Ci, H, W), ops.PackedW(M(Ci, Cm, 3, 3), 1), Cm, M(B, Cm, H, W), M(Cm), M(Cm),
                                  M(Cm), M(Cm))


def run_bn_bwd(ops, B, C, H, W, act=1, want_dz=False, dy_pooled=False, has_pg_out=False, nseg=1, flat=False):
    x = M(B, C) if flat else M(B, C, H, W)
    dy = M(B, C, H // 2, W // 2) if dy_pooled else torch.empty_like(x)
    return ops.bn_bwd(dy, torch.empty_like(x) if act == 1 else None, x, M(nseg * C), M(nseg * C), M(C),
                      want_dz=want_dz, beta=M(C) if act == 2 else None, act_mode=act, dy_pooled=dy_pooled,
                      pg_out=(M(C), M(C)) if has_pg_out else None, nseg=nseg)


def run_bn_signmask(ops, B, C, H, W, dy_pooled=False, dz_sum=False, want_dz=True, nseg=1):
    x = M(B, C, H, W)
    dy = M(B, C, H // 2, W // 2) if dy_pooled else torch.empty_like(x)
    return ops.bn_bwd_signmask(dy, _Mask(), x, M(nseg * C), M(nseg * C), M(C), dy_pooled=dy_pooled, dz_sum=dz_sum,
                               want_dz=want_dz, nseg=nseg)


def run_bn_dzsum(ops, B, C, H, W, nseg=1):
    x = M(B, C, H, W)
    return ops.bn_bwd_dzsum(torch.empty_like(x), torch.empty_like(x), x, M(nseg * C), M(nseg * C), M(C), nseg=nseg)


# the bf16 mode (sivae_hip.ops16): blocked bf16 activations [B, C16/8, H, W, 8]; H, W are the OUTPUT map of a conv
def X(B, C, H, W):
    return M(B, ((C + 15) // 16) * 2, H, W, 8, dtype=torch.bfloat16)


class _WP16:
    """stands for a PackedW16 (the launches only take its buffer's address)"""
    data = M(8, dtype=torch.bfloat16)


def run_conv16(ops, B, Ci, Co, H, W, ks, bias=False, pro=False, upsample=False, want_stats=False, has_out=False,
               accumulate=False, out_f32=False):
    from sivae_hip import ops16
    out = (M(B, Co, H, W) if out_f32 else X(B, Co, H, W)) if has_out else None
    return ops16.conv2d(X(B, Ci, H // 2, W // 2) if upsample else X(B, Ci, H, W), _WP16, Ci, Co, ks,
                        bias=M(Co) if bias else None, pro=_pro(Ci, 1) if pro else None, upsample=upsample,
                        want_stats=want_stats, out=out, accumulate=accumulate, out_f32=out_f32)


def run_pool16(ops, B, Ci, Co, H, W, has_out=False, accumulate=False):
    from sivae_hip import ops16
    return ops16.conv2d_pool(X(B, Ci, H, W), _WP16, Ci, Co, out=X(B, Co, H // 2, W // 2) if has_out else None,
                             accumulate=accumulate)


def run_wgrad16(ops, B, Ci, Co, H, W, ks, pro=False, upsample=False, has_out=False):
    from sivae_hip import ops16
    out = M(*((Co, Ci, 5, 1) if ks == ops16.KS51 else (Co, Ci, ks, ks))) if has_out else None
    return ops16.conv2d_wgrad(X(B, Ci, H // 2, W // 2) if upsample else X(B, Ci, H, W), X(B, Co, H, W), Ci, Co, ks,
                              pro=_pro(Ci, 1) if pro else None, upsample=upsample, out=out)


def run_bn_bwd16(ops, B, C, H, W, y="saved", dy_pooled=False, want_dz=False, dz_sum=False, has_pg_out=False, nseg=1):
    """y: the sign comes from the "saved" output, from the uint8 "mask", or ("none") is recomputed from x"""
    from sivae_hip import ops16
    x = X(B, C, H, W)
    src = {"saved": torch.empty_like(x), "mask": _MaskOf(M(*x.shape[:4], dtype=torch.uint8)), "none": None}[y]
    return ops16.bn_bwd(X(B, C, H // 2, W // 2) if dy_pooled else torch.empty_like(x), src, x, M(nseg * C), M(nseg * C),
                        M(C), M(C), C, dy_pooled=dy_pooled, want_dz=want_dz, dz_sum=dz_sum,
                        pg_out=(M(C), M(C)) if has_pg_out else None, nseg=nseg)


RUNNERS = dict(fwd=run_fwd, wgrad=run_wgrad, up_dgrad=run_up_dgrad, dgrad_bnbwd=run_dgrad_bnbwd, bn_bwd=run_bn_bwd,
               bn_signmask=run_bn_signmask, bn_dzsum=run_bn_dzsum, conv16=run_conv16, pool16=run_pool16,
               wgrad16=run_wgrad16, bn_bwd16=run_bn_bwd16)


def _shapes(r):
    if r is None:
        return None
    if isinstance(r, (tuple, list)):
        return [_shapes(t) for t in r]
    return list(r.shape)


def record_case(ops, events, kind, params):
    del events[:]
    try:
        ret = RUNNERS[kind](ops, **params)
    except Exception as e:  # noqa: BLE001  (a refusal is part of the behaviour recorded)
        return [ev for ev in events if not (ev[0] == "call" and ev[1].startswith("sivae_pack_"))] + [
            ["raise", type(e).__name__, str(e)]]
    return list(events) + [["ret", _shapes(ret)]]


def case_name(kind, params):
    return kind + " " + " ".join("%s=%s" % (k, int(v) if isinstance(v, bool) else v) for k, v in params.items())


# ---- case table ------------------------------------------------------------------------------------------------------
MAPS = (4, 8, 16, 32, 64, 128, 256)
CH = (16, 32, 64, 128, 256, 512)


def _skip(S, *chans):
    return S >= 128 and max(chans) > 128


def table_cases(thin):
    """[(kind, params)] of the generated table; thin: the smaller table of the switch variants"""
    out = []
    batches = (128, 16) if thin else (128, 64, 16, 8, 2, 3)
    if thin:
        pairs = [(16, 16), (64, 64), (512, 512), (128, 64), (64, 128)]
    else:
        pairs = [(c, c) for c in CH] + [(c, 2 * c) for c in CH[:-1]] + [(2 * c, c) for c in CH[:-1]]
    # 3x3 layers
    fwd_flags = [{}, dict(mode=1), dict(pro=True), dict(want_stats=True), dict(pro=True, want_stats=True),
                 dict(upsample=True), dict(upsample=True, want_stats=True), dict(upsample=True, pro=True),
                 dict(mode=1, has_out=True, accumulate=True), dict(upsample=True, has_out=True, accumulate=True),
                 dict(has_out=True), dict(packed=False), dict(packed=False, pro=True, want_stats=True),
                 dict(bias=True), dict(nseg=2, want_stats=True), dict(nseg=2, pro=True, want_stats=True),
                 dict(nseg=2, pro=True), dict(nseg=2, upsample=True, want_stats=True), dict(nseg=2, mode=1),
                 dict(nseg=2, upsample=True, pro=True, want_stats=True), dict(nseg=2, packed=False, want_stats=True)]
    wg_flags = [{}, dict(pro=True), dict(upsample=True), dict(upsample=True, pro=True), dict(has_out=True),
                dict(nseg=2), dict(nseg=2, pro=True), dict(nseg=2, pro=True, has_out=True),
                dict(nseg=2, upsample=True)]
    for B in batches:
        for S in MAPS:
            for Ci, Co in pairs:
                if _skip(S, Ci, Co):
                    continue
                for fl in fwd_flags:
                    if fl.get("nseg", 1) > 1 and B % 2:
                        continue
                    out.append(("fwd", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=3, **fl)))
                for fl in wg_flags:
                    if fl.get("nseg", 1) > 1 and B % 2:
                        continue
                    out.append(("wgrad", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=3, **fl)))
    # non-square and odd maps the Winograd kernels refuse or tile differently
    for B in (128, 2):
        for H, W in ((8, 16), (16, 8), (6, 6), (7, 7), (32, 24), (12, 20)):
            for fl in ({}, dict(pro=True, want_stats=True), dict(upsample=True), dict(nseg=2, pro=True, want_stats=True)):
                out.append(("fwd", dict(B=B, Ci=64, Co=64, H=H, W=W, ks=3, **fl)))
            for fl in ({}, dict(pro=True), dict(upsample=True), dict(nseg=2, pro=True)):
                out.append(("wgrad", dict(B=B, Ci=64, Co=64, H=H, W=W, ks=3, **fl)))
    # 1x1 layers (ResidualBlock.conv_expand; H = W = 1: the Linear layers the small-batch GEMM does not take)
    for B in batches:
        for S in (1,) + MAPS[:-1]:
            for Ci, Co in pairs:
                if _skip(S, Ci, Co):
                    continue
                for fl in ({}, dict(mode=1), dict(bias=True), dict(mode=1, has_out=True, accumulate=True),
                           dict(packed=False), dict(want_stats=True), dict(pro=True)):
                    out.append(("fwd", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=1, **fl)))
                for fl in ({}, dict(has_out=True)):
                    out.append(("wgrad", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=1, **fl)))
    # 5x5 layers with 1 / 3 / 4 image channels on either side (encoder stem, Decoder.predict)
    for B in batches:
        for S in (32, 128, 256):
            for small in (1, 3, 4):
                for big in (16, 64, 128):
                    for Ci, Co in ((small, big), (big, small)):
                        for fl in ({}, dict(want_stats=True), dict(bias=True), dict(mode=1), dict(packed=False),
                                   dict(has_out=True), dict(nseg=2, want_stats=True)):
                            out.append(("fwd", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=5, **fl)))
                        out.append(("wgrad", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=5)))
    # data gradient of conv3x3(Upsample2(x)) to the low-resolution x; conv2's data gradient with BatchNorm-1's sums
    for B in batches:
        for S in MAPS[1:]:
            for C, N in pairs:
                if _skip(S, C, N):
                    continue
                for fl in ({}, dict(has_wp1=True), dict(has_wp1=True, has_out=True, accumulate=True),
                           dict(has_out=True, accumulate=True)):
                    out.append(("up_dgrad", dict(B=B, C=C, N=N, H=S, W=S, **fl)))
                out.append(("dgrad_bnbwd", dict(B=B, Ci=C, Cm=N, H=S, W=S)))
    # the three BatchNorm backwards
    for B in batches:
        for S in MAPS + (6,):
            for C in (16, 64, 512):
                if _skip(S, C):
                    continue
                for nseg in (1, 2):
                    if B % nseg:
                        continue
                    for fl in (dict(act=1, want_dz=True), dict(act=1, want_dz=True, dy_pooled=True), dict(act=1),
                               dict(act=2), dict(act=2, dy_pooled=True), dict(act=0), dict(act=2, has_pg_out=True)):
                        out.append(("bn_bwd", dict(B=B, C=C, H=S, W=S, nseg=nseg, **fl)))
                    for fl in ({}, dict(dy_pooled=True), dict(dz_sum=True), dict(want_dz=False)):
                        out.append(("bn_signmask", dict(B=B, C=C, H=S, W=S, nseg=nseg, **fl)))
                    out.append(("bn_dzsum", dict(B=B, C=C, H=S, W=S, nseg=nseg)))
        out.append(("bn_bwd", dict(B=B, C=512, H=1, W=1, act=0, flat=True)))
    return out


# ---- the benchmarked networks ----------------------------------------------------------------------------------------
# (bench.py: celeb256 at batch 128 and as a 16-image shard, the bootstrap variant at 256x256 with 64 and 8 images,
# cifar10 at batch 256; each unpaired and as segmented pairs)
NETWORKS = [("celeb256_bs128", [64, 128, 256, 512, 512, 512], 256, 128),
            ("celeb256_bs16", [64, 128, 256, 512, 512, 512], 256, 16),
            ("bootstrap256_bs64", [64, 128, 256, 512, 512, 512], 256, 64),
            ("bootstrap256_bs8", [64, 128, 256, 512, 512, 512], 256, 8),
            ("cifar10_bs256", [64, 128, 256], 32, 256)]


def block_cases(ops, B, Ci, Cm, Co, H, W, x_up, post, nseg, has_exp):
    """the ops-level calls of one training-mode functional.ResBlockFn forward + backward (every gradient needed,
    parameter gradients written into slabs), in its order — read off the block's plan; H, W: the block's resolution"""
    from sivae_hip import functional as SF
    plan = SF.resblock_plan(B, Ci, Cm, Co, H, W, x_up=x_up, post=post, nseg=nseg, has_exp=has_exp, training=True)
    out = []

    def add(kind, **p):
        out.append((kind, p))

    Hs, Ws = (H // 2, W // 2) if x_up else (H, W)
    if has_exp:
        add("fwd", B=B, Ci=Ci, Co=Co, H=Hs, W=Ws, ks=1)
    add("fwd", B=B, Ci=Ci, Co=Cm, H=H, W=W, ks=3, want_stats=True, upsample=x_up, nseg=nseg)
    add("fwd", B=B, Ci=Cm, Co=Co, H=H, W=W, ks=3, pro=not plan.h_saved, want_stats=True, nseg=nseg)
    if plan.bn2 == "signmask":
        add("bn_signmask", B=B, C=Co, H=H, W=W, dy_pooled=plan.dy_pooled, dz_sum=plan.dz_sum, nseg=nseg)
    elif plan.bn2 == "dzsum":
        add("bn_dzsum", B=B, C=Co, H=H, W=W, nseg=nseg)
    else:
        add("bn_bwd", B=B, C=Co, H=H, W=W, act=1, want_dz=True, dy_pooled=plan.dy_pooled, has_pg_out=True, nseg=nseg)
    add("wgrad", B=B, Ci=Cm, Co=Co, H=H, W=W, ks=3, pro=not plan.h_saved, has_out=True, nseg=nseg)
    if plan.fuse_bn1:
        add("dgrad_bnbwd", B=B, Ci=Co, Cm=Cm, H=H, W=W)
    else:
        add("fwd", B=B, Ci=Co, Co=Cm, H=H, W=W, ks=3, mode=1)
        add("bn_bwd", B=B, C=Cm, H=H, W=W, act=1 if plan.h_saved else 2, has_pg_out=True, nseg=nseg)
    add("wgrad", B=B, Ci=Ci, Co=Cm, H=H, W=W, ks=3, upsample=x_up, has_out=True)
    # the skip gradient is read at x's resolution when only its 2x2 block sums are needed
    Hz, Wz = (Hs, Ws) if plan.skip_sums else (H, W)
    if plan.skip == "expand":
        add("wgrad", B=B, Ci=Ci, Co=Co, H=Hz, W=Wz, ks=1, has_out=True)
    # conv1's data gradient: onto the skip gradient of an identity skip, unless both are reduced separately
    onto = {} if (plan.skip == "expand" or (plan.dgrad1 == "reduce" and plan.skip_sums)) else dict(has_out=True,
                                                                                                  accumulate=True)
    if plan.dgrad1 == "phase":
        add("up_dgrad", B=B, C=Cm, N=Ci, H=H, W=W, has_wp1=True, **onto)
    else:
        add("fwd", B=B, Ci=Cm, Co=Ci, H=H, W=W, ks=3, mode=1, **onto)
    if plan.skip == "expand":
        add("fwd", B=B, Ci=Co, Co=Ci, H=Hz, W=Wz, ks=1, mode=1, has_out=True, accumulate=True)
    return out


def network_cases(ops, channels, image_size, B, nseg=1, cdim=3):
    """[(layer, kind, params)]: the ops-level calls of every layer group of the fp32 Encoder and Decoder, in the order of
    nn.main_plan (the networks are built on the meta device; nothing runs)"""
    from sivae_hip import functional as SF
    from sivae_hip import nn as N
    with torch.device("meta"), contextlib.redirect_stdout(None):  # (the constructors print their shapes)
        enc = N.Encoder(cdim, 8, channels, image_size)
        dec = N.Decoder(cdim, 8, channels, image_size, conv_input_size=enc.conv_output_size)
    out = []
    for where, main, size in (("enc", enc.main, (image_size, image_size)), ("dec", dec.main, enc.conv_output_size[1:])):
        for s in N.main_plan(main, size):
            d = dict(B=B, Ci=s.Ci, Co=s.Co, H=s.H, W=s.W)
            if s.kind == "block":
                layer = "%s.block%dx%d" % (where, s.H, s.W)
                out.extend((layer, k, p) for k, p in block_cases(ops, B, s.Ci, s.Cm, s.Co, s.H, s.W, s.x_up, s.post,
                                                                 nseg, s.block.conv_expand is not None))
            elif s.kind == "stem":
                out.append((where + ".stem", "fwd", dict(d, ks=5, want_stats=True)))
                out.append((where + ".stem", "bn_bwd", dict(B=B, C=s.Co, H=s.H, W=s.W, act=2, dy_pooled=True,
                                                            has_pg_out=True, nseg=nseg)))
                if not SF.stem_edge5(s.conv.weight):
                    out.append((where + ".stem", "wgrad", dict(d, ks=5, has_out=True)))
            else:
                ks = s.conv.kernel_size[0]
                edge_fwd, edge_wgrad = SF.predict_edge5(s.conv.weight)
                if not edge_fwd:
                    out.append((where + ".predict", "fwd", dict(d, ks=ks, bias=s.conv.bias is not None)))
                if not edge_wgrad:
                    out.append((where + ".predict", "wgrad", dict(d, ks=ks, has_out=True)))
                out.append((where + ".predict", "fwd", dict(d, Ci=s.Co, Co=s.Ci, ks=ks, mode=1)))
    return out


# ---- the bf16 mode ---------------------------------------------------------------------------------------------------
FIXTURE16 = os.path.join(os.path.dirname(FIXTURE), "conv_routes_bf16.json.gz")
# (name, switch overrides of ops, SIVAE_DP_SAME_DEVICE, ops16.POOL_DGRAD): ops16 reads BN_FUSED and SYNC_BN of ops
VARIANTS16 = [("default", {}, "0", True), ("ops16.POOL_DGRAD=0", {}, "0", False),
              ("BN_FUSED=0", dict(BN_FUSED=False), "0", True), ("SIVAE_DP_SAME_DEVICE=1", {}, "1", True),
              ("SYNC_BN", dict(SYNC_BN=_sync_stub), "0", True)]
KS51 = 51  # (ops16.KS51: the 5-row x 1-column conv of the kw-packed RGB-side layers)


def table_cases16(thin):
    """[(kind, params)] of the bf16 table: one public call of ops16 each; thin: the table of the switch variants"""
    out = []
    batches = (16, 2) if thin else (128, 16, 2, 3)
    pairs = [(24, 40), (128, 64), (512, 512)] if thin else [
        (16, 16), (24, 40), (40, 24), (64, 64), (64, 128), (128, 64), (256, 256), (512, 512)]
    maps = [(S, S) for S in MAPS] + [(6, 6), (7, 7), (12, 20), (8, 16)]
    conv3 = [{}, dict(bias=True), dict(pro=True), dict(upsample=True), dict(want_stats=True),
             dict(pro=True, want_stats=True), dict(upsample=True, want_stats=True), dict(has_out=True, accumulate=True),
             dict(upsample=True, has_out=True, accumulate=True), dict(out_f32=True), dict(bias=True, out_f32=True),
             dict(bias=True, want_stats=True)]
    for B in batches:
        for H, W in maps:
            for Ci, Co in pairs:
                if _skip(max(H, W), Ci, Co):
                    continue
                for fl in conv3:
                    out.append(("conv16", dict(B=B, Ci=Ci, Co=Co, H=H, W=W, ks=3, **fl)))
                for fl in ({}, dict(has_out=True, accumulate=True), dict(bias=True), dict(want_stats=True)):
                    out.append(("conv16", dict(B=B, Ci=Ci, Co=Co, H=H, W=W, ks=1, **fl)))
                for fl in ({}, dict(has_out=True, accumulate=True)):
                    out.append(("pool16", dict(B=B, Ci=Ci, Co=Co, H=H, W=W, **fl)))
                for fl in ({}, dict(pro=True), dict(upsample=True), dict(has_out=True)):
                    out.append(("wgrad16", dict(B=B, Ci=Ci, Co=Co, H=H, W=W, ks=3, **fl)))
                for fl in ({}, dict(has_out=True)):
                    out.append(("wgrad16", dict(B=B, Ci=Ci, Co=Co, H=H, W=W, ks=1, **fl)))
    # the RGB-side 5x5 layers, plain (1 / 3 / 4 image channels) and kw-packed (5 x 3 = 15 channels, 5 x 1 taps)
    for B in batches:
        for S in (32, 128, 256):
            for ks, small in ((5, 1), (5, 3), (5, 4), (KS51, 15)):
                for big in (16, 64, 128):
                    for Ci, Co in ((small, big), (big, small)):
                        for fl in ({}, dict(want_stats=True), dict(out_f32=True), dict(bias=True, out_f32=True)):
                            out.append(("conv16", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=ks, **fl)))
                        for fl in ({}, dict(has_out=True)):
                            out.append(("wgrad16", dict(B=B, Ci=Ci, Co=Co, H=S, W=S, ks=ks, **fl)))
    bn = [dict(y="mask", want_dz=True), dict(y="mask", want_dz=True, dz_sum=True),
          dict(y="mask", dy_pooled=True, want_dz=True), dict(y="saved", want_dz=True), dict(y="saved", has_pg_out=True),
          dict(y="none"), dict(y="none", dy_pooled=True), dict(y="none", has_pg_out=True)]
    for B in batches:
        for H, W in maps:
            for C in (16, 24, 64, 512):
                if _skip(max(H, W), C):
                    continue
                for nseg in (1, 2):
                    if B % nseg == 0:
                        for fl in bn:
                            out.append(("bn_bwd16", dict(B=B, C=C, H=H, W=W, nseg=nseg, **fl)))
    return out


def production_cases16():
    """[(case name, kind, params)]: the ops16 calls at every layer shape of the benchmarked bf16 networks
    (block_checks16.PRODUCTION, unpaired and as segmented pairs) — block_checks16.walk_routes lists the convs whose
    epilogue writes statistics (the stem's and both 3x3 convs of every block); each is recorded as a forward, as the data
    gradient back through it (plain, and with the 2x2 block sum folded in), as its weight gradient and as the backward
    of the BatchNorm that follows it"""
    import block_checks16 as bc
    out = []
    for net, channels, size, B in bc.PRODUCTION:
        for nseg in (1, 2):
            convs, block_route = [], bc.block_route
            bc.block_route = lambda *a, **k: None  # (only the shapes are wanted: this file records any commit's ops16)
            try:
                with contextlib.redirect_stdout(None):  # (the constructors print their shapes)
                    bc.walk_routes(channels, size, B * nseg, nseg, convs=convs)
            finally:
                bc.block_route = block_route
            for Ci, Co, H, W, ks in dict.fromkeys(convs):
                d = dict(B=B * nseg, Ci=Ci, Co=Co, H=H, W=W)
                cases = [("conv16", dict(d, ks=ks, want_stats=True)), ("conv16", dict(d, Ci=Co, Co=Ci, ks=ks)),
                         ("wgrad16", dict(d, ks=ks, has_out=True))]
                if ks == 3:
                    cases.append(("pool16", dict(d, Ci=Co, Co=Ci)))
                for fl in (dict(y="mask", want_dz=True), dict(y="mask", dy_pooled=True, want_dz=True, dz_sum=True),
                           dict(y="none", has_pg_out=True)):
                    cases.append(("bn_bwd16", dict(B=B * nseg, C=Co, H=H, W=W, nseg=nseg, **fl)))
                out.extend(("%s nseg=%d: %s" % (net, nseg, case_name(k, p)), k, p) for k, p in cases)
    return out


def variant_cases16(vname):
    seen, out = set(), []
    for kind, p in table_cases16(thin=vname != "default"):
        name = case_name(kind, p)
        if name not in seen:
            seen.add(name)
            out.append((name, kind, p))
    return out + production_cases16()


# ---- recording -------------------------------------------------------------------------------------------------------
def variant_cases(ops, vname):
    """[(case name, kind, params)] of one switch variant (call inside `recording` of that variant: the network walk asks
    the ops module which block forms the switches allow)"""
    seen, out = set(), []
    for kind, p in table_cases(thin=vname != "default"):
        name = case_name(kind, p)
        if name not in seen:
            seen.add(name)
            out.append((name, kind, p))
    if vname == "default":
        for net, channels, size, B in NETWORKS:
            for nseg in (1, 2):
                for layer, kind, p in network_cases(ops, channels, size, B * nseg, nseg):
                    out.append(("%s nseg=%d %s: %s" % (net, nseg, layer, case_name(kind, p)), kind, p))
    return out


def generate(on_case=None, bf16=False):
    """-> {variant: [(case name, record)]} of the fp32 dispatch, or (bf16) of the bf16 mode's; on_case(ops, variant, name,
    kind, params, record) is called for every case while the variant's switches are still set"""
    out = {}
    for vname, *settings in (VARIANTS16 if bf16 else VARIANTS):
        with recording(*settings) as (ops, events):
            rows = []
            for name, kind, p in (variant_cases16(vname) if bf16 else variant_cases(ops, vname)):
                rec = record_case(ops, events, kind, p)
                rows.append((name, rec))
                if on_case is not None:
                    on_case(ops, vname, name, kind, p, rec)
            out[vname] = rows
    return out


def compact(gen):
    """{"records": [unique records], "names": [unique case-name lists], "variants": {variant: [index into names,
    [record index of each case]]}}"""
    index, records, nindex, names, variants = {}, [], {}, [], {}
    for vname, rows in gen.items():
        vr = []
        for _, rec in rows:
            key = json.dumps(rec)
            if key not in index:
                index[key] = len(records)
                records.append(rec)
            vr.append(index[key])
        nkey = tuple(name for name, _ in rows)
        if nkey not in nindex:
            nindex[nkey] = len(names)
            names.append(list(nkey))
        variants[vname] = [nindex[nkey], vr]
    return dict(records=records, names=names, variants=variants)


def expand(fixture):
    """the inverse of `compact`: {variant: [(case name, record)]}"""
    return {v: [(name, fixture["records"][i]) for name, i in zip(fixture["names"][ni], idx)]
            for v, (ni, idx) in fixture["variants"].items()}


def load_fixture(path=FIXTURE):
    with gzip.open(path, "rt", encoding="utf-8") as f:
        return json.load(f)


def write_fixture(path=FIXTURE, bf16=False):
    data = json.dumps(compact(generate(bf16=bf16)), separators=(",", ":")).encode("utf-8")
    with open(path, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
            f.write(data)
    return len(data), os.path.getsize(path)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--bf16"]
    path = args[0] if args else (FIXTURE16 if "--bf16" in sys.argv else FIXTURE)
    n, z = write_fixture(path, bf16="--bf16" in sys.argv)
    print("wrote %s: %d bytes of JSON, %d compressed" % (path, n, z))
