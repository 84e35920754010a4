"""Block-level referee of the bf16 mode: the autograd Functions of functional16.py (ResBlockFn16, StemFn16, PredictFn16) —
the glue that chains the bf16 kernels into a ResidualBlock, the encoder stem and Decoder.predict — against an fp64
evaluation of the same ops on the CPU.

The referee is written from the reference's definitions (soft_intro_vae/train_soft_intro_vae.py:38-75 ResidualBlock with
the AvgPool2d / Upsample that follows it in the nets, :88-93 the stem conv5x5 -> BN -> LeakyReLU -> AvgPool2d, :159
predict), and its backward is torch autograd: nothing of it is copied from the code under test.  It is "rounded where
stored": identity autograd ops round to bf16 (RNE, what .bfloat16() does) exactly where the HIP path stores a bf16
tensor —
  forward:  idt (conv_expand output), a = conv1, h = LeakyReLU(BN1(a)), c = conv2, the block output, the pooled output
            (bf16 weights: the packed operand slabs are the master weights rounded to bf16);
  backward: d_out after the Upsample's adjoint, dc, dz (or its 2x2 block sums when the skip was upsampled), dh, da, dx;
weight and BatchNorm-parameter gradients stay unrounded, and BatchNorm statistics are those of the rounded conv output
(the kernels take them from the stored bf16 values).  What is left between the two is the HIP path's own arithmetic —
fp32 accumulation order and the rare one-ulp flip of a stored value it causes — so the bounds are tight:
  * fp32 results (weight / gamma / beta gradients, predict output, kw-packed stem dx): max-norm relative <= 2e-3;
  * running buffers: <= 1e-5 derived, 3e-5 measured (TOL_RUN) (torch's own update: unbiased variance, momentum 0.1),
    num_batches_tracked exact;
  * bf16 forward tensors: kernel_checks16._err16 (element-wise 2^-7 |ref| + 1e-3 max|ref|); the block / stem outputs
    add the carried one-ulp flip of the stored conv output to that element-wise rule (`_err16c`, TOL_Y);
  * bf16 gradients: max-norm relative <= 1.2e-2 (kernel_checks16.check_bn's dx bound).
A LeakyReLU whose input lies within rounding of the kink may legitimately take the other side in the HIP path (its
input is computed in fp32 from values that can differ from the referee's by one ulp).  There the referee takes the
derivative's side from the HIP path's own sign (the block's saved output / sign mask for BN-2, BN-1 evaluated in fp32
on the saved conv output for BN-1), and each check reports how many elements were resolved that way ("ties") and how
many of those actually differ from the fp64 sign ("flips").

Every block case runs through sivae_hip.nn.ResidualBlock on a blocked bf16 input, the stem / predict cases through
functional16.stem / conv_bias: the real dispatch.  `block_route` / `production_routes` give the route class of a block
from the route functions of ops16 — the code that launches; tests/test_block_routes16_host.py checks that every class
the benchmarked bf16 iterations take is covered by a case here.
Used by tests/test_blocks16_gpu.py (pytest -m gpu) and `python tests/block_checks16.py [filter...]`.
"""
import os
import sys
import traceback

import torch
import torch.nn.functional as F

_here = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(os.path.dirname(_here), "soft-intro-vae-pytorch_amd"), _here):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from kernel_checks16 import _err, _err16, _padded_zero, _r16, _rand, from_blocked, to_blocked  # noqa: E402

DEV = "cuda"
SLOPE = 0.2
TOL_F32 = 2e-3
# running buffers: 1e-5 was the derived bound; measured 1.05e-5 (bn2 running_mean, "splitk exp x_up (no pooled dgrad)":
# 256 samples per channel) — one one-ulp flip of a stored conv output moves that batch mean by ulp / 256, x 0.1 momentum
TOL_RUN = 3e-5
TOL_BF16 = 6e-3    # (bf16 forward tensors: _err16's element-wise rule decides, this is its max-norm companion)
# block / stem outputs: measured max-norm 6.8e-3 ("big pool") and 6.0e-3 (plain stem) — a one-ulp flip of a stored conv
# output, carried through the BatchNorm's gain into the output element; the element-wise rule there admits that carry
# (`_err16c`)
TOL_Y = 1e-2
TOL_GRAD16 = 1.2e-2
EPS, MOM = 1e-5, 0.1


# ---- rounding points -------------------------------------------------------------------------------------------------
class _RoundFwd(torch.autograd.Function):
    """bf16 storage of a forward value (the gradient passes unchanged)"""

    @staticmethod
    def forward(ctx, t):
        return _r16(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBwd(torch.autograd.Function):
    """bf16 storage of the gradient of a value (the value passes unchanged)"""

    @staticmethod
    def forward(ctx, t):
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        return _r16(g)


def _rf(t):
    return _RoundFwd.apply(t)


def _rb(t):
    return _RoundBwd.apply(t)


def _rfb(t):
    return _rb(_rf(t))


class _LeakyReLU(torch.autograd.Function):
    """LeakyReLU(0.2) whose derivative takes the side `pos` (z > 0 everywhere except at the ties resolved by the caller)"""

    @staticmethod
    def forward(ctx, z, pos):
        ctx.save_for_backward(pos)
        return torch.where(z > 0, z, SLOPE * z)

    @staticmethod
    def backward(ctx, g):
        pos, = ctx.saved_tensors
        return g * torch.where(pos, 1.0, SLOPE), None


def _up(t):
    return F.interpolate(t, scale_factor=2, mode="nearest")


class _Ties:
    """tie resolution at the LeakyReLU kink: elements of |z| <= tau take the HIP path's sign"""

    def __init__(self):
        self.ties = 0
        self.flips = 0
        self.carry = []  # per call: one ulp of the stored inputs carried to each output element (`_err16c`)

    def side(self, z, tau, hip_pos):
        pos = z.detach() > 0
        if hip_pos is None:
            return pos
        near = z.detach().abs() <= tau
        self.ties += int(near.sum())
        self.flips += int((near & (pos != hip_pos)).sum())
        return torch.where(near, hip_pos, pos)


def _err16c(a, ref, carry):
    """_err16 with the element-wise bound widened by `carry`: a one-ulp flip of a stored conv output (the HIP path's fp32
    accumulation landing on the other side of a bf16 rounding boundary) carried through the BatchNorm into the element"""
    a = a.detach().double().cpu()
    if a.shape != ref.shape or not torch.isfinite(a).all():
        return float("inf")
    m = float(ref.abs().max()) + 1e-30
    if bool(((a - ref).abs() > ref.abs() * 2.0 ** -7 + carry + 1e-3 * m).any()):
        return float("inf")
    return float((a - ref).abs().max() / m)


def _bn(t, st, g, b, training):
    """nn.BatchNorm2d in fp64 (st: dict of fp64 running buffers, updated in place like the module's)"""
    if training:
        st["nbt"] += 1
    return F.batch_norm(t, st["rm"], st["rv"], g, b, training, MOM, EPS)


def _tau(t, st, g, training, extra=None):
    """one bf16 ulp of the stored inputs of BN(t) (+ extra), carried to the LeakyReLU input"""
    with torch.no_grad():
        if training:
            invstd = (t.var((0, 2, 3), unbiased=False) + EPS).rsqrt()
        else:
            invstd = (st["rv"] + EPS).rsqrt()
        tau = 2.0 ** -7 * t.abs() * (invstd * g.abs()).view(1, -1, 1, 1)
        if extra is not None:
            tau = tau + 2.0 ** -7 * extra.abs()
        return tau + 1e-6 * float(tau.max())


def ref_block(x, P, st1, st2, x_up, post, training, ties, hip1=None, hip2=None):
    """ResidualBlock.forward (train_soft_intro_vae.py:65-75) + its fused neighbour, fp64, rounded where stored.
    x: [B, Ci, Hs, Ws] (bf16 values), P: fp64 leaves w_exp (or None), w1, g1, b1, w2, g2, b2; st1 / st2: fp64 running
    buffers; hip1 / hip2: the HIP path's LeakyReLU signs of BN-1 / BN-2 (tie resolution)"""
    xg = _rb(x)                                                   # dx
    if P["w_exp"] is not None:
        idt = _rfb(F.conv2d(xg, _rf(P["w_exp"])))                 # idt; dz (at half resolution with x_up: block sums)
    else:
        idt = _rb(xg)                                             # dz of the identity skip
    xin = _up(xg) if x_up else xg
    idt = _up(idt) if x_up else idt
    a = _rfb(F.conv2d(xin, _rf(P["w1"]), padding=1))              # a; da
    z1 = _bn(a, st1, P["g1"], P["b1"], training)
    h = _rfb(_LeakyReLU.apply(z1, ties.side(z1, _tau(a.detach(), st1, P["g1"].detach(), training), hip1)))  # h; dh
    c = _rfb(F.conv2d(h, _rf(P["w2"]), padding=1))                # c; dc
    z2 = _bn(c, st2, P["g2"], P["b2"], training) + idt
    tau2 = _tau(c.detach(), st2, P["g2"].detach(), training, idt.detach())
    full = _LeakyReLU.apply(z2, ties.side(z2, tau2, hip2))
    if post == "pool":
        ties.carry.append(F.avg_pool2d(tau2, 2))
        return _rf(F.avg_pool2d(full, 2))
    if post == "up":
        ties.carry.append(_up(tau2))
        return _up(_rb(_rf(full)))                                # d_out after the Upsample's adjoint
    ties.carry.append(tau2)
    return _rf(full)


# ---- route classes ---------------------------------------------------------------------------------------------------
def _tile(ops16, B, Ci, Co, H, W):
    """pixel tile of a 3x3 forward conv: 'splitk' (K-split partials, one statistics row per image), 'big', 'small'"""
    r = ops16.conv2d_route(B, Ci, Co, H, W, 3, want_stats=True)
    return "splitk" if r.split > 1 else ("big" if B * H * W // r.stats_rows > (128 if Co > 64 else 256) else "small")


def block_route(B, nseg, Ci, Cm, Co, H, W, x_up, post, bn_fused=True, pool_dgrad=True):
    """route class of a ResidualBlock call, asked of the route functions of ops16 and the block plan under the case's
    own switches (as check_block sets them):
    (has_exp, x_up, post, conv1 tile, conv2 tile, pooled data gradient (x_up only), BN-1 / BN-2 one-launch backward,
    segmented)"""
    from sivae_hip import functional16 as SF16
    from sivae_hip import ops, ops16
    saved = (ops.BN_FUSED, ops16.POOL_DGRAD)
    ops.BN_FUSED, ops16.POOL_DGRAD = bn_fused, saved[1] and pool_dgrad
    try:
        pool = x_up and SF16.resblock_plan16(B, Ci, Cm, Co, H, W, x_up=x_up, post=post, nseg=nseg, has_exp=Ci != Co,
                                             training=True).dx == "pool"
        f1, f2 = (ops16.bn_bwd_route(B, C, H, W, nseg=nseg).family == "bn_fused" for C in (Cm, Co))
        return ("block", Ci != Co, bool(x_up), post, _tile(ops16, B, Ci, Cm, H, W), _tile(ops16, B, Cm, Co, H, W),
                pool if x_up else None, f1, f2, nseg > 1)
    finally:
        ops.BN_FUSED, ops16.POOL_DGRAD = saved


def walk_routes(channels, image_size, B, nseg=1, cdim=3, convs=None):
    """the route class of every layer group of the bf16 Encoder and Decoder at batch B (nseg > 1: a segmented batch of B
    images), in the order of nn.main_plan (the networks are built on the meta device; nothing runs).  convs (a list):
    gets (Ci, Co, H, W, ks code) of every conv whose epilogue writes BatchNorm statistics (the stem's and both 3x3 convs
    of every block)"""
    from sivae_hip import nn as N
    from sivae_hip import functional16 as SF16
    from sivae_hip import ops16
    with torch.device("meta"):
        enc = N.Encoder(cdim, 8, channels, image_size)
        dec = N.Decoder(cdim, 8, channels, image_size, conv_input_size=enc.conv_output_size)
    rec = []
    for s in N.main_plan(enc.main, (image_size, image_size)) + N.main_plan(dec.main, enc.conv_output_size[1:]):
        if s.kind == "block":
            rec.append(block_route(B, nseg, s.Ci, s.Cm, s.Co, s.H, s.W, s.x_up, s.post))
            if convs is not None:
                convs.extend([(s.Ci, s.Cm, s.H, s.W, 3), (s.Cm, s.Co, s.H, s.W, 3)])
        elif s.kind == "stem":
            kw = SF16._kwpack_ok(s.conv.weight, s.Ci)
            rec.append(("stem", kw, nseg > 1))
            if convs is not None:
                convs.append((5 * s.Ci if kw else s.Ci, s.Co, s.H, s.W, ops16.KS51 if kw else s.conv.kernel_size[0]))
        else:
            rec.append(("predict", SF16._kwpack_ok(s.conv.weight, s.Co), s.conv.bias is not None))
    return rec


# the benchmarked bf16 iterations (bench.py): config 3 (celeb128 batch 128, passes unpaired and as segmented pairs),
# celeb256_bf16_bs128 and the 16-image 256x256 shard (each likewise)
PRODUCTION = [("celeb128_bf16_bs128", [64, 128, 256, 512, 512], 128, 128),
              ("celeb256_bf16_bs128", [64, 128, 256, 512, 512, 512], 256, 128),
              ("celeb256_bf16_bs16_shard", [64, 128, 256, 512, 512, 512], 256, 16)]


def production_routes():
    """{route class: [where it is taken]} over the benchmarked workloads"""
    out = {}
    for name, channels, size, B in PRODUCTION:
        for nseg in (1, 2):
            for r in walk_routes(channels, size, B * nseg, nseg):
                out.setdefault(r, []).append("%s nseg=%d" % (name, nseg))
    return out


# ---- block cases -----------------------------------------------------------------------------------------------------
def _case(name, B, Ci, Co, H, x_up=False, post=None, nseg=1, seg_rev=False, mat_h=True, signmask=True, bn_fused=True,
          pool_dgrad=True, training=True, replay=False):
    return dict(name=name, B=B, Ci=Ci, Co=Co, H=H, x_up=x_up, post=post, nseg=nseg, seg_rev=seg_rev, mat_h=mat_h,
                signmask=signmask, bn_fused=bn_fused, pool_dgrad=pool_dgrad, training=training, replay=replay)


# H: the block's (full) resolution.  Big pixel tiles need >= 512 blocks: 40 channels (the 64-channel tile
# configuration, 512 pixels) at 128 x 128 take them from B = 16; split-K needs >= 8 sixteen-channel chunks on a small
# grid: 128 channels at 4 x 4 / 8 x 8.
BLOCK_CASES = [
    # -- split-K plans of the 512-channel small maps (4 x 4 / 8 x 8), plain and segmented
    _case("splitk pool", 8, 128, 128, 8, post="pool"),
    _case("splitk pool seg", 16, 128, 128, 8, post="pool", nseg=2),
    _case("splitk", 8, 128, 128, 4),
    _case("splitk seg rev", 16, 128, 128, 4, nseg=2, seg_rev=True),
    _case("splitk up_deferred", 8, 128, 128, 4, post="up_deferred"),
    _case("splitk up_deferred seg", 16, 128, 128, 4, post="up_deferred", nseg=2),
    _case("splitk x_up (no pooled dgrad)", 8, 128, 128, 8, x_up=True, post="up_deferred"),
    _case("splitk x_up (no pooled dgrad) seg", 16, 128, 128, 8, x_up=True, post="up_deferred", nseg=2),
    _case("splitk exp x_up (pooled dgrad)", 32, 256, 128, 32, x_up=True, post="up_deferred"),
    _case("splitk exp x_up (no pooled dgrad)", 4, 256, 128, 8, x_up=True, post="up_deferred"),
    # -- big pixel tiles (the 128 / 256-wide maps at the bench batches)
    _case("big pool", 16, 40, 40, 128, post="pool"),
    _case("big pool seg", 16, 40, 40, 128, post="pool", nseg=2),
    _case("big x_up up_deferred", 16, 40, 40, 128, x_up=True, post="up_deferred"),
    _case("big x_up up_deferred seg", 16, 40, 40, 128, x_up=True, post="up_deferred", nseg=2),
    _case("big x_up", 16, 40, 40, 128, x_up=True),
    _case("big x_up seg rev", 16, 40, 40, 128, x_up=True, nseg=2, seg_rev=True),
    _case("big x_up 3-launch BN", 16, 40, 40, 128, x_up=True, bn_fused=False),
    _case("big x_up 3-launch BN seg", 16, 40, 40, 128, x_up=True, bn_fused=False, nseg=2),
    _case("big exp pool", 16, 24, 40, 128, post="pool"),
    _case("big exp pool seg", 16, 24, 40, 128, post="pool", nseg=2),
    _case("big exp x_up up_deferred", 16, 24, 40, 128, x_up=True, post="up_deferred"),
    _case("big exp x_up up_deferred seg", 16, 24, 40, 128, x_up=True, post="up_deferred", nseg=2),
    # -- small pixel tiles
    _case("small pool seg", 8, 40, 40, 16, post="pool", nseg=2),
    _case("small exp pool", 4, 24, 40, 16, post="pool"),
    _case("small exp x_up up_deferred", 4, 48, 40, 16, x_up=True, post="up_deferred"),
    _case("small exp x_up up_deferred seg", 8, 48, 40, 16, x_up=True, post="up_deferred", nseg=2),
    _case("small x_up up_deferred seg", 8, 40, 40, 16, x_up=True, post="up_deferred", nseg=2),
    # -- the other branches of the glue
    _case("exp ragged", 3, 24, 40, 12),
    _case("exp up", 4, 40, 24, 8, post="up"),
    _case("7x7 up", 4, 40, 40, 7, post="up"),
    _case("exp pool to 7x7", 4, 24, 40, 14, post="pool"),
    _case("x_up (pooled dgrad off)", 4, 40, 40, 16, x_up=True, pool_dgrad=False),
    _case("exp x_up (pooled dgrad off)", 4, 24, 40, 16, x_up=True, post="up_deferred", pool_dgrad=False),
    _case("fused prologue", 4, 40, 40, 16, mat_h=False),
    _case("fused prologue exp x_up", 4, 24, 40, 16, x_up=True, post="up_deferred", mat_h=False),
    _case("fused prologue up", 4, 40, 24, 8, post="up", mat_h=False),
    _case("no signmask pool", 4, 24, 40, 16, post="pool", signmask=False),
    _case("no signmask x_up", 4, 40, 40, 16, x_up=True, post="up_deferred", signmask=False),
    _case("3-launch BN exp pool", 4, 24, 40, 16, post="pool", bn_fused=False),
    _case("3-launch BN exp x_up seg", 8, 48, 40, 16, x_up=True, nseg=2, bn_fused=False),
    _case("eval pool", 4, 24, 40, 16, post="pool", training=False),
    _case("eval exp x_up up", 4, 48, 40, 8, x_up=True, post="up", training=False),
    _case("replay", 4, 24, 40, 16, x_up=True, post="up_deferred", replay=True),
    _case("replay seg", 8, 40, 40, 8, post="up", nseg=2, seg_rev=True, replay=True),
]


def case_route(cs):
    H = cs["H"]
    return block_route(cs["B"], cs["nseg"], cs["Ci"], cs["Co"], cs["Co"], H, H, cs["x_up"], cs["post"],
                       bn_fused=cs["bn_fused"], pool_dgrad=cs["pool_dgrad"])


def _block_params(Ci, Co, seed):
    P = {"w_exp": None if Ci == Co else _rand(Co, Ci, 1, 1, seed=seed, scale=Ci ** -0.5),
         "w1": _rand(Co, Ci, 3, 3, seed=seed + 1, scale=(9 * Ci) ** -0.5),
         "g1": _rand(Co, seed=seed + 2, scale=0.3) + 1.0, "b1": _rand(Co, seed=seed + 3, scale=0.2),
         "w2": _rand(Co, Co, 3, 3, seed=seed + 4, scale=(9 * Co) ** -0.5),
         "g2": _rand(Co, seed=seed + 5, scale=0.3) + 1.0, "b2": _rand(Co, seed=seed + 6, scale=0.2)}
    return {k: None if v is None else v.float().double() for k, v in P.items()}


def _running(C, seed):
    return {"rm": _rand(C, seed=seed, scale=0.1).float().double(),
            "rv": (_rand(C, seed=seed + 1, scale=0.3).abs() + 0.7).float().double(),
            "nbt": 3}


def _signs_from_mask(out, C):
    """BN-2's sign: the uint8 sign mask (bit e of (b, cb, h, w): channel 8 cb + e > 0) or the bf16 block output"""
    out = out.detach().cpu()
    if out.dtype == torch.uint8:
        B, Cb, H, W = out.shape
        bits = (out.to(torch.int32).unsqueeze(-1) >> torch.arange(8, dtype=torch.int32)) & 1
        return bits.permute(0, 1, 4, 2, 3).reshape(B, Cb * 8, H, W)[:, :C].bool()
    return from_blocked(out, C) > 0


def _signs_bn1(cache, g1, b1, C, nseg):
    """BN-1's sign as its backward recomputes it: the affine of the stored conv output in fp32"""
    a = from_blocked(cache["a"], C).float()
    B = a.shape[0]
    m = cache["mean1"].detach().cpu().view(nseg, C)
    iv = cache["invstd1"].detach().cpu().view(nseg, C)
    out = []
    for g in range(nseg):
        sl = a[g * B // nseg:(g + 1) * B // nseg]
        sc = iv[g] * g1.float()
        out.append(((sl - m[g].view(1, -1, 1, 1)) * sc.view(1, -1, 1, 1) + b1.float().view(1, -1, 1, 1)) > 0)
    return torch.cat(out)


def check_block(cs):
    from sivae_hip import functional16 as SF16
    from sivae_hip import nn as N
    from sivae_hip import ops, ops16
    B, Ci, Co, H, x_up, post, nseg = cs["B"], cs["Ci"], cs["Co"], cs["H"], cs["x_up"], cs["post"], cs["nseg"]
    training, replay = cs["training"], cs["replay"]
    tag = "block[%s] B=%d %d->%d %dx%d" % (cs["name"], B, Ci, Co, H, H)
    route = case_route(cs)
    Hs = H // 2 if x_up else H
    Ho = H // 2 if post == "pool" else (2 * H if post == "up" else H)
    x = _r16(_rand(B, Ci, Hs, Hs, seed=1) + 0.2)
    dy = _r16(_rand(B, Co, Ho, Ho, seed=2))
    P = _block_params(Ci, Co, 10)
    run = [_running(Co, 20), _running(Co, 30)]
    # ---- the HIP path
    blk = N.ResidualBlock(Ci, Co).to(DEV)
    with torch.no_grad():
        if P["w_exp"] is not None:
            blk.conv_expand.weight.copy_(P["w_exp"].float())
        for mod, k in ((blk.conv1, "w1"), (blk.conv2, "w2")):
            mod.weight.copy_(P[k].float())
        for bn, k, r in ((blk.bn1, "1", run[0]), (blk.bn2, "2", run[1])):
            bn.weight.copy_(P["g" + k].float())
            bn.bias.copy_(P["b" + k].float())
            bn.running_mean.copy_(r["rm"].float())
            bn.running_var.copy_(r["rv"].float())
            bn.num_batches_tracked.fill_(r["nbt"])
    blk.train(training)
    saved = (SF16.MATERIALIZE_H, SF16.SIGNMASK, ops.BN_FUSED, ops16.POOL_DGRAD)
    SF16.MATERIALIZE_H, SF16.SIGNMASK = cs["mat_h"], cs["signmask"]
    ops.BN_FUSED, ops16.POOL_DGRAD = cs["bn_fused"], saved[3] and cs["pool_dgrad"]
    res = []
    try:
        xb = to_blocked(x).to(DEV).requires_grad_(training)
        cache = {} if training else None
        kw = dict(post=post, cache=cache, x_up=x_up, nseg=nseg, seg_rev=cs["seg_rev"])
        if replay:
            with torch.no_grad():
                y0 = blk(xb, **kw).clone()
            y = blk(xb, **kw)
            res.append((tag + " replay: y bit for bit", 0.0 if torch.equal(y, y0) else float("inf"), 0.0))
        else:
            y = blk(xb, **kw)
        if training:
            y.backward(to_blocked(dy).to(DEV))
        if replay:
            # a replay of a `cache_segment` view: same output, running buffers untouched
            bufs = [t.clone() for t in (blk.bn1.running_mean, blk.bn1.running_var, blk.bn2.running_mean,
                                        blk.bn2.running_var, blk.bn1.num_batches_tracked)]
            with torch.no_grad():
                y2 = blk(xb, **dict(kw, replay_update=False))
            same = torch.equal(y2, y0) and all(torch.equal(a, b) for a, b in zip(bufs, (
                blk.bn1.running_mean, blk.bn1.running_var, blk.bn2.running_mean, blk.bn2.running_var,
                blk.bn1.num_batches_tracked)))
            res.append((tag + " replay_update=False: y, buffers unchanged", 0.0 if same else float("inf"), 0.0))
        torch.cuda.synchronize()
    finally:
        SF16.MATERIALIZE_H, SF16.SIGNMASK, ops.BN_FUSED, ops16.POOL_DGRAD = saved
    # ---- the referee: nseg separate calls, running buffers updated in the reference's call order
    Pr = {k: None if v is None else v.clone().requires_grad_(training) for k, v in P.items()}
    st = [{"rm": r["rm"].clone(), "rv": r["rv"].clone(), "nbt": r["nbt"]} for r in run]
    ties = _Ties()
    hip1 = hip2 = None
    if training:
        hip1 = _signs_bn1(cache, P["g1"], P["b1"], Co, nseg)
        hip2 = _signs_from_mask(cache["out"], Co)
    Bs = B // nseg
    order = list(range(nseg))[::-1] if cs["seg_rev"] else list(range(nseg))
    if replay:  # the filling pass counted once already
        with torch.no_grad():
            for g in order:
                ref_block(x[g * Bs:(g + 1) * Bs], Pr, st[0], st[1], x_up, post, training, _Ties())
    xr = x.clone().requires_grad_(training)
    ys, carries = [None] * nseg, [None] * nseg
    for g in order:
        sl = slice(g * Bs, (g + 1) * Bs)
        ys[g] = ref_block(xr[sl], Pr, st[0], st[1], x_up, post, training, ties,
                          None if hip1 is None else hip1[sl], None if hip2 is None else hip2[sl])
        carries[g] = ties.carry[-1]
    yref = torch.cat(ys)
    if training:
        yref.backward(dy)
    if training:
        tag += " (ties %d, flips %d)" % (ties.ties, ties.flips)
    carry = torch.cat([carries[g] for g in range(nseg)])
    res.append((tag + " y", _err16c(from_blocked(y, Co), yref.detach(), carry), TOL_Y))
    res.append((tag + " y pad", _padded_zero(y, Co), 0.0))
    if training:
        # forward tensors the block stores for its backward (cached here), against the referee's
        with torch.no_grad():
            a = _r16(F.conv2d(_up(x) if x_up else x, _r16(P["w1"]), padding=1))
            res.append((tag + " a", _err16(from_blocked(cache["a"], Co), a), TOL_BF16))
        res.append((tag + " dx", _err(from_blocked(xb.grad, Ci), xr.grad), TOL_GRAD16))
        res.append((tag + " dx pad", _padded_zero(xb.grad, Ci), 0.0))
        named = [("dw_exp", blk.conv_expand.weight if Ci != Co else None, "w_exp"), ("dw1", blk.conv1.weight, "w1"),
                 ("dgamma1", blk.bn1.weight, "g1"), ("dbeta1", blk.bn1.bias, "b1"), ("dw2", blk.conv2.weight, "w2"),
                 ("dgamma2", blk.bn2.weight, "g2"), ("dbeta2", blk.bn2.bias, "b2")]
        for nm, p, k in named:
            if p is not None:
                res.append((tag + " " + nm, _err(p.grad, Pr[k].grad), TOL_F32))
    for i, (bn, s) in enumerate(((blk.bn1, st[0]), (blk.bn2, st[1]))):
        res.append((tag + " bn%d running_mean" % (i + 1), _err(bn.running_mean, s["rm"]), TOL_RUN))
        res.append((tag + " bn%d running_var" % (i + 1), _err(bn.running_var, s["rv"]), TOL_RUN))
        res.append((tag + " bn%d num_batches_tracked" % (i + 1),
                    float(abs(int(bn.num_batches_tracked) - s["nbt"])), 0.0))
    res.append((tag + " route %s" % (route[1:],), 0.0, 0.0))
    return res


# ---- stem / predict --------------------------------------------------------------------------------------------------
def ref_stem(x, w, g, b, st, training, ties, kw, hip=None):
    """conv5x5 -> BatchNorm -> LeakyReLU -> AvgPool2d(2) (train_soft_intro_vae.py:88-93), fp64, rounded where stored: the
    image enters as bf16; kw-packed, the data gradient is an fp32 fold (no rounding), plain, a bf16 conv output"""
    xin = _rf(x if kw else _rb(x))
    a = _rfb(F.conv2d(xin, _rf(w), padding=2))
    z = _bn(a, st, g, b, training)
    tau = _tau(a.detach(), st, g.detach(), training)
    ties.carry.append(F.avg_pool2d(tau, 2))
    return _rf(F.avg_pool2d(_LeakyReLU.apply(z, ties.side(z, tau, hip)), 2))


def check_stem(cdim, Co, H, B, nseg=1, seg_rev=False):
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    tag = "stem cdim=%d %d->%d %dx%d B=%d%s" % (cdim, cdim, Co, H, H, B, " nseg=%d%s" % (nseg, " rev" if seg_rev else "")
                                                 if nseg > 1 else "")
    x = _rand(B, cdim, H, H, seed=3).float().double() * 0.5 + 0.5
    w = _rand(Co, cdim, 5, 5, seed=4, scale=(25 * cdim) ** -0.5).float().double()
    g, b = (_rand(Co, seed=5, scale=0.3) + 1.0).float().double(), _rand(Co, seed=6, scale=0.2).float().double()
    run = _running(Co, 7)
    Ho = H // 2
    dy = _r16(_rand(B, Co, Ho, Ho, seed=8))
    bn = torch.nn.BatchNorm2d(Co).to(DEV).train()
    with torch.no_grad():
        bn.running_mean.copy_(run["rm"].float())
        bn.running_var.copy_(run["rv"].float())
        bn.num_batches_tracked.fill_(run["nbt"])
    xd = x.float().to(DEV).requires_grad_(True)
    wd, gd, bd = (t.float().to(DEV).requires_grad_(True) for t in (w, g, b))
    kw = SF16._kwpack_ok(wd, cdim)
    y = SF16.stem(xd, wd, gd, bd, SF.BNState(bn), nseg, seg_rev)
    y.backward(to_blocked(dy).to(DEV))
    torch.cuda.synchronize()
    # tie resolution: BN's sign as the backward recomputes it (fp32 affine of the conv output) — the referee's own
    # rounded conv output and fp64 statistics in fp32 (the block's stored a is not reachable here)
    st = {"rm": run["rm"].clone(), "rv": run["rv"].clone(), "nbt": run["nbt"]}
    ties = _Ties()
    xr, wr, gr, br = (t.clone().requires_grad_(True) for t in (x, w, g, b))
    Bs = B // nseg
    ys = [None] * nseg
    for s in (range(nseg)[::-1] if seg_rev else range(nseg)):
        sl = slice(s * Bs, (s + 1) * Bs)
        with torch.no_grad():
            a = _r16(F.conv2d(_r16(x[sl]), _r16(w), padding=2)).float()
            m, v = a.double().mean((0, 2, 3)).float(), a.double().var((0, 2, 3), unbiased=False)
            iv = (v + EPS).rsqrt().float()
            hip = ((a - m.view(1, -1, 1, 1)) * (iv * g.float()).view(1, -1, 1, 1) + b.float().view(1, -1, 1, 1)) > 0
        ys[s] = ref_stem(xr[sl], wr, gr, br, st, True, ties, kw, hip)
    torch.cat(ys).backward(dy)
    tag += "%s (ties %d, flips %d)" % (" kw-packed" if kw else " plain", ties.ties, ties.flips)
    carry = torch.cat([ties.carry[(nseg - 1 - s) if seg_rev else s] for s in range(nseg)])
    res = [(tag + " y", _err16c(from_blocked(y, Co), torch.cat(ys).detach(), carry), TOL_Y),
           (tag + " dx", _err(xd.grad, xr.grad), TOL_F32 if kw else TOL_GRAD16),
           (tag + " dw", _err(wd.grad, wr.grad), TOL_F32),
           (tag + " dgamma", _err(gd.grad, gr.grad), TOL_F32),
           (tag + " dbeta", _err(bd.grad, br.grad), TOL_F32),
           (tag + " running_mean", _err(bn.running_mean, st["rm"]), TOL_RUN),
           (tag + " running_var", _err(bn.running_var, st["rv"]), TOL_RUN),
           (tag + " num_batches_tracked", float(abs(int(bn.num_batches_tracked) - st["nbt"])), 0.0)]
    return res


def check_predict(cdim, Ci, H, B, bias=True):
    """Decoder.predict (conv5x5 + bias, train_soft_intro_vae.py:159): blocked bf16 in, fp32 out; the loss's fp32 gradient
    enters as bf16 for the data / weight gradients (its fp32 channel sum is the bias gradient)"""
    from sivae_hip import functional16 as SF16
    tag = "predict cdim=%d %d->%d %dx%d B=%d%s" % (cdim, Ci, cdim, H, H, B, "" if bias else " no bias")
    x = _r16(_rand(B, Ci, H, H, seed=11))
    w = _rand(cdim, Ci, 5, 5, seed=12, scale=(25 * Ci) ** -0.5).float().double()
    bv = _rand(cdim, seed=13).float().double() if bias else None
    dy = _rand(B, cdim, H, H, seed=14).float().double()
    xb = to_blocked(x).to(DEV).requires_grad_(True)
    wd = w.float().to(DEV).requires_grad_(True)
    bd = None if bv is None else bv.float().to(DEV).requires_grad_(True)
    kw = SF16._kwpack_ok(wd, cdim)
    y = SF16.conv_bias(xb, wd, bd)
    y.backward(dy.float().to(DEV))
    torch.cuda.synchronize()
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = None if bv is None else bv.clone().requires_grad_(True)
    yr = _rb(F.conv2d(_rb(xr), _rf(wr), padding=2))   # dx (bf16); the loss gradient as bf16 for dx / dw
    if br is not None:
        yr = yr + br.view(1, -1, 1, 1)
    yr.backward(dy)
    tag += " kw-packed" if kw else " plain"
    res = [(tag + " y", _err(y, yr), TOL_F32),
           (tag + " dx", _err(from_blocked(xb.grad, Ci), xr.grad), TOL_GRAD16),
           (tag + " dx pad", _padded_zero(xb.grad, Ci), 0.0),
           (tag + " dw", _err(wd.grad, wr.grad), TOL_F32)]
    if bias:
        res.append((tag + " dbias", _err(bd.grad, br.grad), TOL_F32))
    return res


STEM_CASES = [(3, 40, 32, 4, 1, False), (1, 40, 28, 4, 1, False), (4, 40, 16, 3, 1, False), (3, 40, 32, 4, 2, True)]
PREDICT_CASES = [(3, 40, 32, 3, True), (1, 40, 28, 2, True), (4, 40, 16, 3, True), (3, 24, 16, 2, False)]


def stem_route(cdim, nseg):
    from sivae_hip import functional16 as SF16
    return ("stem", SF16._kwpack_ok(torch.empty(1, cdim, 5, 5, device="meta"), cdim), nseg > 1)


def predict_route(cdim, bias):
    from sivae_hip import functional16 as SF16
    return ("predict", SF16._kwpack_ok(torch.empty(cdim, 1, 5, 5, device="meta"), cdim), bias)


def covered_routes():
    out = {case_route(cs): cs["name"] for cs in BLOCK_CASES if cs["training"] and not cs["replay"]}
    for cdim, Co, H, B, nseg, rev in STEM_CASES:
        out.setdefault(stem_route(cdim, nseg), "stem cdim=%d" % cdim)
    for cdim, Ci, H, B, bias in PREDICT_CASES:
        out.setdefault(predict_route(cdim, bias), "predict cdim=%d" % cdim)
    return out


def all_checks():
    checks = [("block[%s]" % cs["name"], lambda cs=cs: check_block(cs)) for cs in BLOCK_CASES]
    checks += [("stem%s" % (c,), lambda c=c: check_stem(*c)) for c in STEM_CASES]
    checks += [("predict%s" % (c,), lambda c=c: check_predict(*c)) for c in PREDICT_CASES]
    return checks


def main():
    nfail = 0
    rows = []
    filt = sys.argv[1:]
    for label, thunk in all_checks():
        if filt and not any(f in label for f in filt):
            continue
        try:
            for name, err, tol in thunk():
                ok = err <= tol
                nfail += (not ok)
                rows.append("%-4s %-100s err=%.3e tol=%.1e" % ("ok" if ok else "FAIL", name, err, tol))
        except Exception:  # noqa: BLE001
            nfail += 1
            rows.append("EXC  %s\n%s" % (label, traceback.format_exc(limit=4)))
        torch.cuda.synchronize()
    print("\n".join(rows))
    print("block_checks16: %d failures of %d" % (nfail, len(rows)))
    return nfail


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
