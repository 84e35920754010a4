"""The style variant's non-conv layers (reference: style_soft_intro_vae/net.py) as autograd Functions on the kernels of
csrc/style.hip:

  style_layer(x, noise_weight, bias, style, noise=None, mode=None, layer=0, eps=1e-8) -> y
      what follows a 3x3 convolution of DecodeBlock (net.py:169-185, :189-205): noise injection -> bias ->
      LeakyReLU(0.2) -> InstanceNorm -> style_mod.  mode: None / False (no noise tensor, the layer's fixed bump), True or
      'per_sample' (noise [B, 1, H, W]), 'batch_constant' (noise [1, 1, H, W]).  The noise tensor is an ARGUMENT: the
      caller draws it (blocks.DecodeBlock does, in the reference's order).
  stat_norm(x, bias, eps=1e-5) -> (xn, m, std)
      what follows a convolution of EncodeBlock (net.py:94-101, :113-121): bias -> LeakyReLU(0.2) -> the style statistics
      m, std [B, C] -> InstanceNorm.  All three outputs are differentiable.  Where std == 0 (a constant plane) the
      reference's gradient is NaN; the kernel drops the dstd term there.
  blur(x) -> the depthwise [1, 2, 1] x [1, 2, 1] / 16 filter (net.py:49-60), its own adjoint.

and the RGB layers with the level-of-detail blend on the kernels of csrc/rgb.hip:

  to_rgb(x, weight, bias, prev=None, blend=1.0) -> y [B, K, H, W]
      ToRGB (net.py:229-231): the 1x1 convolution with weight [K, C, 1, 1] plus bias [K].  With prev [B, K, H/2, W/2], the
      previous level's image: torch.lerp(F.interpolate(prev, size=2 H), that, blend) as Generator.decode2 does
      (net.py:563-571).  x, weight, bias and prev are differentiable; blend is a Python float.
  from_rgb(img, weight, bias, pool=False, other=None, blend=1.0) -> y [B, C, Ho, Wo]
      FromRGB followed by the encoders' second LeakyReLU (net.py:215-217, :270-271): the 1x1 convolution with weight
      [C, K, 1, 1] plus bias [C], then LeakyReLU(0.2) twice.  pool=True runs it on F.avg_pool2d(img, 2, 2); with other
      [B, C, Ho, Wo], the first block's output: torch.lerp(that, other, blend) (encode2, net.py:289-294).  img, weight,
      bias and other are differentiable.  1 <= K <= 4 image channels.

One forward and one backward launch per call (plus a small one for the sums over the batch); the activation is
recomputed in the backward, so a layer saves its input and two [B, C] vectors (an RGB layer its inputs alone).  There is
no CPU path.
"""
import torch

from . import ops

_MODES = {None: ops.STYLE_NOISE_NONE, False: ops.STYLE_NOISE_NONE, "": ops.STYLE_NOISE_NONE,
          True: ops.STYLE_NOISE_PER_SAMPLE, "per_sample": ops.STYLE_NOISE_PER_SAMPLE,
          "batch_constant": ops.STYLE_NOISE_BATCH_CONSTANT}


def noise_mode(mode):
    """the reference's `noise` argument (net.py:169-175: falsy, 'batch_constant', anything else truthy) -> 0 / 2 / 1"""
    if isinstance(mode, int) and not isinstance(mode, bool) and mode in (0, 1, 2):
        return mode
    try:
        return _MODES[mode]
    except (KeyError, TypeError):
        return ops.STYLE_NOISE_PER_SAMPLE if mode else ops.STYLE_NOISE_NONE


class StyleLayerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, noise_weight, bias, style, noise, mode, layer, eps):
        x, style = x.contiguous(), style.contiguous()
        nw = None if mode == ops.STYLE_NOISE_NONE else noise_weight.detach().reshape(-1)
        nz = None if mode == ops.STYLE_NOISE_NONE else noise.contiguous()
        b_ = bias.detach().reshape(-1)
        y, mean, rstd = ops.style_dec_fwd(x, nz, nw, b_, style, mode, layer, eps)
        ctx.mode, ctx.layer = mode, layer
        ctx.save_for_backward(x, noise_weight, bias, style, nz, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, noise_weight, bias, style, nz, mean, rstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        if need[4]:
            raise RuntimeError("sivae_hip.style_layer: no gradient with respect to the noise tensor")
        nw = None if ctx.mode == ops.STYLE_NOISE_NONE else noise_weight.detach().reshape(-1)
        dx, dnw, db, ds = ops.style_dec_bwd(dy.contiguous(), x, nz, nw, bias.detach().reshape(-1), style, mean, rstd,
                                            ctx.mode, ctx.layer, want_dx=need[0], want_dnw=need[1], want_dbias=need[2],
                                            want_dstyle=need[3])
        # (mode 0: noise_weight takes no part and gets no gradient, as in the reference)
        return (dx, None if dnw is None else dnw.view_as(noise_weight), None if db is None else db.view_as(bias), ds,
                None, None, None, None)


class StatNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, eps):
        x = x.contiguous()
        xn, mean, std = ops.style_enc_fwd(x, bias.detach().reshape(-1), eps)
        ctx.eps = eps
        ctx.save_for_backward(x, bias, mean, std)
        return xn, mean, std

    @staticmethod
    def backward(ctx, dxn, dmean, dstd):
        x, bias, mean, std = ctx.saved_tensors
        need = ctx.needs_input_grad
        c = lambda t: None if t is None else t.contiguous()  # noqa: E731
        dx, db = ops.style_enc_bwd(c(dxn), c(dmean), c(dstd), x, bias.detach().reshape(-1), mean, std, ctx.eps,
                                   want_dx=need[0], want_dbias=need[1])
        return dx, None if db is None else db.view_as(bias), None


class BlurFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return ops.style_blur(x.contiguous())

    @staticmethod
    def backward(ctx, dy):
        return ops.style_blur(dy.contiguous())


class ToRGBFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, prev, blend):
        x = x.contiguous()
        prev = None if prev is None else prev.contiguous()
        y = ops.style_to_rgb_fwd(x, weight.detach().contiguous(), bias.detach().contiguous(), prev, blend)
        ctx.blend, ctx.has_prev = blend, prev is not None
        ctx.save_for_backward(x, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dw, db, dp = ops.style_to_rgb_bwd(dy.contiguous(), x, weight.detach().contiguous(), ctx.has_prev, ctx.blend,
                                              want_dx=need[0], want_dw=need[1], want_dbias=need[2],
                                              want_dprev=ctx.has_prev and need[3])
        return dx, None if dw is None else dw.view_as(weight), db, dp, None


class FromRGBFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, weight, bias, pool, other, blend):
        img = img.contiguous()
        other = None if other is None else other.contiguous()
        y = ops.style_from_rgb_fwd(img, weight.detach().contiguous(), bias.detach().contiguous(), pool, other, blend)
        ctx.pool, ctx.blend, ctx.has_other = pool, blend, other is not None
        ctx.save_for_backward(img, weight, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        img, weight, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        di, dw, db, do = ops.style_from_rgb_bwd(dy.contiguous(), img, weight.detach().contiguous(),
                                                bias.detach().contiguous(), ctx.pool, ctx.has_other, ctx.blend,
                                                want_dimg=need[0], want_dw=need[1], want_dbias=need[2],
                                                want_dother=ctx.has_other and need[4])
        return di, None if dw is None else dw.view_as(weight), db, None, do, None


def style_layer(x, noise_weight, bias, style, noise=None, mode=None, layer=0, eps=1e-8):
    mode = noise_mode(mode)
    if mode != ops.STYLE_NOISE_NONE and noise is None:
        raise ValueError("sivae_hip.style_layer: noise mode %d needs the noise tensor" % mode)
    return StyleLayerFn.apply(x, noise_weight, bias, style, noise, mode, int(layer), float(eps))


def stat_norm(x, bias, eps=1e-5):
    return StatNormFn.apply(x, bias, float(eps))


def blur(x):
    return BlurFn.apply(x)


def to_rgb(x, weight, bias, prev=None, blend=1.0):
    return ToRGBFn.apply(x, weight, bias, prev, float(blend))


def from_rgb(img, weight, bias, pool=False, other=None, blend=1.0):
    return FromRGBFn.apply(img, weight, bias, bool(pool), other, float(blend))
