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
  style_layer(..., blur=True) is style_layer(blur(x), ...) and stat_norm(x, bias, blur=True) returns (blur(xn), m, std),
      each still ONE kernel per direction and bit for bit the composition: the chain reads the 9 taps itself, the blurred
      tensor is neither written nor saved (the decoder layer saves the unblurred x).  Above the LDS bound of the decoder
      backward (ops.style_dec_blur_bwd_fused) its dx is finished by one ops.style_blur call.

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

and what sits between the latent and the networks, on the kernels of csrc/mapping.hip and the LeakyReLU epilogue of
csrc/linear.hip:

  mapping(x, weights, biases, pixel_norm, slope=0.2, last_activation=True) -> y [B, N]
      a whole mapping network (net.py:755-855) as ONE autograd node: pixel_norm of the rows of x [B, Z] if asked for, then
      per layer one linear with LeakyReLU(slope) as its epilogue (the last layer without it when last_activation is
      False, no layer with it when slope is None: VAEMappingToLatentNoStyle).  Every layer's output is kept; the backward runs, per layer from the last, the LeakyReLU backward with the
      bias gradient in one pass, the weight gradient into the parameter's gradient slot and the data gradient, then the
      pixel-norm backward — each only where needs_input_grad asks for it, so frozen parameters cost no weight gradient.
      A layer shape the linear kernels do not take (ops.linear_supported) sends the whole call down the per-layer path
      (mapping_chain), which is also what non-float32 tensors take.
  styles(s, num_layers, s2=None, cutoff=None, avg=None, beta=None, psi=None, trunc_cutoff=None) -> styles [B, L, Z]
      SoftIntroVAEModelTL.generate's assembly (model.py:176-200): the repeat over the layers; with beta the running
      average avg [L, Z] <- lerp(avg, mean_b s, 1 - beta), IN PLACE and without a gradient, BEFORE the truncation; with s2
      the layers l >= cutoff take s2; with psi the layers l < trunc_cutoff become lerp(avg[l], ., psi).  s and s2 are
      differentiable.

One forward and one backward launch per call (plus a small one for the sums over the batch); the activation is
recomputed in the backward, so a layer saves its input and two [B, C] vectors (an RGB layer its inputs alone).  There is
no CPU path.
"""
import torch
from torch.nn import functional as F

from . import functional as SF
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
    def forward(ctx, x, noise_weight, bias, style, noise, mode, layer, eps, blur=False):
        x, style = x.contiguous(), style.contiguous()
        nw = None if mode == ops.STYLE_NOISE_NONE else noise_weight.detach().reshape(-1)
        nz = None if mode == ops.STYLE_NOISE_NONE else noise.contiguous()
        b_ = bias.detach().reshape(-1)
        y, mean, rstd = ops.style_dec_fwd(x, nz, nw, b_, style, mode, layer, eps, blur=blur)
        ctx.mode, ctx.layer, ctx.blur = mode, layer, blur
        ctx.save_for_backward(x, noise_weight, bias, style, nz, mean, rstd)  # (blur: the unblurred x)
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
                                            want_dstyle=need[3], blur=ctx.blur)
        # (mode 0: noise_weight takes no part and gets no gradient, as in the reference)
        return (dx, None if dnw is None else dnw.view_as(noise_weight), None if db is None else db.view_as(bias), ds,
                None, None, None, None, None)


class StatNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, eps, blur=False):
        x = x.contiguous()
        xn, mean, std = ops.style_enc_fwd(x, bias.detach().reshape(-1), eps, blur=blur)
        ctx.eps, ctx.blur = eps, blur
        ctx.save_for_backward(x, bias, mean, std)
        return xn, mean, std

    @staticmethod
    def backward(ctx, dxn, dmean, dstd):
        x, bias, mean, std = ctx.saved_tensors
        need = ctx.needs_input_grad
        c = lambda t: None if t is None else t.contiguous()  # noqa: E731
        dx, db = ops.style_enc_bwd(c(dxn), c(dmean), c(dstd), x, bias.detach().reshape(-1), mean, std, ctx.eps,
                                   want_dx=need[0], want_dbias=need[1], blur=ctx.blur)
        return dx, None if db is None else db.view_as(bias), None, None


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


def style_layer(x, noise_weight, bias, style, noise=None, mode=None, layer=0, eps=1e-8, blur=False):
    mode = noise_mode(mode)
    if mode != ops.STYLE_NOISE_NONE and noise is None:
        raise ValueError("sivae_hip.style_layer: noise mode %d needs the noise tensor" % mode)
    return StyleLayerFn.apply(x, noise_weight, bias, style, noise, mode, int(layer), float(eps), bool(blur))


def stat_norm(x, bias, eps=1e-5, blur=False):
    return StatNormFn.apply(x, bias, float(eps), bool(blur))


def blur(x):
    return BlurFn.apply(x)


def to_rgb(x, weight, bias, prev=None, blend=1.0):
    return ToRGBFn.apply(x, weight, bias, prev, float(blend))


def from_rgb(img, weight, bias, pool=False, other=None, blend=1.0):
    return FromRGBFn.apply(img, weight, bias, bool(pool), other, float(blend))


class MappingFn(torch.autograd.Function):
    """inputs: x, pixel_norm, slope, last_activation, then (weight, bias) per layer"""
    FIRST = 4  # position of the first weight among the inputs

    @staticmethod
    def forward(ctx, x, pixel_norm, slope, last_activation, *params):
        n = len(params) // 2
        SF._claim(ctx, [(MappingFn.FIRST + j, p) for j, p in enumerate(params)])
        x = x.contiguous()
        h, r = ops.pixel_norm_fwd(x) if pixel_norm else (x, None)
        acts = [h]  # the input of every layer, then the output of the last
        for i in range(n):
            w, b = params[2 * i].detach(), params[2 * i + 1].detach()
            if slope is not None and (i < n - 1 or last_activation):
                h = ops.linear_lrelu_fwd(h, w, b, slope)
            else:
                h = ops.linear_fwd(h, w, b)
            acts.append(h)
        ctx.cfg = (n, bool(pixel_norm), slope, bool(last_activation))
        ctx.save_for_backward(x if pixel_norm else None, r, *acts, *params)
        return h

    @staticmethod
    def backward(ctx, dy):
        n, pixel_norm, slope, last_activation = ctx.cfg
        saved = ctx.saved_tensors
        x, r, acts, params = saved[0], saved[1], saved[2:3 + n], saved[3 + n:]
        need, first = ctx.needs_input_grad, MappingFn.FIRST
        grads = [None] * (2 * n)
        g = dy.contiguous()
        upstream = need[0]
        for i in reversed(range(n)):
            w, b = params[2 * i], params[2 * i + 1]
            k_w, k_b = ctx.use[2 * i], ctx.use[2 * i + 1]
            need_w, need_b = need[first + 2 * i], need[first + 2 * i + 1]
            below = need[0] or any(need[first:first + 2 * i])  # does anything in front of this layer want a gradient
            y = acts[i + 1] if (slope is not None and (i < n - 1 or last_activation)) else None
            dz, db = ops.lrelu_bias_bwd(g, y, 0.0 if slope is None else slope, want_dz=need_w or below, want_dbias=need_b,
                                        out=SF._dst(b, k_b) if need_b else None)
            dw = ops.linear_wgrad(dz, acts[i], out=SF._dst(w, k_w)) if need_w else None
            grads[2 * i], grads[2 * i + 1] = SF._hand(dw, w, k_w), SF._hand(db, b, k_b)
            if not below:
                g = None
                break
            g = ops.linear_dgrad(dz, w.detach())
        dx = None
        if upstream and g is not None:
            dx = ops.pixel_norm_bwd(g, x, r) if pixel_norm else g
        return (dx, None, None, None) + tuple(grads)


class StylesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, s2, num_layers, cutoff, avg, beta, psi, trunc_cutoff):
        s = s.contiguous()
        s2 = None if s2 is None else s2.contiguous()
        out = ops.styles_fwd(s, num_layers, s2, cutoff, avg, beta, psi, trunc_cutoff)
        ctx.cfg = (s2 is not None, cutoff, psi, trunc_cutoff)
        return out

    @staticmethod
    def backward(ctx, dstyles):
        has_s2, cutoff, psi, trunc_cutoff = ctx.cfg
        need = ctx.needs_input_grad
        ds, ds2 = ops.styles_bwd(dstyles.contiguous(), has_s2, cutoff, psi, trunc_cutoff, want_ds=need[0],
                                 want_ds2=has_s2 and need[1])
        return ds, ds2, None, None, None, None, None, None


def mapping_chain(x, weights, biases, pixel_norm, slope=0.2, last_activation=True):
    """the per-layer path mapping() replaces: torch's pixel_norm, one functional.linear node and one torch LeakyReLU per
    layer"""
    if pixel_norm:
        x = x * torch.rsqrt(x.pow(2.0).mean(dim=1, keepdim=True) + 1e-8)
    n = len(weights)
    for i, (w, b) in enumerate(zip(weights, biases)):
        x = SF.linear(x, w, b)
        if slope is not None and (i < n - 1 or last_activation):
            x = F.leaky_relu(x, slope)
    return x


def mapping(x, weights, biases, pixel_norm, slope=0.2, last_activation=True):
    weights, biases = list(weights), list(biases)
    if not weights or len(weights) != len(biases) or any(b is None for b in biases):
        raise ValueError("sivae_hip.mapping: one weight and one bias per layer, at least one layer")
    if x.dim() != 2:
        raise ValueError("sivae_hip.mapping: expected rows [B, Z], got %s" % (tuple(x.shape),))
    B = x.shape[0]
    fused = x.dtype == torch.float32 and all(
        w.dim() == 2 and w.dtype == torch.float32 and ops.linear_supported(B, w.shape[1], w.shape[0]) for w in weights)
    if not fused:
        return mapping_chain(x, weights, biases, pixel_norm, slope, last_activation)
    k = x.shape[1]
    for w, b in zip(weights, biases):
        if w.shape[1] != k or b.numel() != w.shape[0]:
            raise RuntimeError("mat1 and mat2 shapes cannot be multiplied (%dx%d and %dx%d)" % (B, k, w.shape[1], w.shape[0]))
        k = w.shape[0]
    params = [p for wb in zip(weights, biases) for p in wb]
    return SF._apply(MappingFn, x, bool(pixel_norm), None if slope is None else float(slope), bool(last_activation), *params)


def styles(s, num_layers, s2=None, cutoff=None, avg=None, beta=None, psi=None, trunc_cutoff=None):
    if avg is not None and avg.requires_grad:
        raise ValueError("sivae_hip.styles: the running average takes no gradient; pass a buffer (or .data)")
    return StylesFn.apply(s, s2, int(num_layers), None if cutoff is None else int(cutoff), avg,
                          None if beta is None else float(beta), None if psi is None else float(psi),
                          None if trunc_cutoff is None else int(trunc_cutoff))
