"""Drop-in blocks of the style variant (reference: style_soft_intro_vae/net.py:28-207) on the HIP kernels.

Put this directory on PYTHONPATH and, in the reference's net.py, replace the definitions of Blur, EncodeBlock and
DecodeBlock with

    from blocks import Blur, EncodeBlock, DecodeBlock

(or take the whole-file drop-ins next to this one: net.py for the reference's net.py, and model.py, the third drop-in
file, for its model.py).
Constructor arguments, forward signatures, state_dict keys (the `blur.weight` buffer included), initial values for a
seed and the `lr_equalization_coef` attributes the reference's custom_adam.py reads are the reference's; only the
implicit learning-rate-equalised form (its default) is built.  What follows each convolution runs on sivae_hip.style
(one fused kernel per chain and direction), the 3x3 stride-1 convolutions on sivae_hip.functional.conv_bias, the linears
on functional.linear, the fused_scale=True convolutions (stride 2 with the transformed kernel, the resolutions from 128
up) on functional.conv_upscale / conv_downscale: the phase-form upsample-convolution kernels run one way or the other.
The blur in front of the decoder's first layer and behind the encoder's first norm is folded into that chain
(style.style_layer / stat_norm with blur=True: no blur launch, no blurred tensor, the same bits); the Blur module and its
buffer stay for the state dict.  SIVAE_STYLE_FUSE_BLUR=0 restores the separate calls.
Still torch here: upscale2d and downscale2d around the fused_scale=False pairs.  ROCm device tensors only: there is no
CPU path (the convolutions alone still take CPU tensors through torch's).
"""
import os

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from sivae_hip import functional as SF
from sivae_hip import ops, style


# SIVAE_STYLE_SCALE_CONV=0: the fused_scale convolutions stay on torch's stride-2 convolutions (read at call time: tests
# and tools assign blocks.SCALE_CONV)
SCALE_CONV = os.environ.get("SIVAE_STYLE_SCALE_CONV", "1") != "0"
# SIVAE_STYLE_FUSE_BLUR=0: the blur stays a call and an autograd node of its own in front of the decoder's first layer
# and behind the encoder's first norm (read at call time, like SCALE_CONV)
FUSE_BLUR = os.environ.get("SIVAE_STYLE_FUSE_BLUR", "1") != "0"
# Decoder planes above this many elements keep the composition (None: no limit).  It is the LDS bound of csrc/style.hip's
# decoder backward (ST_BLUR_LDS_MAX): above it the fused pair still ends with a blur launch, and that class, 256 x 256,
# measured as a loss (README, profiles/style_blur_bench.txt).  The encoder's pair gained at every shape and has no limit.
FUSE_BLUR_DEC_MAX_HW = 16384


def _fuse_blur_dec(x):
    return FUSE_BLUR and (FUSE_BLUR_DEC_MAX_HW is None or x.shape[2] * x.shape[3] <= FUSE_BLUR_DEC_MAX_HW)


def pixel_norm(x, epsilon=1e-8):
    return x * torch.rsqrt(x.pow(2.0).mean(dim=1, keepdim=True) + epsilon)


def style_mod(x, style):
    s = style.view(style.shape[0], 2, x.shape[1], 1, 1)
    return torch.addcmul(s[:, 1], x, s[:, 0] + 1)


def upscale2d(x, factor=2):
    return x.repeat_interleave(factor, dim=2).repeat_interleave(factor, dim=3)


def downscale2d(x, factor=2):
    return F.avg_pool2d(x, factor, factor)


def _equalised(weight, std, bias=None):
    """N(0, std) weights carrying the coefficient custom_adam.py scales their step by; a zero bias carries 1.0"""
    nn.init.normal_(weight, mean=0, std=std)
    weight.lr_equalization_coef = std
    if bias is not None:
        bias.lr_equalization_coef = 1.0


class _Linear(nn.Module):
    def __init__(self, in_features, out_features, gain=np.sqrt(2.0)):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.zeros(out_features))
        self.std = gain / np.sqrt(in_features) * 1.0
        _equalised(self.weight, self.std, self.bias)

    def forward(self, x):
        return SF.linear(x, self.weight, self.bias)


class _Conv3x3(nn.Module):
    """bias-free 3x3 convolution with padding 1.  scale None: stride 1, on the HIP kernels.  'down': stride 2 with the
    kernel averaged over its four shifts; 'up': the transposed stride-2 form with the summed kernel — both on the HIP
    kernels for float32 device tensors whose shape ops.scale_conv_routes takes, on torch's convolutions otherwise."""

    def __init__(self, in_channels, out_channels, scale=None):
        super().__init__()
        shape = (in_channels, out_channels, 3, 3) if scale == "up" else (out_channels, in_channels, 3, 3)
        self.weight = nn.Parameter(torch.empty(*shape))
        self.register_parameter("bias", None)
        self.scale = scale
        self.std = np.sqrt(2.0) / np.sqrt(9 * in_channels)
        _equalised(self.weight, self.std)

    def _shifted_sum(self):
        w = F.pad(self.weight, (1, 1, 1, 1))
        return w[:, :, 1:, 1:] + w[:, :, :-1, 1:] + w[:, :, 1:, :-1] + w[:, :, :-1, :-1]

    def _on_kernels(self, x):
        if not (SCALE_CONV and x.is_cuda and x.dtype == torch.float32 and self.weight.dtype == torch.float32):
            return False
        B, Ci, H, W = x.shape
        return not ops.scale_conv_routes(self.scale, B, Ci, self.weight.shape[1 if self.scale == "up" else 0], H, W).refused

    def forward(self, x):
        if self.scale is not None and self._on_kernels(x):
            return SF.conv_upscale(x, self.weight) if self.scale == "up" else SF.conv_downscale(x, self.weight)
        if self.scale == "up":
            return F.conv_transpose2d(x, self._shifted_sum(), None, stride=2, padding=1)
        if self.scale == "down":
            return F.conv2d(x, self._shifted_sum() * 0.25, None, stride=2, padding=1)
        B, Ci, H, W = x.shape
        Co = self.weight.shape[0]
        refused = (ops.conv2d_fwd_route(B, Ci, Co, H, W, 3).error or ops.conv2d_fwd_route(B, Co, Ci, H, W, 3, mode=1).error
                   or ops.conv2d_wgrad_route(B, Ci, Co, H, W, 3).error) if x.is_cuda else None
        if refused:
            return F.conv2d(x, self.weight, None, padding=1)
        return SF.conv_bias(x, self.weight, None)


class Blur(nn.Module):
    def __init__(self, channels):
        super().__init__()
        f = torch.tensor([1.0, 2.0, 1.0])
        self.register_buffer("weight", (f[:, None] * f[None, :] / 16.0).view(1, 1, 3, 3).repeat(channels, 1, 1, 1))
        self.groups = channels

    def forward(self, x):
        return style.blur(x)  # (the buffer is the reference's state_dict entry; the kernel has the filter built in)


class EncodeBlock(nn.Module):
    def __init__(self, inputs, outputs, latent_size, last=False, fused_scale=True):
        super().__init__()
        self.conv_1 = _Conv3x3(inputs, inputs)
        self.bias_1 = nn.Parameter(torch.zeros(1, inputs, 1, 1))
        self.blur = Blur(inputs)
        self.last, self.fused_scale = last, fused_scale
        if last:
            self.dense = _Linear(inputs * 4 * 4, outputs)
        else:
            self.conv_2 = _Conv3x3(inputs, outputs, "down" if fused_scale else None)
        self.bias_2 = nn.Parameter(torch.zeros(1, outputs, 1, 1))
        self.style_1 = _Linear(2 * inputs, latent_size)
        self.style_2 = _Linear(outputs if last else 2 * outputs, latent_size)

    def forward(self, x):
        x = self.conv_1(x)
        fuse = FUSE_BLUR and not self.last
        x, m, std = style.stat_norm(x, self.bias_1, blur=True) if fuse else style.stat_norm(x, self.bias_1)
        w1 = self.style_1(torch.cat((m, std), dim=1))
        if self.last:
            x = F.leaky_relu(self.dense(x.view(x.shape[0], -1)), 0.2)
            return x, w1, self.style_2(x)
        x = self.conv_2(x if fuse else self.blur(x))
        if not self.fused_scale:
            x = downscale2d(x)
        x, m, std = style.stat_norm(x, self.bias_2)
        return x, w1, self.style_2(torch.cat((m, std), dim=1))


class DecodeBlock(nn.Module):
    def __init__(self, inputs, outputs, latent_size, has_first_conv=True, fused_scale=True, layer=0):
        super().__init__()
        self.inputs, self.has_first_conv, self.fused_scale, self.layer = inputs, has_first_conv, fused_scale, layer
        if has_first_conv:
            self.conv_1 = _Conv3x3(inputs, outputs, "up" if fused_scale else None)
        self.blur = Blur(outputs)
        self.noise_weight_1 = nn.Parameter(torch.zeros(1, outputs, 1, 1))
        self.bias_1 = nn.Parameter(torch.zeros(1, outputs, 1, 1))
        self.style_1 = _Linear(latent_size, 2 * outputs, gain=1)
        self.conv_2 = _Conv3x3(outputs, outputs)
        self.noise_weight_2 = nn.Parameter(torch.zeros(1, outputs, 1, 1))
        self.bias_2 = nn.Parameter(torch.zeros(1, outputs, 1, 1))
        self.style_2 = _Linear(latent_size, 2 * outputs, gain=1)

    def _layer(self, x, noise_weight, bias, s, noise, blur=False):
        mode = style.noise_mode(noise)
        nz = None
        if mode:  # (drawn here, shape and order as in the reference: one tensor per layer, the first layer's first)
            nz = torch.randn([1 if mode == ops.STYLE_NOISE_BATCH_CONSTANT else x.shape[0], 1, x.shape[2], x.shape[3]],
                             device=x.device)
        if blur:  # (the layer reads blur(x) from x; without it the call stays the one it was)
            return style.style_layer(x, noise_weight, bias, s, nz, mode, self.layer, blur=True)
        return style.style_layer(x, noise_weight, bias, s, nz, mode, self.layer)

    def forward(self, x, s1, s2, noise):
        fuse = False
        if self.has_first_conv:
            if not self.fused_scale:
                x = upscale2d(x)
            x = self.conv_1(x)
            fuse = _fuse_blur_dec(x)
            if not fuse:
                x = self.blur(x)
        x = self._layer(x, self.noise_weight_1, self.bias_1, self.style_1(s1), noise, fuse)
        return self._layer(self.conv_2(x), self.noise_weight_2, self.bias_2, self.style_2(s2), noise)
