"""Drop-in network classes of the style variant (reference: style_soft_intro_vae/net.py) on the HIP kernels.

Put this directory in front of the reference's style_soft_intro_vae directory on PYTHONPATH: model.py (`from net import *`;
the third drop-in file, next to this one and blocks.py, or the reference's own) and the reference's training script then
build their encoder, generator and mapping networks from these classes.
Constructor arguments, forward signatures, registry names, state_dict keys and their order, initial values for a seed
and the `.std` / `lr_equalization_coef` attributes are the reference's; only the implicit learning-rate-equalised form
(its default) is built, and the DCGAN encoder / generator are not.

What runs where.  The blocks are blocks.py's (fused instance-norm chains, the blur, 3x3 convolutions and linears on the
HIP kernels).  ToRGB with Generator.decode2's upsample-and-lerp, and FromRGB with the encoders' second LeakyReLU and
encode2's avg-pool-and-lerp, are one kernel per direction each (sivae_hip.style.to_rgb / from_rgb).  A mapping network
is ONE autograd node (sivae_hip.style.mapping): the row pixel-norm kernel, one linear per layer with the LeakyReLU as
its epilogue, and in the backward one pass per layer for the LeakyReLU and the bias gradient.  Each mapping class has
`map(x, fused=True)`, which returns the rows [B, N] before the class's view / repeat; `forward` is `map` followed by that
view / repeat.  `fused=False`, tensors that are not float32 and layer shapes the linear kernels refuse take the per-layer
chain (torch's pixel_norm and LeakyReLU around sivae_hip.functional.linear).  The fused_scale convolutions of the
resolutions from 128 up run on the phase-form upsample-convolution kernels (blocks._Conv3x3, functional.conv_upscale /
conv_downscale).  Still torch: what blocks.py leaves to torch (upscale2d and downscale2d around the fused_scale=False
pairs of the resolutions below 128).
ROCm device tensors only.  An RGB layer with more than 4 image channels, or tensors that are not float32, takes the torch
chain of the reference instead.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from blocks import *  # noqa: F401,F403
from blocks import DecodeBlock, EncodeBlock, _equalised, pixel_norm
from sivae_hip import functional as SF
from sivae_hip import ops, style

try:
    from registry import *  # noqa: F401,F403  (next to the reference's files: its registries, which model.py shares)
    from registry import ENCODERS, GENERATORS, MAPPINGS
except ImportError:
    class Registry(dict):
        def register(self, name):
            def add(cls):
                assert name not in self
                self[name] = cls
                return cls
            return add

    MODELS, ENCODERS, GENERATORS, MAPPINGS, DISCRIMINATORS = (Registry() for _ in range(5))


class _LreqLinear(nn.Module):
    """the reference's lreq.Linear with its lrmul: std = gain / sqrt(in) lrmul, N(0, std / lrmul) weights whose step the
    optimizer scales by std, a zero bias whose step it scales by lrmul.  Inputs of any rank are flattened to rows."""

    def __init__(self, in_features, out_features, gain=np.sqrt(2.0), lrmul=1.0):
        super().__init__()
        self.in_features = in_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        self.bias = nn.Parameter(torch.zeros(out_features))
        self.gain, self.lrmul = gain, lrmul
        self.std = gain / np.sqrt(in_features) * lrmul
        _equalised(self.weight, self.std / lrmul)
        self.weight.lr_equalization_coef = self.std
        self.bias.lr_equalization_coef = lrmul

    def forward(self, x):
        y = SF.linear(x.reshape(-1, x.shape[-1]), self.weight, self.bias)
        return y.view(*x.shape[:-1], y.shape[-1])


class _Conv1x1(nn.Module):
    """the parameters of the reference's 1x1 lreq.Conv2d: weight [out, in, 1, 1], a zero bias [out]"""

    def __init__(self, in_channels, out_channels, gain=np.sqrt(2.0)):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 1, 1))
        self.bias = nn.Parameter(torch.zeros(out_channels))
        self.std = gain / np.sqrt(in_channels)
        _equalised(self.weight, self.std, self.bias)

    def forward(self, x):
        return F.conv2d(x, self.weight, self.bias)


def _fused_rgb(image_channels, *tensors):
    return image_channels <= ops.STYLE_RGB_MAX_K and all(t is None or t.dtype == torch.float32 for t in tensors)


class FromRGB(nn.Module):
    def __init__(self, channels, outputs):
        super().__init__()
        self.channels = channels
        self.from_rgb = _Conv1x1(channels, outputs)

    def forward(self, x):
        return F.leaky_relu(self.from_rgb(x), 0.2)

    def encode_input(self, x, pool=False, other=None, blend=1.0):
        """what the encoders do with an image: forward, their second LeakyReLU, and in encode2 the average pool in front
        and the lerp with the first block's output behind; one kernel per direction"""
        if _fused_rgb(self.channels, x, other):
            return style.from_rgb(x, self.from_rgb.weight, self.from_rgb.bias, pool, other, blend)
        a = F.leaky_relu(self.forward(F.avg_pool2d(x, 2, 2) if pool else x), 0.2)
        return a if other is None else torch.lerp(a, other, blend)


class ToRGB(nn.Module):
    def __init__(self, inputs, channels):
        super().__init__()
        self.inputs, self.channels = inputs, channels
        self.to_rgb = _Conv1x1(inputs, channels, gain=0.03)

    def forward(self, x):
        return self.blended(x)

    def blended(self, x, prev=None, blend=1.0):
        """forward, and with prev (the previous level's image) Generator.decode2's upsampling and lerp behind it; one
        kernel per direction"""
        if _fused_rgb(self.channels, x, prev):
            return style.to_rgb(x, self.to_rgb.weight, self.to_rgb.bias, prev, blend)
        y = self.to_rgb(x)
        return y if prev is None else torch.lerp(F.interpolate(prev, size=y.shape[2:]), y, blend)


def _conv_statistics(blocks, first_has_conv_1=True):
    layers = []
    for i, block in enumerate(blocks):
        conv_1 = conv_1_c = 1.0
        if i or first_has_conv_1:
            conv_1, conv_1_c = block.conv_1.weight.std().item(), block.conv_1.std
        layers.append((conv_1 / conv_1_c, block.conv_2.weight.std().item() / block.conv_2.std))
    return layers


class _EncoderBase(nn.Module):
    dense_last = False  # the last block ends in a linear layer instead of a second convolution
    with_fc = False     # ... and a one-output linear head follows it

    def __init__(self, startf, maxf, layer_count, latent_size, channels=3):
        super().__init__()
        self.maxf, self.startf, self.layer_count = maxf, startf, layer_count
        self.from_rgb = nn.ModuleList()
        self.channels, self.latent_size = channels, latent_size
        self.encode_block = nn.ModuleList()
        mul, inputs, resolution = 2, startf, 2 ** (layer_count + 1)
        for i in range(layer_count):
            outputs = min(maxf, startf * mul)
            self.from_rgb.append(FromRGB(channels, inputs))
            self.encode_block.append(EncodeBlock(inputs, outputs, latent_size, self.dense_last and i == layer_count - 1,
                                                 fused_scale=resolution >= 128))
            resolution //= 2
            inputs = outputs
            mul *= 2
        if self.with_fc:
            self.fc2 = _LreqLinear(inputs, 1, gain=1)

    def _run(self, x, styles, first):
        for i in range(first, self.layer_count):
            x, s1, s2 = self.encode_block[i](x)
            styles = styles + (s1 + s2)
        styles = styles.unsqueeze(1)
        return (styles, self.fc2(x)) if self.with_fc else styles

    def _styles(self, x):
        return torch.zeros(x.shape[0], self.latent_size, device=x.device, dtype=x.dtype)

    def encode(self, x, lod):
        first = self.layer_count - lod - 1
        return self._run(self.from_rgb[first].encode_input(x), self._styles(x), first)

    def encode2(self, x, lod, blend):
        first = self.layer_count - lod - 1
        y, s1, s2 = self.encode_block[first](self.from_rgb[first].encode_input(x))
        styles = self._styles(x) + (s1 * blend + s2 * blend)
        y = self.from_rgb[first + 1].encode_input(x, pool=True, other=y, blend=blend)
        return self._run(y, styles, first + 1)

    def forward(self, x, lod, blend):
        return self.encode(x, lod) if blend == 1 else self.encode2(x, lod, blend)

    def get_statistics(self, lod):
        first = self.layer_count - lod - 1
        rgb = self.from_rgb[first].from_rgb
        return rgb.weight.std().item() / rgb.std, _conv_statistics(list(self.encode_block)[first:])


@ENCODERS.register("EncoderDefault")
class Encoder_old(_EncoderBase):
    pass


@ENCODERS.register("EncoderWithFC")
class EncoderWithFC(_EncoderBase):
    dense_last = with_fc = True


@ENCODERS.register("EncoderWithStatistics")
class Encoder(_EncoderBase):
    dense_last = True


@GENERATORS.register("GeneratorDefault")
class Generator(nn.Module):
    def __init__(self, startf=32, maxf=256, layer_count=3, latent_size=128, channels=3):
        super().__init__()
        self.maxf, self.startf, self.layer_count = maxf, startf, layer_count
        self.channels, self.latent_size = channels, latent_size
        mul = 2 ** (layer_count - 1)
        inputs = min(maxf, startf * mul)
        self.const = nn.Parameter(torch.ones(1, inputs, 4, 4))
        self.layer_to_resolution = [0] * layer_count
        self.style_sizes = []
        self.decode_block = nn.ModuleList()
        to_rgb = nn.ModuleList()
        resolution = 2
        for i in range(layer_count):
            outputs = min(maxf, startf * mul)
            self.decode_block.append(DecodeBlock(inputs, outputs, latent_size, i != 0, fused_scale=resolution * 2 >= 128,
                                                 layer=i))
            resolution *= 2
            self.layer_to_resolution[i] = resolution
            self.style_sizes += [2 * (inputs if i else outputs), 2 * outputs]
            to_rgb.append(ToRGB(outputs, channels))
            inputs = outputs
            mul //= 2
        self.to_rgb = to_rgb

    def _blocks(self, styles, n, noise, x=None, start=0):
        if x is None:  # (the kernels take one batch size: the constant is expanded, autograd sums its gradient back)
            x = self.const.expand(styles.shape[0], -1, -1, -1)
        for i in range(start, n):
            x = self.decode_block[i](x, styles[:, 2 * i + 0], styles[:, 2 * i + 1], noise)
        return x

    def decode(self, styles, lod, noise):
        return self.to_rgb[lod](self._blocks(styles, lod + 1, noise))

    def decode2(self, styles, lod, blend, noise):
        x = self._blocks(styles, lod, noise)
        x_prev = self.to_rgb[lod - 1](x)
        x = self._blocks(styles, lod + 1, noise, x, lod)
        return self.to_rgb[lod].blended(x, x_prev, blend)

    def forward(self, styles, lod, blend, noise):
        return self.decode(styles, lod, noise) if blend == 1 else self.decode2(styles, lod, blend, noise)

    def get_statistics(self, lod):
        rgb = self.to_rgb[lod].to_rgb
        return rgb.weight.std().item() / rgb.std, _conv_statistics(list(self.decode_block)[:lod + 1], False)


class MappingBlock(nn.Module):
    def __init__(self, inputs, output, lrmul):
        super().__init__()
        self.fc = _LreqLinear(inputs, output, lrmul=lrmul)

    def forward(self, x):
        return F.leaky_relu(self.fc(x), 0.2)


def _run_mapping(x, fcs, normalise, slope, fused):
    """rows x through the linear layers fcs, each followed by LeakyReLU(slope) (none of them when slope is None): one
    fused node, or the per-layer chain"""
    run = style.mapping if fused else style.mapping_chain
    return run(x, [fc.weight for fc in fcs], [fc.bias for fc in fcs], normalise, slope)


def _mapping_widths(mapping_layers, first, hidden, last):
    """(inputs, outputs) of each layer"""
    widths = [first] + [hidden] * (mapping_layers - 1) + [last]
    return list(zip(widths[:-1], widths[1:]))


@MAPPINGS.register("MappingDefault")
class Mapping(nn.Module):
    def __init__(self, num_layers, mapping_layers=5, latent_size=256, dlatent_size=256, mapping_fmaps=256):
        super().__init__()
        self.mapping_layers, self.num_layers = mapping_layers, num_layers
        for i, (a, b) in enumerate(_mapping_widths(mapping_layers, latent_size, mapping_fmaps, dlatent_size)):
            setattr(self, "block_%d" % (i + 1), MappingBlock(a, b, lrmul=0.01))

    def map(self, z, fused=True):
        """the mapped rows [B, dlatent_size], before the repeat over the layers"""
        fcs = [getattr(self, "block_%d" % (i + 1)).fc for i in range(self.mapping_layers)]
        return _run_mapping(z, fcs, True, 0.2, fused)

    def forward(self, z):
        x = self.map(z)
        return x.view(x.shape[0], 1, x.shape[1]).repeat(1, self.num_layers, 1)


class _MapBlocks(nn.Module):
    def __init__(self, mapping_layers, first, hidden, last, block):
        super().__init__()
        self.mapping_layers = mapping_layers
        self.map_blocks = nn.ModuleList(block(a, b, lrmul=0.1) for a, b in _mapping_widths(mapping_layers, first, hidden, last))

    normalise = False  # pixel_norm in front of the first layer
    slope = 0.2        # the blocks are MappingBlocks: LeakyReLU(0.2) behind every linear (None: plain linears)

    def map(self, x, fused=True):
        """the mapped rows [B, N] of x [..., L] flattened to rows, before the class's view / repeat"""
        fcs = [getattr(block, "fc", block) for block in self.map_blocks]
        return _run_mapping(x.reshape(-1, x.shape[-1]), fcs, self.normalise, self.slope, fused)


@MAPPINGS.register("MappingToLatent")
class VAEMappingToLatent_old(_MapBlocks):
    def __init__(self, mapping_layers=5, latent_size=256, dlatent_size=256, mapping_fmaps=256):
        super().__init__(mapping_layers, latent_size, mapping_fmaps, 2 * dlatent_size, MappingBlock)

    def forward(self, x):  # ([B, 1, L] from the encoder: flattened to rows)
        y = self.map(x)
        return y.view(x.shape[0], 2, y.shape[1] // 2)


@MAPPINGS.register("MappingToLatentNoStyle")
class VAEMappingToLatentNoStyle(_MapBlocks):
    def __init__(self, mapping_layers=5, latent_size=256, dlatent_size=256, mapping_fmaps=256):
        super().__init__(mapping_layers, latent_size, mapping_fmaps, dlatent_size,
                         lambda a, b, lrmul: _LreqLinear(a, b, lrmul=lrmul))

    slope = None

    def forward(self, x):
        y = self.map(x)
        return y.view(*x.shape[:-1], y.shape[1])


@MAPPINGS.register("MappingFromLatent")
class VAEMappingFromLatent(_MapBlocks):
    def __init__(self, num_layers, mapping_layers=5, latent_size=256, dlatent_size=256, mapping_fmaps=256):
        super().__init__(mapping_layers, dlatent_size, mapping_fmaps, latent_size, MappingBlock)
        self.num_layers = num_layers

    normalise = True

    def forward(self, x):
        x = self.map(x)
        return x.view(x.shape[0], 1, x.shape[1]).repeat(1, self.num_layers, 1)
