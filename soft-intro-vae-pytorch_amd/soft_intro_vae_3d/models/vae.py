"""The networks of the reference's soft_intro_vae_3d/models/vae.py on the HIP kernels of sivae_hip: same class names,
constructor arguments, method names, return orders, parameter shapes and state_dict keys, so the reference's
train_soft_intro_vae_3d.py and its checkpoints (strict=True) work unchanged.  No CPU path."""
import os
import sys

import torch
import torch.nn as nn

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (where sivae_hip lies)
if _PKG not in sys.path:
    sys.path.append(_PKG)
from sivae_hip import functional as SF  # noqa: E402
from sivae_hip import pointcloud as PC  # noqa: E402
from sivae_hip.engine import reparameterize  # noqa: E402,F401  (reference API; eps from the device Philox stream)


def _mlp(layers, x):
    """nn.Sequential of nn.Linear / nn.ReLU: each Linear with the ReLU behind it fused"""
    mods = list(layers)
    i = 0
    while i < len(mods):
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
        x = SF.linear(x, mods[i].weight, mods[i].bias, relu=relu)
        i += 2 if relu else 1
    return x


class Decoder(nn.Module):
    """reference :21-47"""

    def __init__(self, config):
        super().__init__()
        self.z_size = config['z_size']
        self.use_bias = config['model']['D']['use_bias']
        self.relu_slope = config['model']['D']['relu_slope']
        widths = (self.z_size, 64, 128, 512, 1024, 2048 * 3)
        layers = []
        for i in range(5):
            layers.append(nn.Linear(in_features=widths[i], out_features=widths[i + 1], bias=self.use_bias))
            if i < 4:
                layers.append(nn.ReLU(inplace=True))
        self.model = nn.Sequential(*layers)

    def forward(self, input):
        z = input.squeeze()
        if z.dim() == 1:  # (a batch of one arrives 1-D, as in the reference)
            z = z.unsqueeze(0)
        return _mlp(self.model, z).view(-1, 3, 2048)


def _heads(enc, pooled):
    logit = _mlp(enc.fc, pooled)
    return (SF.linear(logit, enc.mu_layer.weight, enc.mu_layer.bias),
            SF.linear(logit, enc.std_layer.weight, enc.std_layer.bias))


class EncoderNoBatchNorm(nn.Module):
    """reference :50-93"""

    def __init__(self, config):
        super().__init__()
        self.z_size = config['z_size']
        self.use_bias = config['model']['E']['use_bias']
        self.relu_slope = config['model']['E']['relu_slope']
        widths = (3, 64, 128, 256, 256, 512)
        layers = []
        for i in range(5):
            layers.append(nn.Conv1d(in_channels=widths[i], out_channels=widths[i + 1], kernel_size=1, bias=self.use_bias))
            if i < 4:
                layers.append(nn.ReLU(inplace=True))
        self.conv = nn.Sequential(*layers)
        self.fc = nn.Sequential(nn.Linear(512, 256, bias=True), nn.ReLU(inplace=True))
        self.mu_layer = nn.Linear(256, self.z_size, bias=True)
        self.std_layer = nn.Linear(256, self.z_size, bias=True)

    def forward(self, x):
        mods = list(self.conv)
        i = 0
        while i < len(mods):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            x = PC.pointwise_conv(x, mods[i].weight, mods[i].bias, relu=relu)
            i += 2 if relu else 1
        return _heads(self, PC.max_points(x))


class Encoder(nn.Module):
    """reference :96-145: five stages Conv1d(k=1, no bias) -> ReLU -> BatchNorm1d, max over the points, fc, two heads"""

    def __init__(self, config):
        super().__init__()
        self.z_size = config['z_size']
        self.use_bias = config['model']['E']['use_bias']
        self.relu_slope = config['model']['E']['relu_slope']
        widths = (3, 64, 128, 256, 256, 512)
        layers = []
        for i in range(5):
            layers += [nn.Conv1d(in_channels=widths[i], out_channels=widths[i + 1], kernel_size=1, bias=False),
                       nn.ReLU(inplace=True), nn.BatchNorm1d(widths[i + 1])]
        self.conv = nn.Sequential(*layers)
        self.fc = nn.Sequential(nn.Linear(512, 256, bias=True), nn.ReLU(inplace=True))
        self.mu_layer = nn.Linear(256, self.z_size, bias=True)
        self.std_layer = nn.Linear(256, self.z_size, bias=True)

    def forward(self, x):
        mods = list(self.conv)
        for i in range(0, len(mods), 3):
            bn = mods[i + 2]
            a = PC.pointwise_conv(x, mods[i].weight, None)
            if i + 3 == len(mods) and PC.RELU_BN_MAX:  # (the last stage and the max in one piece: y is never stored)
                return _heads(self, PC.relu_bn_max(a, bn.weight, bn.bias, SF.BNState(bn)))
            x = PC.relu_bn(a, bn.weight, bn.bias, SF.BNState(bn))
        return _heads(self, PC.max_points(x))


class SoftIntroVAE(nn.Module):
    """reference :148-181; forward returns (y, mu, logvar)"""

    def __init__(self, config):
        super(SoftIntroVAE, self).__init__()
        self.zdim = config['z_size']
        self.encoder = Encoder(config)
        self.decoder = Decoder(config)

    def forward(self, x, deterministic=False):
        mu, logvar = self.encoder(x)
        z = mu if deterministic else reparameterize(mu, logvar)
        return self.decoder(z), mu, logvar

    def sample(self, z):
        return self.decode(z)

    def sample_with_noise(self, num_samples=1, device=torch.device("cpu")):
        from sivae_hip import rng
        return self.decode(rng.randn((num_samples, self.zdim), device))

    def encode(self, x):
        return self.encoder(x)

    def decode(self, z):
        return self.decoder(z)


class SoftIntroVAEBootstrap(nn.Module):
    """reference :184-229: a second, target decoder"""

    def __init__(self, config):
        super(SoftIntroVAEBootstrap, self).__init__()
        self.zdim = config['z_size']
        self.encoder = Encoder(config)
        self.decoder = Decoder(config)
        self.target_decoder = Decoder(config)

    def forward(self, x, deterministic=False, use_target_decoder=True):
        mu, logvar = self.encoder(x)
        z = mu if deterministic else reparameterize(mu, logvar)
        y = self.target_decoder(z) if use_target_decoder else self.decoder(z)
        return y, mu, logvar

    def sample(self, z, use_target_decoder=False):
        return self.decode_target(z) if use_target_decoder else self.decode(z)

    def sample_with_noise(self, num_samples=1, device=torch.device("cpu")):
        from sivae_hip import rng
        return self.decode(rng.randn((num_samples, self.zdim), device))

    def encode(self, x):
        return self.encoder(x)

    def decode(self, z):
        return self.decoder(z)

    def decode_target(self, z):
        return self.target_decoder(z)
