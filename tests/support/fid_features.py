"""What the FID tests share: the fixture tests/golden/fid.npz unpacked (tests/golden/make_golden_fid.py states what it
holds) and the stand-in feature network of its loader case."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "fid.npz")
FULL_RANK = ((16, 64), (48, 200), (64, 512), (192, 1000))
RANK_DEFICIENT = (64, 50)
_cache = {}


def _full(triu, d):
    sigma = np.zeros((d, d))
    sigma[np.triu_indices(d)] = triu
    return sigma + np.triu(sigma, 1).T


def fixture():
    """-> the npz as a dict (read once)"""
    if "z" not in _cache:
        with np.load(GOLDEN) as z:
            _cache["z"] = {k: z[k] for k in z.files}
    return _cache["z"]


def pair(d, n):
    """-> dict(act1, act2 float32 [n, d]; mu1, mu2 float32; sigma1, sigma2 float64 [d, d]; fid, fid_f32, sqrtm_imag)"""
    key = (d, n)
    if key not in _cache:
        z, p = fixture(), "p%d_%d_" % (d, n)
        _cache[key] = dict(act1=z[p + "q1"].astype(np.float32) / np.float32(32),
                           act2=z[p + "q2"].astype(np.float32) / np.float32(32), mu1=z[p + "mu1"], mu2=z[p + "mu2"],
                           sigma1=_full(z[p + "sigma1_triu"], d), sigma2=_full(z[p + "sigma2_triu"], d),
                           fid=float(z[p + "fid"]), fid_f32=float(z[p + "fid_f32"]),
                           sqrtm_imag=float(z[p + "sqrtm_imag"]))
    return _cache[key]


class Features(torch.nn.Module):
    """one 3 x 3 convolution (non-negative weights and bias: on images in [0, 1) no sum cancels) + ReLU; the call
    returns a list with the [b, 16, h, w] feature map first, as the reference's Inception wrapper does"""

    def __init__(self, weight, bias):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 16, 3, padding=1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.as_tensor(weight))
            self.conv.bias.copy_(torch.as_tensor(bias))

    def forward(self, x):
        return [torch.relu(self.conv(x))]


def loader_case():
    """-> (list of (images, labels) CPU batches, Features on the CPU, num_images, batch, mu float32, sigma float64)"""
    z = fixture()
    images, labels = torch.from_numpy(z["loader_images"]), torch.from_numpy(z["loader_labels"])
    b = int(z["loader_batch"])
    batches = [(images[i:i + b], labels[i:i + b]) for i in range(0, images.shape[0], b)]
    return (batches, Features(z["loader_weight"], z["loader_bias"]), int(z["loader_num_images"]), b, z["loader_mu"],
            z["loader_sigma"])
