"""Generate the FID fixture from the REAL reference (runs only where the reference checkout is mounted; needs the scipy
the reference imports).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fid.py /path/to/reference

The reference's soft_intro_vae/metrics/fid_score.py is imported BY FILE PATH under a private module name.  It imports
torchvision (for the Inception network, which no case here runs) and PIL: where those are missing, an empty stand-in is
put into sys.modules (`models.inception.InceptionA/C/E` classes to subclass, a `models.utils` without the weight loader,
`utils`, `PIL.Image`).  fid.npz holds inputs and recorded results only:

  pairs  five seeded float32 activation pairs (d, n) = (16, 64), (48, 200), (64, 512), (192, 1000), (64, 50).  An
         activation is relu(z W + b) for normal z, rounded to a multiple of 1 / 32 below 8: non-negative and correlated,
         as pooled post-ReLU features are, and one byte an element in the file (`*_q`; act = q / 32 in float32, exactly),
         which keeps the fixture under the size limit of a committed file.  Of each side: the activations,
         mu = np.mean(act, axis=0) and sigma = np.cov(act, rowvar=False) as fid_score.py:349-350 takes them; sigma is
         exactly symmetric (asserted) and stored as its upper triangle, row by row (`*_triu`).  np.mean of the float32
         array the reference holds is a FLOAT32 mean (np.cov converts to float64), so mu is recorded as the float32 array
         the reference returns.
         fid     calculate_frechet_distance(mu1.astype(float64), sigma1, mu2.astype(float64), sigma2): the reference's
                 function on its own statistics, the means' VALUES unchanged, their difference taken in float64
         fid_f32 the same call with the float32 means as they come: |mu1 - mu2|^2 is then a float32 dot product
         For the four n > d cases the script asserts that sqrtm came back finite and real (no complex part at all, or
         imaginary parts below 1e-12 of the largest entry) and lambda_min(M) / lambda_max(M) >= 1e-6 for M = R sigma2 R.
         For (64, 50) it records the largest imaginary part of sqrtm's result.
  loader calculate_activation_statistics_given_dataset on the CPU: a stand-in feature network (one 3 x 3 convolution with
         NON-NEGATIVE weights and bias on images in [0, 1) + ReLU, 16 feature maps of 8 x 8 that the reference pools) and a
         list of five (images, labels) batches of 24 with num_images = 100: the fifth batch is cut.  Recorded: the images,
         the weights, the reference's mu (float32) and sigma.
"""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fid_oracle as FO  # noqa: E402

if len(sys.argv) != 2:
    raise SystemExit("usage: make_golden_fid.py /path/to/reference")
REF = os.path.join(os.path.abspath(sys.argv[1]), "soft_intro_vae")
PAIRS = ((16, 64), (48, 200), (64, 512), (192, 1000), (64, 50))


def _stand_in(name, **attrs):
    if name in sys.modules:
        return sys.modules[name]
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], leaf, m)
    return m


def import_reference():
    try:
        import torchvision  # noqa: F401
    except ImportError:
        _stand_in("torchvision", __version__="0.0")
        _stand_in("torchvision.models")
        _stand_in("torchvision.models.inception", InceptionA=type("InceptionA", (torch.nn.Module,), {}),
                  InceptionC=type("InceptionC", (torch.nn.Module,), {}),
                  InceptionE=type("InceptionE", (torch.nn.Module,), {}))
        _stand_in("torchvision.models.utils")
        _stand_in("torchvision.utils")
    try:
        import PIL.Image  # noqa: F401
    except ImportError:
        _stand_in("PIL")
        _stand_in("PIL.Image")
    sys.path.insert(0, REF)  # (its `from metrics.inception import InceptionV3`)
    saved_argv, sys.argv = sys.argv, sys.argv[:1]
    try:
        spec = importlib.util.spec_from_file_location("_ref_fid_score", os.path.join(REF, "metrics", "fid_score.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules["_ref_fid_score"] = mod
        spec.loader.exec_module(mod)
    finally:
        sys.argv = saved_argv
    return mod


def activations(g, d, n):
    """float32 [n, d]: relu(z W + b), W = I + a dense mixing of norm ~ 0.5: non-negative, correlated, full rank for n > d"""
    w = np.eye(d) + 0.5 * g.standard_normal((d, d)) / np.sqrt(d)
    b = 0.25 + 0.5 * g.random(d)
    z = g.standard_normal((n, d))
    q = np.minimum(np.round(np.maximum(z @ w + b, 0.0) * 32.0), 255.0).astype(np.uint8)
    assert (q == 255).mean() < 1e-3
    return q


class Features(torch.nn.Module):
    """the stand-in feature network of the loader case (tests/support/fid_features.py is the tests' copy)"""

    def __init__(self, weight, bias):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 16, 3, padding=1)
        with torch.no_grad():
            self.conv.weight.copy_(torch.from_numpy(weight))
            self.conv.bias.copy_(torch.from_numpy(bias))

    def forward(self, x):
        return [torch.relu(self.conv(x))]


if __name__ == "__main__":
    ref = import_reference()
    from scipy import linalg
    g = np.random.Generator(np.random.PCG64(2031))
    out = {"pairs": np.array(PAIRS, dtype=np.int32)}
    for d, n in PAIRS:
        key = "p%d_%d_" % (d, n)
        q1, q2 = activations(g, d, n), activations(g, d, n)
        a1, a2 = q1.astype(np.float32) / np.float32(32), q2.astype(np.float32) / np.float32(32)
        assert a1.dtype == np.float32 and (a1 >= 0).all() and (a2 >= 0).all()
        mu1, sigma1 = np.mean(a1, axis=0), np.cov(a1, rowvar=False)   # fid_score.py:349-350
        mu2, sigma2 = np.mean(a2, axis=0), np.cov(a2, rowvar=False)
        assert mu1.dtype == np.float32 and sigma1.dtype == np.float64
        assert np.array_equal(sigma1, sigma1.T) and np.array_equal(sigma2, sigma2.T)
        fid = ref.calculate_frechet_distance(mu1.astype(np.float64), sigma1, mu2.astype(np.float64), sigma2)
        fid_f32 = ref.calculate_frechet_distance(mu1, sigma1, mu2, sigma2)
        covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
        imag = float(np.abs(covmean.imag).max()) if np.iscomplexobj(covmean) else 0.0
        assert np.isfinite(covmean).all()
        lam = np.linalg.eigvalsh(FO.inner_matrix(sigma1, sigma2))
        if n > d:
            assert imag <= 1e-12 * np.abs(covmean).max(), (d, n, imag)
            assert lam.min() / lam.max() >= 1e-6, (d, n, lam.min() / lam.max())
        mine = FO.frechet_distance(mu1, sigma1, mu2, sigma2)
        print("(%3d, %4d): fid %.15g (float32 means %.9g), oracle rel %.2e, sqrtm imag %.1e, lambda min/max %.2e, |dmu|^2 "
              "%.4g" % (d, n, fid, fid_f32, abs(mine - fid) / abs(fid), imag, lam.min() / lam.max(),
                        float(((mu1.astype(np.float64) - mu2) ** 2).sum())))
        iu = np.triu_indices(d)
        out.update({key + "q1": q1, key + "q2": q2, key + "mu1": mu1, key + "mu2": mu2, key + "sigma1_triu": sigma1[iu],
                    key + "sigma2_triu": sigma2[iu], key + "fid": np.float64(fid), key + "fid_f32": np.float64(fid_f32),
                    key + "sqrtm_imag": np.float64(imag)})

    weight = (g.random((16, 3, 3, 3)) * (g.random((16, 3, 1, 1)) < 0.7) / 8.0).astype(np.float32)
    bias = (0.05 * g.random(16)).astype(np.float32)
    images = g.random((120, 3, 8, 8), dtype=np.float32)
    labels = g.integers(0, 10, 120)
    net = Features(weight, bias)
    loader = [(torch.from_numpy(images[i:i + 24]), torch.from_numpy(labels[i:i + 24])) for i in range(0, 120, 24)]
    with torch.no_grad():
        mu, sigma = ref.calculate_activation_statistics_given_dataset(loader, net, 24, 16, False, False,
                                                                      torch.device("cpu"), 100)
    assert mu.shape == (16,) and mu.dtype == np.float32 and sigma.shape == (16, 16) and sigma.dtype == np.float64
    out.update(loader_images=images, loader_labels=labels.astype(np.int64), loader_weight=weight, loader_bias=bias,
               loader_mu=mu, loader_sigma=sigma, loader_num_images=np.int32(100), loader_batch=np.int32(24))
    path = os.path.join(HERE, "fid.npz")
    np.savez_compressed(path, **out)
    print("fid.npz: %d bytes" % os.path.getsize(path))
