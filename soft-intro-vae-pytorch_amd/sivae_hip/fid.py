"""FID on the device (reference: soft_intro_vae/metrics/fid_score.py): everything around the Inception network.

The reference copies every activation batch to the host (:197, :262), keeps 2 x num_images x dims float64 there, takes
np.mean / np.cov (:349-350, :375-376) and scipy's sqrtm of a non-symmetric product (:307).  Here

    stats = ActivationStatistics(dims, device)        # fp64 moments (n, s = sum of rows, G = A^T A), csrc/fid.hip
    stats.update(act)                                  # [b, d], [b, d, 1, 1] or [b, d, h, w] fp32 on the device
    mu, sigma = stats.finalize()                       # fp64 device tensors: np.mean / np.cov of the rows seen
    fid = frechet_distance(mu1, sigma1, mu2, sigma2)   # symmetric eigenvalue form, a Python float
    fid = calculate_fid_given_dataset(loader, model_s, batch_size, True, 2048, device, 50000)   # the reference's call

The Inception network itself stays a torch module that is passed in (default: the reference's metrics.inception); its
cost is unchanged.  The moment state is additive (`merge`), so a pass sharded over ranks needs one sum of (n, s, G).
There is no CPU path.
"""
import os
import warnings

import numpy as np
import torch

from . import infer, ops

# SIVAE_FID_EIGH=device|cpu: where the two symmetric eigen-decompositions of frechet_distance run (plumbing: torch's
# solver).  "device" is torch's ROCm solver (measured: 98 ms a distance at d = 2048 against 474 ms); "cpu" works on host
# copies of the d x d matrices (32 MB each at d = 2048), for a torch build without a device solver.
EIGH = os.environ.get("SIVAE_FID_EIGH", "device")


def activation_rows(act, dims):
    """what `ActivationStatistics.update` accepts -> rows [b, dims]: [b, d], [b, d, 1, 1] or [b, d, h, w] (averaged over
    h, w) float32 on the device"""
    if not isinstance(act, torch.Tensor) or not act.is_cuda or act.dtype != torch.float32:
        raise TypeError("sivae_hip.fid: activations must be a float32 ROCm tensor (no CPU fallback)")
    if act.dim() == 4:
        if act.shape[2] != 1 or act.shape[3] != 1:  # fid_score.py:195-196
            act = torch.nn.functional.adaptive_avg_pool2d(act, output_size=(1, 1))
        act = act.reshape(act.shape[0], -1)
    if act.dim() != 2 or act.shape[1] != dims:
        raise ValueError("sivae_hip.fid: expected activations [b, %d], [b, %d, 1, 1] or [b, %d, h, w], got %s"
                         % (dims, dims, dims, tuple(act.shape)))
    return act


class ActivationStatistics:
    """Running first and second moments of activation rows, in fp64 on the device.

    Rows are collected in a staging buffer and given to the moment kernel in blocks of exactly `flush_rows` rows (and one
    remainder), so the result depends only on the row sequence, not on how `update` was fed.  The last full block is
    held back until the next one is full: `finalize(num)` can then cut inside it and still runs the arithmetic of the
    truncated sequence."""

    def __init__(self, dims, device, flush_rows=1024):
        self.dims, self.device, self.flush_rows = int(dims), torch.device(device), int(flush_rows)
        if self.device.type != "cuda":
            raise RuntimeError("sivae_hip.fid.ActivationStatistics: device %s is not a ROCm device (no CPU fallback)"
                               % self.device)
        if self.flush_rows < 1:
            raise ValueError("flush_rows must be positive")
        self.G, self.s = ops.fid_state(self.dims, self.device)
        self.n = 0                # rows in (G, s)
        self._held = None         # a full block that is not in (G, s) yet
        self._stage = ops.fid_staging(self.flush_rows, self.dims, self.device)
        self._fill = 0            # rows in _stage
        self._spare = None        # the second staging buffer while no block is held

    @property
    def rows_seen(self):
        return self.n + (self.flush_rows if self._held is not None else 0) + self._fill

    def _rows(self, act):
        return activation_rows(act, self.dims)

    def _flush_held(self):
        if self._held is not None:
            ops.fid_moments(self._held, self.flush_rows, self.G, self.s)
            self.n += self.flush_rows
            self._held, self._spare = None, self._held

    @torch.no_grad()
    def update(self, act):
        if act.shape[0] == 0:
            return self
        act = self._rows(act)
        at = 0
        while at < act.shape[0]:
            if self._fill == self.flush_rows:
                # a row for the next block: the held block goes into the moments, the full one is held in its place
                self._flush_held()
                spare = self._spare
                if spare is None:
                    spare = ops.fid_staging(self.flush_rows, self.dims, self.device)
                self._held, self._stage, self._spare, self._fill = self._stage, spare, None, 0
            take = min(self.flush_rows - self._fill, act.shape[0] - at)
            self._stage[self._fill:self._fill + take].copy_(act[at:at + take])
            self._fill += take
            at += take
        return self

    @torch.no_grad()
    def state(self, num=None):
        """-> the additive moment state (n, s, G) over the first `num` rows seen (all of them by default), on copies: the
        accumulator is unchanged.  G holds A^T A on the 64 x 64 block tiles on and above the diagonal, zeros below."""
        seen = self.rows_seen
        num = seen if num is None else int(num)
        if num > seen or num < 0:
            raise ValueError("sivae_hip.fid: %d rows asked for, %d seen" % (num, seen))
        if num < self.n:
            raise ValueError("sivae_hip.fid: finalize(num) can cut at most into the last full block: rows before %d "
                             "are already in the moments, num = %d" % (self.n, num))
        G, s = ops.fid_state_copy(self.G, self.s)
        n = self.n
        for block, rows in ((self._held, self.flush_rows if self._held is not None else 0), (self._stage, self._fill)):
            take = min(rows, num - n)
            if take > 0:
                ops.fid_moments(block, take, G, s)
                n += take
        return n, s, G

    @torch.no_grad()
    def merge(self, other):
        """add another accumulator's rows (its state is left as it is); this one's pending rows go into its moments
        first"""
        if other.dims != self.dims:
            raise ValueError("sivae_hip.fid: merge of %d-dimensional into %d-dimensional statistics"
                             % (other.dims, self.dims))
        self.n, self.s, self.G = self.state()
        if self._held is not None:
            self._held, self._spare = None, self._held
        self._fill = 0
        n, s, G = other.state()
        self.G += G.to(self.device)
        self.s += s.to(self.device)
        self.n += n
        return self

    @torch.no_grad()
    def finalize(self, num=None):
        """-> (mu [d], sigma [d, d]) fp64 on the device over exactly the first `num` rows seen (fid_score.py:203, :265:
        activations[:num_images]); the accumulator can be updated further afterwards"""
        n, s, G = self.state(num)
        if n < 1:
            raise ValueError("sivae_hip.fid: no rows to take statistics of")
        if n == 1:  # what np.cov says of one observation
            warnings.warn("Degrees of freedom <= 0 for slice", RuntimeWarning, stacklevel=2)
        return ops.fid_finalize(G, s, n)


def _f64_on(x, device):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=torch.float64)
    return torch.as_tensor(np.asarray(x, dtype=np.float64)).to(device)


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    if not torch.cuda.is_available():
        raise RuntimeError("sivae_hip.fid.frechet_distance: no ROCm device (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _eigh(a, vectors):
    """symmetric eigen-decomposition through torch (plumbing), on the device or on a host copy (EIGH)"""
    if EIGH not in ("device", "cpu"):
        raise ValueError("SIVAE_FID_EIGH must be 'device' or 'cpu', got %r" % EIGH)
    m = a if EIGH == "device" else a.cpu()
    if vectors:
        w, v = torch.linalg.eigh(m)
        return w.to(a.device), v.to(a.device)
    return torch.linalg.eigvalsh(m).to(a.device)


@torch.no_grad()
def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + Tr sigma1 + Tr sigma2 - 2 Tr (sigma1 sigma2)^(1/2)  (fid_score.py:274-325), a Python float.

    sigma1 sigma2 is similar to R sigma2 R with R = sigma1^(1/2), which is symmetric positive semi-definite: the trace of
    the square root is the sum of the square roots of its eigenvalues.  No non-symmetric square root, no complex or
    singular fallback.  numpy arrays, CPU tensors and device tensors are accepted."""
    dev = _device_of(mu1, sigma1, mu2, sigma2)
    mu1, sigma1, mu2, sigma2 = (_f64_on(x, dev) for x in (mu1, sigma1, mu2, sigma2))
    mu1, mu2 = mu1.reshape(-1), mu2.reshape(-1)
    d = mu1.shape[0]
    if mu2.shape != mu1.shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if tuple(sigma1.shape) != (d, d) or tuple(sigma2.shape) != (d, d):
        raise ValueError("Training and test covariances have different dimensions")
    w, v = _eigh(sigma1, True)
    x = (v * w.clamp_min(0.0).pow(0.25)).t().contiguous()      # diag(max(w, 0)^(1/4)) V^T
    r = ops.fid_xty(x, x, symmetric=True)                       # R = sigma1^(1/2)
    t = ops.fid_xty(sigma2.contiguous(), r)                     # T = sigma2^T R
    m = ops.fid_xty(r, t, symmetric=True)                       # M = R^T T = R sigma2 R
    lam = _eigh(m, False)
    diff = mu1 - mu2
    value = diff.dot(diff) + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * lam.clamp_min(0.0).sqrt().sum()
    return float(value.item())


def reference_inception(dims):
    from metrics.inception import InceptionV3  # the reference's metrics package (needs torchvision and its weights)
    return InceptionV3([InceptionV3.BLOCK_INDEX_BY_DIM[dims]])


@torch.no_grad()
def calculate_fid_given_dataset(dataloader, model_s, batch_size, cuda, dims, device, num_images, inception=None,
                                real_stats=None):
    """The reference's fid_score.py:454-470 with its parameters in its order, on the device.

    inception: any module whose call returns a sequence with the feature map first (default: the reference's
        metrics.inception.InceptionV3([BLOCK_INDEX_BY_DIM[dims]]), imported lazily); its mode is left as found (the
        reference never calls .eval() on it).
    real_stats: (mu, sigma) of the real side, which is then skipped (`real_statistics` computes them).
    Nothing is copied to the host before the final scalar."""
    device = torch.device(device)
    if inception is None:
        inception = reference_inception(dims)
    if cuda:
        inception.to(device)
    if real_stats is None:
        real_stats = real_statistics(dataloader, inception, dims, device, num_images, cuda=cuda)
    m1, s1 = real_stats
    stats = ActivationStatistics(dims, device)
    for images in infer.generate(model_s, num_images, batch_size, as_uint8=True, eval_mode=None):
        act = inception(ops.u8_to_f32(images))[0]
        stats.update(act[:num_images - stats.rows_seen])
    print("total generated activations: ", (stats.rows_seen, dims))
    m2, s2 = stats.finalize()
    return frechet_distance(m1, s1, m2, s2)


@torch.no_grad()
def real_statistics(dataloader, inception, dims, device, num_images, cuda=True):
    """(mu, sigma) of the first num_images images the loader yields (fid_score.py:181-203), fp64 on the device"""
    device = torch.device(device)
    stats = ActivationStatistics(dims, device)
    for batch in dataloader:
        if isinstance(batch, (list, tuple)) and len(batch) in (2, 3):  # (images, labels[, ...]): fid_score.py:182-183
            batch = batch[0]
        if cuda:
            batch = batch.to(device)
        act = inception(batch)[0]
        stats.update(act[:num_images - stats.rows_seen])
        if stats.rows_seen >= num_images:
            break
    print("total real activations: ", (stats.rows_seen, dims))
    return stats.finalize()
