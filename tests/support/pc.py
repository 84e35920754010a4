"""What the point-cloud GPU tests share (test_pointcloud*_gpu, test_relu_bn_max_gpu, test_pc_*_gpu, the point-cloud part of
test_guarded_kernels_gpu): the device, the lazy import of the wrappers, device copies, the project's element-wise
criterion, the Chamfer cases and the encoder / model helpers.  Tolerances are stated in tests/test_pointcloud_gpu.py."""
import functools

import numpy as np
import torch

import pc3d_oracle as O

DEV = "cuda:0"


def _PC():
    from sivae_hip import pointcloud as PC
    return PC


def _np(t):
    return t.cpu().numpy()


def put(t, misaligned=False):
    """device copy of t (a tensor, or a numpy array that may be read-only); misaligned: contiguous, 4 bytes behind a
    16-byte boundary (carved one element into a larger buffer)"""
    if not torch.is_tensor(t):
        t = torch.from_numpy(np.array(t))
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def viol(a, b, rtol=1e-4, atol_scale=1e-5):
    """the project's element-wise criterion |a - b| <= rtol |b| + atol_scale max|b| as a ratio: <= 1 passes; a non-finite
    `a` never does"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    atol = atol_scale * float(b.abs().max())
    return float(((a - b).abs() / (rtol * b.abs() + atol + 1e-300)).max())


@functools.lru_cache(maxsize=None)
def _chamfer_case(B, N, M, seed):
    """-> (preds fp32 [B, M, 3], gts fp32 [B, N, 3], fp64 pairwise distances [B, N, M], fp64 loss [B])"""
    g = torch.Generator().manual_seed(seed)
    gts = torch.rand(B, N, 3, generator=g, dtype=torch.float64).float()
    preds = torch.rand(B, M, 3, generator=g, dtype=torch.float64).float()
    P = O.pairwise_sqdist(preds.double(), gts.double())
    return preds, gts, P, P.min(dim=1)[0].sum(1) + P.min(dim=2)[0].sum(1)


def _check_indices_by_distance(P, idx_p, idx_g):
    """P [B, N, M] fp64; idx_p [B, M] into the N ground-truth points, idx_g [B, N] into the M predictions"""
    B, N, M = P.shape
    idx_p, idx_g = idx_p.cpu().long(), idx_g.cpu().long()
    assert idx_p.min() >= 0 and idx_p.max() < N and idx_g.min() >= 0 and idx_g.max() < M
    dp = P.gather(1, idx_p[:, None, :])[:, 0, :]
    dg = P.gather(2, idx_g[:, :, None])[:, :, 0]
    mp, mg = P.min(dim=1)[0], P.min(dim=2)[0]
    worst = max(float(((dp - mp) / mp.clamp_min(1e-300)).max()), float(((dg - mg) / mg.clamp_min(1e-300)).max()))
    assert worst <= 1e-5, worst


class _BN:
    """what functional.BNState reads from a BatchNorm module"""

    def __init__(self, C, training, seed):
        g = torch.Generator().manual_seed(seed)
        self.running_mean = (torch.rand(C, generator=g) * 0.2 - 0.1).to(DEV)
        self.running_var = (torch.rand(C, generator=g) + 0.5).to(DEV)
        self.num_batches_tracked = torch.tensor(3, dtype=torch.int64, device=DEV)
        self.training, self.eps, self.momentum = training, 1e-5, 0.1


def _load(module, sd, prefix=""):
    module.load_state_dict({k[len(prefix):]: v.detach().clone().float() for k, v in sd.items() if k.startswith(prefix)},
                           strict=True)
    return module.to(DEV)


def _grad_report(name, named_params, sd64, sd32, prefix=""):
    """per-tensor relative L2 of the GPU gradient against fp64, gated by max(4 e32, 1e-5)"""
    bad = []
    for k, p in named_params:
        ref = sd64[prefix + k].grad
        e_gpu, e32 = O.rel_l2(p.grad, ref), O.rel_l2(sd32[prefix + k].grad, ref)
        gate = max(4 * e32, 1e-5)
        print("%s grad %-28s gpu %.3e  cpu-fp32 %.3e  gate %.3e" % (name, k, e_gpu, e32, gate))
        if not e_gpu <= gate:
            bad.append((k, e_gpu, gate))
    assert not bad, bad
