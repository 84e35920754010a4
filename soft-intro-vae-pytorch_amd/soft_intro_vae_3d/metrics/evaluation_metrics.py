"""Minimum matching distance and coverage of two sets of point clouds, on a Chamfer matrix (MMD-CD, COV-CD) or an earth
mover's matrix (MMD-EMD, COV-EMD): the figures the reference's README (soft_intro_vae_3d/README.md:47-48) sends the arrays
of evaluation/generate_data_for_metrics.py to the latent_3d_points evaluation notebook for.  The function names,
signatures and return types are that notebook's (`minimum_mathing_distance` is its spelling); the work runs on the kernels
of csrc/pc_eval.hip and csrc/pc_emd.hip through `sivae_hip.pointcloud`.  Inputs are ROCm tensors, CPU tensors or numpy
arrays [S, N, 3]; host data is uploaded once.  No TensorFlow session (`sess`, `batch_size` and `verbose` are accepted and
ignored: the whole matrix is one walk over the rows on the device).

    D = chamfer_matrix(sample_pcs, ref_pcs)               # pay for the matrix once ...
    mmd, matched_dists = minimum_mathing_distance(sample_pcs, ref_pcs, dist=D)
    cov, matched_ref = coverage(sample_pcs, ref_pcs, dist=D)
    mmd_emd, _ = minimum_mathing_distance(x_g, x, dist=emd_matrix(x_g, x))   # the earth mover's figures: the same calls
"""
import os
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (where sivae_hip lies)
if _PKG not in sys.path:
    sys.path.append(_PKG)
from sivae_hip import pointcloud as PC  # noqa: E402

__all__ = ['chamfer_matrix', 'emd_matrix', 'minimum_mathing_distance', 'minimum_matching_distance', 'coverage']


def _device_of(*arrays):
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    if not torch.cuda.is_available():
        raise RuntimeError("sivae_hip: the point-cloud metrics need a ROCm device and have no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _clouds(pcs, device, name):
    """-> a float32 tensor [S, N, 3] on `device`; a device tensor is taken as it is (any strides)"""
    if not isinstance(pcs, torch.Tensor):
        pcs = torch.from_numpy(np.ascontiguousarray(pcs, dtype=np.float32))
    if pcs.dim() != 3 or pcs.shape[2] != 3 or pcs.shape[0] == 0 or pcs.shape[1] == 0:
        raise ValueError("%s: expected point clouds [S, N, 3], got %s" % (name, tuple(pcs.shape)))
    if pcs.dtype != torch.float32:
        pcs = pcs.float()
    return pcs if pcs.device == device else pcs.to(device)


def chamfer_matrix(sample_pcs, ref_pcs, normalize=True, use_sqrt=False):
    """D [S, R] float32 on the device, D[s, r] = CD(sample_s, ref_r): the mean (the sum without `normalize`) over the
    points of each cloud of the squared distance (its root with `use_sqrt`) to the nearest point of the other, added"""
    for name, pcs in (("sample_pcs", sample_pcs), ("ref_pcs", ref_pcs)):  # (the shape error before any device is asked for)
        if np.ndim(pcs) != 3 or np.shape(pcs)[2] != 3:
            raise ValueError("%s: expected point clouds [S, N, 3], got %s" % (name, tuple(np.shape(pcs))))
    dev = _device_of(sample_pcs, ref_pcs)
    return PC.chamfer_matrix(_clouds(sample_pcs, dev, "sample_pcs"), _clouds(ref_pcs, dev, "ref_pcs"), normalize, use_sqrt)


def emd_matrix(sample_pcs, ref_pcs, normalize=True):
    """D [S, R] float32 on the device, D[s, r] = EMD(ref_r, sample_s): the cost of the approximate matching (the notebook's
    approxmatch / matchcost pair) of the two clouds, divided by the larger point count with `normalize`.  At most 4096
    points a cloud.  `dist=` of the two functions below takes it: MMD-EMD and COV-EMD."""
    for name, pcs in (("sample_pcs", sample_pcs), ("ref_pcs", ref_pcs)):  # (the shape error before any device is asked for)
        if np.ndim(pcs) != 3 or np.shape(pcs)[2] != 3:
            raise ValueError("%s: expected point clouds [S, N, 3], got %s" % (name, tuple(np.shape(pcs))))
    dev = _device_of(sample_pcs, ref_pcs)
    return PC.emd_matrix(_clouds(sample_pcs, dev, "sample_pcs"), _clouds(ref_pcs, dev, "ref_pcs"), normalize)


def _matrix(sample_pcs, ref_pcs, normalize, use_sqrt, use_EMD, dist):
    if use_EMD:
        raise NotImplementedError("use_EMD is not wired to the earth mover's matrix: pass dist=emd_matrix(sample_pcs, "
                                  "ref_pcs) for MMD-EMD / COV-EMD")
    if dist is None:
        dist = chamfer_matrix(sample_pcs, ref_pcs, normalize, use_sqrt)
    else:
        if not isinstance(dist, torch.Tensor):
            dist = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32))
        if dist.dim() != 2:
            raise ValueError("dist: expected a matrix [S, R], got %s" % (tuple(dist.shape),))
        if not dist.is_cuda:
            dist = dist.to(_device_of(sample_pcs, ref_pcs))
        dist = dist.float().contiguous()
    if not bool(torch.isfinite(dist).all()):
        raise ValueError("the distance matrix has %d non-finite entries (a cloud with a NaN or infinite coordinate?)"
                         % int((~torch.isfinite(dist)).sum()))
    return dist


def minimum_mathing_distance(sample_pcs, ref_pcs, batch_size=None, normalize=True, sess=None, verbose=False, use_sqrt=False,
                             use_EMD=False, dist=None):
    """-> (mmd: float, matched_dists: float32 numpy [R]): for every reference cloud the distance of the sample cloud
    nearest to it, and their mean.  `dist`: a matrix from `chamfer_matrix` or `emd_matrix` (the flags are then its own)."""
    D = _matrix(sample_pcs, ref_pcs, normalize, use_sqrt, use_EMD, dist)
    _, _, col_min, _ = PC.match_min(D)
    matched_dists = col_min.cpu().numpy()
    return float(np.mean(matched_dists, dtype=np.float64)), matched_dists


minimum_matching_distance = minimum_mathing_distance


def coverage(sample_pcs, ref_pcs, batch_size=None, normalize=True, sess=None, verbose=False, use_sqrt=False, use_EMD=False,
             ret_dist=False, dist=None):
    """-> (cov: float, matched_ref: int numpy [S][, matched_dist: float32 numpy [S]]): every sample cloud is matched to its
    nearest reference cloud (the lowest index on a tie); cov is the fraction of the reference clouds matched at least
    once."""
    D = _matrix(sample_pcs, ref_pcs, normalize, use_sqrt, use_EMD, dist)
    row_min, row_arg, _, _ = PC.match_min(D)
    matched_ref = row_arg.cpu().numpy().astype(np.int64)
    cov = len(np.unique(matched_ref)) / float(D.shape[1])
    if ret_dist:
        return cov, matched_ref, row_min.cpu().numpy()
    return cov, matched_ref
