"""Drop-in for the reference's soft_intro_vae_3d/metrics/jsd.py: the same names, signatures and return types, on the
kernels of csrc/pc_jsd.hip through `sivae_hip.pointcloud`.  The point clouds are ROCm tensors ([S, N, 3], any strides:
the `transpose_(1, 2)` view of a decoder output is read in place) and never leave the device; only the counters
(a few thousand integers) and the result do.  No scipy, no scikit-learn."""
import os
import sys

import numpy as np
import torch

_PKG = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (where sivae_hip lies)
if _PKG not in sys.path:
    sys.path.append(_PKG)
from sivae_hip import pointcloud as PC  # noqa: E402

__all__ = ['js_divercence_between_pc', 'jsd_between_point_cloud_sets']


def js_divercence_between_pc(pc1: torch.Tensor, pc2: torch.Tensor, voxels: int = 64) -> float:
    """JSD of the voxel histograms of two sets of clouds [S, N, 3] (reference :16-22), as numpy.float64"""
    return _js_divergence(PC.voxel_histogram(pc1, voxels), PC.voxel_histogram(pc2, voxels))


def _entropy(p):
    """base-2 entropy of a float64 vector that sums to one, 0 log 0 = 0"""
    nz = p[p > 0]
    return -np.sum(nz * np.log2(nz))


def _js_divergence(P, Q):
    """H2((P + Q) / 2) - (H2(P) + H2(Q)) / 2 of two count vectors after normalising each (reference :25-42).  Two ROCm
    tensors (int32 / float64) go to the kernel; two numpy arrays take a host float64 path, because the reference's
    function accepts arrays; of a mixed pair the numpy side is uploaded to the tensor's device."""
    on_dev = [isinstance(v, torch.Tensor) for v in (P, Q)]
    if any(on_dev):
        dev = (P if on_dev[0] else Q).device
        P, Q = [v if t else torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device=dev)
                for v, t in ((P, on_dev[0]), (Q, on_dev[1]))]
        return np.float64(PC.js_divergence(P, Q).item())
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        P_, Q_ = P / np.sum(P), Q / np.sum(Q)
    if np.isnan(P_).any() or np.isnan(Q_).any():
        return np.float64(np.nan)  # (a zero total: the reference's 0 / 0)
    return np.float64(_entropy((P_ + Q_) / 2.0) - (_entropy(P_) + _entropy(Q_)) / 2.0)


def _pc_to_voxel_distribution(pc: torch.Tensor, n_voxels: int = 64) -> np.ndarray:
    """int32 counts over the n_voxels^3 bins of the cube (reference :63-72), as a numpy array"""
    return PC.voxel_histogram(pc, n_voxels).cpu().numpy()


def jsd_between_point_cloud_sets(sample_pcs, ref_pcs, voxels=28, in_unit_sphere=True):
    """JSD of the occupancy-grid point counts of two sets of clouds [S1, N1, 3] and [S2, N2, 3] (reference :80-94):
    every point counts for its nearest cell centre of the voxels^3 grid, clipped to the sphere when in_unit_sphere.
    The counters stay on the device; the per-cloud counts are not needed here and are not taken."""
    return _js_divergence(*(PC.occupancy_grid(pcs, voxels, in_unit_sphere, want_bernoulli=False)[0]
                            for pcs in (sample_pcs, ref_pcs)))


def _entropy_of_occupancy_grid(pclouds, grid_resolution, in_sphere=False):
    """-> (mean over the cells of the entropy, in nats, of "does a cloud touch this cell": float, points per cell:
    float64 numpy array) for clouds [S, N, 3] on a grid_resolution^3 grid (reference :97-136)"""
    counters, bernoulli = PC.occupancy_grid(pclouds, grid_resolution, in_sphere)
    # the array is small: the entropy of the per-cell Bernoulli variables in float64 on the host
    p = bernoulli.cpu().numpy().astype(np.float64) / float(len(pclouds))
    acc = 0.0
    for v in (p, 1.0 - p):
        nz = v[(p > 0) & (v > 0)]
        acc -= float(np.sum(nz * np.log(nz)))
    return acc / len(p), counters.cpu().numpy().astype(np.float64)


def _unit_cube_grid_point_cloud(resolution, clip_sphere=False):
    """-> (cell centres, spacing): float32 [res, res, res, 3], or [G, 3] with the cells whose centre lies outside the
    radius-0.5 sphere left out when clip_sphere (reference :139-157); built by `sivae_hip.pointcloud.unit_cube_grid`"""
    axis, mask, spacing = PC.unit_cube_grid(resolution, clip_sphere)
    grid = PC.grid_cells(axis, mask)
    if not clip_sphere:
        grid = grid.reshape(resolution, resolution, resolution, 3)
    return grid, spacing
