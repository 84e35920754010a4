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

__all__ = ['chamfer_matrix', 'emd_matrix', 'minimum_mathing_distance', 'minimum_matching_distance', 'coverage',
           'chamfer_matrix_self', 'one_nn_accuracy']


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


def chamfer_matrix_self(pcs, normalize=True, use_sqrt=False):
    """J [S, S] float32 on the device, the Chamfer matrix of one set against itself: chamfer_matrix(pcs, pcs) at half the
    work (the pairs i <= j are computed, bit for bit its entries, and mirrored)"""
    if np.ndim(pcs) != 3 or np.shape(pcs)[2] != 3:  # (the shape error before any device is asked for)
        raise ValueError("pcs: expected point clouds [S, N, 3], got %s" % (tuple(np.shape(pcs)),))
    return PC.chamfer_matrix_self(_clouds(pcs, _device_of(pcs), "pcs"), normalize, use_sqrt)


def _given_matrix(dist, name, device_of):
    """a caller's matrix -> float32, contiguous, on the device (`device_of()` names it when `dist` is host data)"""
    if not isinstance(dist, torch.Tensor):
        dist = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float32))
    if dist.dim() != 2:
        raise ValueError("%s: expected a matrix [S, R], got %s" % (name, tuple(dist.shape)))
    if not dist.is_cuda:
        dist = dist.to(device_of())
    return dist.float().contiguous()


def _finite(dist):
    if not bool(torch.isfinite(dist).all()):
        raise ValueError("the distance matrix has %d non-finite entries (a cloud with a NaN or infinite coordinate?)"
                         % int((~torch.isfinite(dist)).sum()))
    return dist


def _matrix(sample_pcs, ref_pcs, normalize, use_sqrt, use_EMD, dist):
    if use_EMD:
        raise NotImplementedError("use_EMD is not wired to the earth mover's matrix: pass dist=emd_matrix(sample_pcs, "
                                  "ref_pcs) for MMD-EMD / COV-EMD")
    if dist is None:
        dist = chamfer_matrix(sample_pcs, ref_pcs, normalize, use_sqrt)
    else:
        dist = _given_matrix(dist, "dist", lambda: _device_of(sample_pcs, ref_pcs))
    return _finite(dist)


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


def one_nn_accuracy(sample_pcs, ref_pcs, normalize=True, use_sqrt=False, metric="cd", dist=None, dist_ss=None,
                    dist_rr=None):
    """1-nearest-neighbour accuracy (1-NNA): every cloud of the union of the two sets is assigned the set of its nearest
    OTHER cloud; the score is the fraction assigned to their own set (0.5: the sets cannot be told apart, 1.0: trivially
    separable).  -> dict(acc, acc_sample, acc_ref: floats; nn: int64 numpy [S + R], the neighbour's joint index (samples
    0 .. S - 1, references S .. S + R - 1, the lowest on a tie); nn_dist: float32 numpy [S + R]).
    metric "cd": Chamfer matrices (`chamfer_matrix_self` for each set, `chamfer_matrix` across); "emd": `emd_matrix` for all
    three (whole matrices: the approximate matching is not symmetric; item t reads ITS row).  `dist` [S, R] is the matrix
    `minimum_mathing_distance` and `coverage` take, `dist_ss` [S, S] and `dist_rr` [R, R] the same-set ones; the flags of
    a given matrix are its own."""
    if metric not in ("cd", "emd"):
        raise ValueError("metric: expected 'cd' or 'emd', got %r" % (metric,))

    def device():
        return _device_of(sample_pcs, ref_pcs, dist, dist_ss, dist_rr)

    need = [("sample_pcs", sample_pcs, dist is None or dist_ss is None), ("ref_pcs", ref_pcs, dist is None or dist_rr is None)]
    for name, pcs, needed in need:  # (the shape error before any device is asked for)
        if needed and (np.ndim(pcs) != 3 or np.shape(pcs)[2] != 3):
            raise ValueError("%s: expected point clouds [S, N, 3], got %s" % (name, tuple(np.shape(pcs))))
    # (host clouds are uploaded once, not once per matrix)
    sample_pcs, ref_pcs = (_clouds(pcs, device(), name) if needed else pcs for name, pcs, needed in need)

    def build(name):
        if name == "dist":
            return (emd_matrix(sample_pcs, ref_pcs, normalize) if metric == "emd"
                    else chamfer_matrix(sample_pcs, ref_pcs, normalize, use_sqrt))
        pcs = sample_pcs if name == "dist_ss" else ref_pcs
        return emd_matrix(pcs, pcs, normalize) if metric == "emd" else chamfer_matrix_self(pcs, normalize, use_sqrt)

    Dss, Dsr, Drr = (_finite(build(name) if given is None else _given_matrix(given, name, device))
                     for name, given in (("dist_ss", dist_ss), ("dist", dist), ("dist_rr", dist_rr)))
    S, R = Dsr.shape
    if tuple(Dss.shape) != (S, S) or tuple(Drr.shape) != (R, R):
        raise ValueError("expected dist_ss [S, S], dist [S, R] and dist_rr [R, R], got %s, %s and %s"
                         % (tuple(Dss.shape), tuple(Dsr.shape), tuple(Drr.shape)))
    nn_val, nn_arg = PC.nn1_loo(Dss, Dsr, Drr)
    nn = nn_arg.cpu().numpy().astype(np.int64)
    own = (nn < S) == (np.arange(S + R) < S)
    return dict(acc=float(np.mean(own, dtype=np.float64)), acc_sample=float(np.mean(own[:S], dtype=np.float64)),
                acc_ref=float(np.mean(own[S:], dtype=np.float64)), nn=nn, nn_dist=nn_val.cpu().numpy())
