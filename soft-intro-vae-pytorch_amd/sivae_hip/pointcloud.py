"""Point-cloud building blocks of the 3-D Soft-IntroVAE (reference: soft_intro_vae_3d/), on the kernels of
csrc/pointcloud.hip: tensor-level wrappers in the style of `ops` and the autograd Functions on top of them.

  chamfer_distance(preds [B, M, 3], gts [B, N, 3]) -> [B]       losses/chamfer_loss.py:11-17 (direct-form distances)
  emd_distance(preds [B, N, 3], gts [B, M, 3])     -> [B]       the loop's 'earth_mover' loss: emd_matrix's quantity with
                                                                 matchcostgrad's gradients (csrc/pc_emd.hip)
  relu_bn(a [B, C, N], weight, bias, BNState)      -> [B, C, N]  nn.ReLU -> nn.BatchNorm1d, relu(a) never stored
  max_points(y [B, C, N])                          -> [B, C]     y.max(dim=2)[0]
  relu_bn_max(a [B, C, N], weight, bias, BNState)  -> [B, C]     max_points(relu_bn(a)) in one piece: neither y nor the
                                                                 max's dense gradient is stored (RELU_BN_MAX: the encoder
                                                                 uses it for its last stage)
  pointwise_conv(x [B, Ci, N], w [Co, Ci, 1], bias, relu=False)  nn.Conv1d(kernel_size=1) on the ks = 1 conv kernels

and the validation metric (metrics/jsd.py) on the kernels of csrc/pc_jsd.hip, not differentiable:

  occupancy_grid(pcs [S, N, 3], resolution, in_sphere=False) -> (counters, bernoulli) int32 [G]
  voxel_histogram(pc [S, N, 3], n_voxels)                    -> counts int32 [n_voxels^3]
  js_divergence(P, Q)                                        -> 0-dim float64 tensor

and the set-to-set evaluation (metrics/evaluation_metrics.py: minimum matching distance, coverage) on the kernels of
csrc/pc_eval.hip, not differentiable:

  chamfer_matrix(sample [S, M, 3], ref [R, N, 3], normalize=True, use_sqrt=False) -> D [S, R], D[s, r] = CD(sample_s, ref_r)
  match_min(D [S, R])                                        -> (row_min [S], row_arg int32 [S], col_min [R], col_arg int32 [R])
  emd_matrix(sample [S, M, 3], ref [R, N, 3], normalize=True) -> D [S, R], D[s, r] = EMD(left = ref_r, right = sample_s)  (csrc/pc_emd.hip)
  chamfer_matrix_self(clouds [S, M, 3], normalize=True, use_sqrt=False) -> J [S, S] = chamfer_matrix(clouds, clouds), upper triangle computed, mirrored
  nn1_loo(Dss [S, S], Dsr [S, R], Drr [R, R])                -> (nn_val [S + R], nn_arg int32 [S + R]): 1-NN accuracy's leave-one-out neighbour

The pointwise convolutions and the MLPs run on what exists (`ops.conv2d_fwd` / `conv2d_wgrad` with ks = 1, `SF.linear`).
There is no CPU path: a CPU tensor raises the engine's usual message.
"""
import numpy as np
import torch

from . import functional as SF
from . import lib as _lib
from . import ops
from .ops import _p, _require, _s, timer_begin, timer_end, workspace

BN_EVAL_BWD_MSG = "sivae_hip: backward through eval-mode BatchNorm is not supported"  # (the image blocks' message)
# models/vae.py::Encoder sends its last ReLU -> BatchNorm1d -> max stage through relu_bn_max (same values, bit for bit)
RELU_BN_MAX = True


def _require_i32(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
            raise TypeError("sivae_hip: expected a contiguous int32 ROCm tensor")


def _require_f32(*tensors):
    _require(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise TypeError("sivae_hip: expected float32, got %s" % t.dtype)


# ------------------------------------------------------------------------------------------------ tensor level
def chamfer_fwd(preds, gts):
    """preds [B, M, 3], gts [B, N, 3] -> (loss [B], idx_p int32 [B, M] into gts, idx_g int32 [B, N] into preds)"""
    _require_f32(preds, gts)
    if preds.dim() != 3 or gts.dim() != 3 or preds.shape[2] != 3 or gts.shape[2] != 3 or preds.shape[0] != gts.shape[0]:
        raise ValueError("sivae_hip.chamfer: expected preds [B, M, 3] and gts [B, N, 3], got %s and %s"
                         % (tuple(preds.shape), tuple(gts.shape)))
    B, M, N = preds.shape[0], preds.shape[1], gts.shape[1]
    ws = workspace(_lib.load().sivae_chamfer_workspace_bytes(B, M, N), preds.device)
    idx_p = torch.empty((B, M), dtype=torch.int32, device=preds.device)
    idx_g = torch.empty((B, N), dtype=torch.int32, device=preds.device)
    loss = torch.empty(B, dtype=torch.float32, device=preds.device)
    t0 = timer_begin()
    _lib.call("sivae_chamfer_fwd", _p(preds), _p(gts), _p(idx_p), _p(idx_g), _p(loss), B, M, N, _p(ws), ws.numel(),
              _s(preds))
    if t0 is not None:
        timer_end(t0, "chamfer_fwd_kernel", 2.0 * 8 * B * M * N)
    return loss, idx_p, idx_g


def chamfer_bwd(g, preds, gts, idx_p, idx_g, want_dpreds=True, want_dgts=False):
    """-> (dpreds or None, dgts or None) from the upstream gradient g [B] and the forward's indices"""
    _require_f32(g, preds, gts)
    _require_i32(idx_p, idx_g)
    B, M, N = preds.shape[0], preds.shape[1], gts.shape[1]
    if g.numel() != B or tuple(idx_p.shape) != (B, M) or tuple(idx_g.shape) != (B, N):
        raise ValueError("sivae_hip.chamfer_bwd: g [B], idx_p [B, M], idx_g [B, N] expected")
    if not (want_dpreds or want_dgts):
        return None, None
    dp = torch.empty_like(preds) if want_dpreds else None
    dg = torch.empty_like(gts) if want_dgts else None
    t0 = timer_begin()
    _lib.call("sivae_chamfer_bwd", _p(g), _p(preds), _p(gts), _p(idx_p), _p(idx_g), _p(dp), _p(dg), B, M, N, _s(preds))
    if t0 is not None:
        timer_end(t0, "chamfer_bwd_kernel", 1.0 * B * M * N * (int(want_dpreds) + int(want_dgts)))
    return dp, dg


def _bcn(a):
    if a.dim() != 3:
        raise ValueError("sivae_hip: expected a [B, C, N] tensor, got %s" % (tuple(a.shape),))
    return a.shape


def relu_bn_stats(a, running_mean=None, running_var=None, num_batches_tracked=None, eps=1e-5, momentum=0.1):
    """per-channel (mean, invstd) of relu(a), a [B, C, N]; the running buffers get sivae_bn_stats' update"""
    _require_f32(a, running_mean, running_var)
    _require(num_batches_tracked)
    B, C, N = _bcn(a)
    ws = workspace(_lib.load().sivae_relu_bn_workspace_bytes(B, C, N), a.device)
    mean = torch.empty(C, dtype=torch.float32, device=a.device)
    invstd = torch.empty(C, dtype=torch.float32, device=a.device)
    t0 = timer_begin()
    _lib.call("sivae_relu_bn_stats", _p(a), B, C, N, float(eps), float(momentum), _p(running_mean), _p(running_var),
              _p(num_batches_tracked), _p(mean), _p(invstd), _p(ws), ws.numel(), _s(a))
    if t0 is not None:
        timer_end(t0, "relu_bn_reduce_kernel", 4.0 * a.numel())
    return mean, invstd


def relu_bn_apply(a, mean, invstd, gamma, beta):
    """y = gamma * (relu(a) - mean) * invstd + beta"""
    _require_f32(a, mean, invstd, gamma, beta)
    B, C, N = _bcn(a)
    y = torch.empty_like(a)
    t0 = timer_begin()
    _lib.call("sivae_relu_bn_apply", _p(a), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(y), B, C, N, _s(a))
    if t0 is not None:
        timer_end(t0, "relu_bn_apply_kernel", 3.0 * a.numel())
    return y


def relu_bn_bwd(dy, a, mean, invstd, gamma):
    """-> (da, dgamma, dbeta), relu(a) recomputed"""
    _require_f32(dy, a, mean, invstd, gamma)
    B, C, N = _bcn(a)
    if dy.shape != a.shape:
        raise ValueError("sivae_hip.relu_bn_bwd: dy and a differ in shape")
    ws = workspace(_lib.load().sivae_relu_bn_workspace_bytes(B, C, N), a.device)
    da = torch.empty_like(a)
    dgamma = torch.empty(C, dtype=torch.float32, device=a.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=a.device)
    t0 = timer_begin()
    _lib.call("sivae_relu_bn_bwd", _p(dy), _p(a), _p(mean), _p(invstd), _p(gamma), _p(da), _p(dgamma), _p(dbeta), B, C, N,
              _p(ws), ws.numel(), _s(a))
    if t0 is not None:
        timer_end(t0, "relu_bn_bwd", 12.0 * a.numel())
    return da, dgamma, dbeta


def max_points_fwd(x):
    """x [B, C, N] -> (values [B, C], int32 argmax [B, C], lowest index on a tie)"""
    _require_f32(x)
    B, C, N = _bcn(x)
    vals = torch.empty((B, C), dtype=torch.float32, device=x.device)
    arg = torch.empty((B, C), dtype=torch.int32, device=x.device)
    _lib.call("sivae_max_points_fwd", _p(x), _p(vals), _p(arg), B, C, N, _s(x))
    return vals, arg


def max_points_bwd(g, arg, N):
    """g [B, C] placed at arg in a zero [B, C, N] tensor"""
    _require_f32(g)
    _require_i32(arg)
    B, C = g.shape
    dx = torch.empty((B, C, N), dtype=torch.float32, device=g.device)
    _lib.call("sivae_max_points_bwd", _p(g), _p(arg), _p(dx), B, C, N, _s(g))
    return dx


def relu_bn_max_fwd(a, mean, invstd, gamma, beta):
    """max over the points of relu_bn_apply(a, ...) without storing it -> (values [B, C], int32 argmax [B, C]), bit-identical
    to max_points_fwd(relu_bn_apply(a, mean, invstd, gamma, beta))"""
    _require_f32(a, mean, invstd, gamma, beta)
    B, C, N = _bcn(a)
    vals = torch.empty((B, C), dtype=torch.float32, device=a.device)
    arg = torch.empty((B, C), dtype=torch.int32, device=a.device)
    t0 = timer_begin()
    _lib.call("sivae_relu_bn_max_fwd", _p(a), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(vals), _p(arg), B, C, N, _s(a))
    if t0 is not None:
        timer_end(t0, "relu_bn_max_fwd_kernel", 7.0 * a.numel())
    return vals, arg


def relu_bn_max_bwd(g, arg, a, mean, invstd, gamma):
    """-> (da, dgamma, dbeta) from the upstream gradient g [B, C] and the forward's arg: the max's gradient is g at arg and
    zero elsewhere, never stored"""
    _require_f32(g, a, mean, invstd, gamma)
    _require_i32(arg)
    B, C, N = _bcn(a)
    if tuple(g.shape) != (B, C) or tuple(arg.shape) != (B, C):
        raise ValueError("sivae_hip.relu_bn_max_bwd: g and arg [B, C] expected for a [B, C, N]")
    da = torch.empty_like(a)
    dgamma = torch.empty(C, dtype=torch.float32, device=a.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=a.device)
    t0 = timer_begin()
    _lib.call("sivae_relu_bn_max_bwd", _p(g), _p(arg), _p(a), _p(mean), _p(invstd), _p(gamma), _p(da), _p(dgamma), _p(dbeta),
              B, C, N, _s(a))
    if t0 is not None:
        timer_end(t0, "relu_bn_max_bwd", 8.0 * a.numel())
    return da, dgamma, dbeta


# ------------------------------------------------------------------------------------------------ the JSD metric
def unit_cube_grid(resolution, clip_sphere=False):
    """host float32 table of the reference's _unit_cube_grid_point_cloud (metrics/jsd.py:139-157)
    -> (axis [res], mask [res^3] bool in row-major (i, j, k) order, spacing): the centre of cell (i, j, k) is
    (axis[i], axis[j], axis[k]) with axis[i] = float32(i * spacing - 0.5); mask keeps a cell where the float32 norm of its
    centre is <= 0.5 (all of them without clipping)"""
    resolution = int(resolution)
    if resolution < 2:
        raise ValueError("sivae_hip.occupancy_grid: resolution must be at least 2, got %d" % resolution)
    spacing = 1.0 / float(resolution - 1)
    axis = (np.arange(resolution, dtype=np.float64) * spacing - 0.5).astype(np.float32)
    if clip_sphere:
        sq = axis * axis  # (numpy.linalg.norm over the last axis: sqrt of the float32 sum of squares, in axis order)
        nrm = np.sqrt((sq[:, None, None] + sq[None, :, None]) + sq[None, None, :])
        mask = (nrm <= np.float32(0.5)).reshape(-1)
    else:
        mask = np.ones(resolution ** 3, dtype=bool)
    return axis, mask, spacing


def grid_cells(axis, mask):
    """-> the table of centres [G, 3] float32 in the reference's order"""
    r = len(axis)
    full = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), axis=-1).reshape(r ** 3, 3)
    return np.ascontiguousarray(full[mask])


_grids = {}


def device_grid(device, resolution, in_sphere=False):
    """(cells [G, 3], lut int32 [res^3], axis [res]) on the device, cached per (device, resolution, in_sphere)"""
    key = (device.index, int(resolution), bool(in_sphere))
    g = _grids.get(key)
    if g is None:
        axis, mask, _ = unit_cube_grid(resolution, in_sphere)
        lut = np.full(mask.shape[0], -1, dtype=np.int32)
        lut[mask] = np.arange(int(mask.sum()), dtype=np.int32)
        g = tuple(torch.from_numpy(a).to(device) for a in (grid_cells(axis, mask), lut, axis))
        _grids[key] = g
    return g


def _require_clouds(pcs, who):
    """[S, N, 3] float32 on a ROCm device, ANY strides (read in place) -> (S, N, element strides)"""
    if not pcs.is_cuda:
        _require(pcs)  # (the engine's message)
    if pcs.dtype != torch.float32:
        raise TypeError("sivae_hip: expected float32, got %s" % pcs.dtype)
    if pcs.dim() != 3 or pcs.shape[2] != 3 or pcs.shape[0] == 0 or pcs.shape[1] == 0:
        raise ValueError("sivae_hip.%s: expected point clouds [S, N, 3], got %s" % (who, tuple(pcs.shape)))
    return pcs.shape[0], pcs.shape[1], pcs.stride()


def _both_require_clouds(sample, ref, who, max_points=None):
    """the checks of a set-to-set matrix, sample [S, M, 3] against ref [R, N, 3] -> (S, M, sample strides, R, N, ref strides)"""
    for pcs in (sample, ref):  # (the shape error before the device's, as relu_bn_max does)
        if pcs.dim() != 3 or pcs.shape[2] != 3:
            raise ValueError("sivae_hip.%s: expected point clouds [S, N, 3], got %s" % (who, tuple(pcs.shape)))
    S, M, sa = _require_clouds(sample, who)
    R, N, sb = _require_clouds(ref, who)
    if sample.device != ref.device:
        raise ValueError("sivae_hip.%s: sample is on %s, ref on %s" % (who, sample.device, ref.device))
    if max_points is not None and (M > max_points or N > max_points):
        raise ValueError("sivae_hip.%s: clouds of %d and %d points, at most %d are supported" % (who, M, N, max_points))
    if S * R >= 0x7fffffff:
        raise ValueError("sivae_hip.%s: %d x %d cloud pairs do not fit an int32 index" % (who, S, R))
    return S, M, sa, R, N, sb


def occupancy_grid(pcs, resolution, in_sphere=False, want_bernoulli=True, return_status=False):
    """_entropy_of_occupancy_grid's counting (metrics/jsd.py:113-126): -> (counters, bernoulli), int32 [G] each, over the
    resolution^3 cells (the ones inside the sphere when in_sphere); bernoulli is None when not wanted.  return_status:
    also the int32 [2] device word pair (non-finite points, points on the exhaustive route).  A non-finite coordinate
    raises ValueError (what sklearn's input check does in the reference)."""
    S, N, st = _require_clouds(pcs, "occupancy_grid")
    cells, lut, axis = device_grid(pcs.device, resolution, in_sphere)
    G = cells.shape[0]
    counters = torch.empty(G, dtype=torch.int32, device=pcs.device)
    bernoulli = torch.empty(G, dtype=torch.int32, device=pcs.device) if want_bernoulli else None
    status = torch.empty(2, dtype=torch.int32, device=pcs.device)
    t0 = timer_begin()
    _lib.call("sivae_occupancy_grid", _p(pcs), st[0], st[1], st[2], S, N, _p(cells), _p(lut), _p(axis), int(resolution), G,
              _p(counters), _p(bernoulli), _p(status), _s(pcs))
    t1 = ops.TIMER.begin() if t0 is not None else None  # (the end event, right behind the launch)
    bad, exhaustive = status.tolist()  # (one read; it synchronises, which a metric may)
    if t0 is not None:
        # 8 operations per distance of the exhaustive route, about 30 per point for the lookup route and the counting;
        # the record is appended here because the work is only known once the status words are back
        work = 8.0 * exhaustive * G + 30.0 * S * N
        ops.TIMER.records.append(("occupancy_grid_kernel", work, t0, t1, work))
    if bad:
        raise ValueError("sivae_hip.occupancy_grid: %d point(s) with a NaN or infinite coordinate" % bad)
    return (counters, bernoulli, status) if return_status else (counters, bernoulli)


def voxel_histogram(pc, n_voxels):
    """_pc_to_voxel_distribution (metrics/jsd.py:63-72) -> counts int32 [n_voxels^3]"""
    S, N, st = _require_clouds(pc, "voxel_histogram")
    n_voxels = int(n_voxels)
    if n_voxels < 1:
        raise ValueError("sivae_hip.voxel_histogram: n_voxels must be positive")
    counts = torch.empty(n_voxels ** 3, dtype=torch.int32, device=pc.device)
    status = torch.empty(1, dtype=torch.int32, device=pc.device)
    t0 = timer_begin()
    _lib.call("sivae_voxel_histogram", _p(pc), st[0], st[1], st[2], S, N, n_voxels, _p(counts), _p(status), _s(pc))
    if t0 is not None:
        timer_end(t0, "voxel_histogram_kernel", 9.0 * S * N)
    bad = int(status[0])
    if bad:
        raise ValueError("sivae_hip.voxel_histogram: %d point(s) with a NaN coordinate" % bad)
    return counts


def js_divergence(P, Q):
    """_js_divergence (metrics/jsd.py:25-42) of two count vectors (int32 or float64, equal length) -> 0-dim float64"""
    for t in (P, Q):
        if not t.is_cuda:
            _require(t)
        if t.dtype not in (torch.int32, torch.float64) or not t.is_contiguous():
            raise TypeError("sivae_hip.js_divergence: expected contiguous int32 or float64 counts, got %s" % t.dtype)
    if P.device != Q.device:
        raise ValueError("sivae_hip.js_divergence: P is on %s, Q on %s" % (P.device, Q.device))
    if P.dim() != 1 or P.shape != Q.shape or P.numel() == 0:
        raise ValueError("sivae_hip.js_divergence: two vectors of equal length expected, got %s and %s"
                         % (tuple(P.shape), tuple(Q.shape)))
    out = torch.empty((), dtype=torch.float64, device=P.device)
    t0 = timer_begin()
    _lib.call("sivae_js_divergence", _p(P), _p(Q), int(P.dtype == torch.float64), int(Q.dtype == torch.float64), P.numel(),
              _p(out), _s(P))
    if t0 is not None:
        timer_end(t0, "js_divergence_kernel", 12.0 * P.numel())
    return out


# ------------------------------------------------------------------------------------------------ MMD-CD / COV-CD
# Point pairs (rows x R x M x N) one launch of chamfer_matrix may cover: the rows of D are walked in slabs of at least one
# row so that a launch stays short on a device other work shares.
# Measured on an MI355X (tools/bench_pc_eval.py, profiles/pc_eval_bench.txt): 2400 x 800 clouds of 2048 points are 60
# launches of 40 rows, the longest 21.6 ms (the first), the others 18.6 - 19.0 ms.
MATRIX_POINT_PAIRS_PER_LAUNCH = 1 << 37


def chamfer_matrix(sample, ref, normalize=True, use_sqrt=False):
    """All-pairs Chamfer distance of two sets of clouds, sample [S, M, 3] and ref [R, N, 3] (float32, any strides: the
    `transpose(1, 2)` view of a [S, 3, M] decoder output is read in place) -> D [S, R] float32 with
    D[s, r] = sum_j f(min_i |P_j - Q_i|^2) / m + sum_i f(min_j |P_j - Q_i|^2) / n, f = sqrt when use_sqrt, m = M and n = N
    when normalize (1 otherwise).  A cloud with a non-finite coordinate makes its row / column of D non-finite."""
    S, M, sa, R, N, sb = _both_require_clouds(sample, ref, "chamfer_matrix")
    D = torch.empty((S, R), dtype=torch.float32, device=sample.device)
    slab = max(1, min(S, MATRIX_POINT_PAIRS_PER_LAUNCH // (R * M * N)))
    ws = workspace(_lib.load().sivae_chamfer_matrix_workspace_bytes(slab, R, M, N), sample.device)
    for s0 in range(0, S, slab):
        s1 = min(S, s0 + slab)
        t0 = timer_begin()
        _lib.call("sivae_chamfer_matrix", _p(sample), sa[0], sa[1], sa[2], _p(ref), sb[0], sb[1], sb[2], _p(D), S, R, M, N,
                  s0, s1, int(bool(normalize)), int(bool(use_sqrt)), _p(ws), ws.numel(), _s(sample))
        if t0 is not None:
            # per point pair: 3 subtractions, a multiply and 2 FMAs, the row minimum and a share of the column minimum
            timer_end(t0, "chamfer_matrix_kernel", 8.0 * (s1 - s0) * R * M * N)
    return D


def match_min(D):
    """D [S, R] float32 -> (row_min [S], row_arg int32 [S], col_min [R], col_arg int32 [R]); the lowest index wins a tie,
    +inf / NaN entries never win, a row or column of nothing else gives (+inf, 0)"""
    if D.dim() != 2 or D.shape[0] == 0 or D.shape[1] == 0:
        raise ValueError("sivae_hip.match_min: expected a matrix [S, R], got %s" % (tuple(D.shape),))
    _require_f32(D)
    S, R = D.shape
    row_min = torch.empty(S, dtype=torch.float32, device=D.device)
    row_arg = torch.empty(S, dtype=torch.int32, device=D.device)
    col_min = torch.empty(R, dtype=torch.float32, device=D.device)
    col_arg = torch.empty(R, dtype=torch.int32, device=D.device)
    t0 = timer_begin()
    _lib.call("sivae_match_min", _p(D), S, R, _p(row_min), _p(row_arg), _p(col_min), _p(col_arg), _s(D))
    if t0 is not None:
        timer_end(t0, "match_min_kernel", 4.0 * S * R)
    return row_min, row_arg, col_min, col_arg


# ------------------------------------------------------------------------------------------------ 1-NN accuracy
def chamfer_matrix_self(clouds, normalize=True, use_sqrt=False):
    """The Chamfer matrix of ONE set against itself, clouds [S, M, 3] (float32, any strides) -> J [S, S] float32: the upper
    triangle with the diagonal is bit for bit that of chamfer_matrix(clouds, clouds) (the diagonal exactly 0 for finite
    clouds), J[j, i] is a copy of J[i, j].  Only the S (S + 1) / 2 pairs i <= j are computed, walked by folded rows (row f
    of the triangle followed by row S - 1 - f: S + 1 pairs each) in slabs of MATRIX_POINT_PAIRS_PER_LAUNCH point pairs.  A
    cloud with a non-finite coordinate makes its row and column non-finite."""
    if clouds.dim() != 3 or clouds.shape[2] != 3:  # (the shape error before the device's, as chamfer_matrix does)
        raise ValueError("sivae_hip.chamfer_matrix_self: expected point clouds [S, N, 3], got %s" % (tuple(clouds.shape),))
    S, M, st = _require_clouds(clouds, "chamfer_matrix_self")
    if S * S >= 0x7fffffff:
        raise ValueError("sivae_hip.chamfer_matrix_self: %d x %d cloud pairs do not fit an int32 index" % (S, S))
    J = torch.empty((S, S), dtype=torch.float32, device=clouds.device)
    folded = (S + 1) // 2
    slab = max(1, min(folded, MATRIX_POINT_PAIRS_PER_LAUNCH // ((S + 1) * M * M)))
    ws = workspace(_lib.load().sivae_chamfer_matrix_self_workspace_bytes(slab, S, M), clouds.device)
    for f0 in range(0, folded, slab):
        f1 = min(folded, f0 + slab)
        t0 = timer_begin()
        _lib.call("sivae_chamfer_matrix_self", _p(clouds), st[0], st[1], st[2], _p(J), S, M, f0, f1, int(bool(normalize)),
                  int(bool(use_sqrt)), _p(ws), ws.numel(), _s(clouds))
        if t0 is not None:
            # 8 per point pair computed, as chamfer_matrix counts; the middle folded row f of an odd S has S - f pairs
            pairs = (f1 - f0) * (S + 1) - (f1 if S % 2 and f1 == folded else 0)
            timer_end(t0, "chamfer_matrix_self_kernel", 8.0 * pairs * M * M)
    return J


def nn1_loo(Dss, Dsr, Drr):
    """The joint leave-one-out nearest neighbour behind 1-NN accuracy: Dss [S, S], Dsr [S, R], Drr [R, R] (float32,
    contiguous) -> (nn_val float32 [S + R], nn_arg int32 [S + R]).  Items 0 .. S - 1 are the samples, S .. S + R - 1 the
    references; item t's distances are row t of [[Dss, Dsr], [Dsr^T, Drr]] without the entry t itself.  The lowest index
    wins a tie, +inf / NaN entries never win, an item with no candidate left gives (+inf, -1)."""
    for name, D in (("Dss", Dss), ("Dsr", Dsr), ("Drr", Drr)):
        if D.dim() != 2 or D.shape[0] == 0 or D.shape[1] == 0:
            raise ValueError("sivae_hip.nn1_loo: %s: expected a matrix, got %s" % (name, tuple(D.shape)))
    S, R = Dsr.shape
    if tuple(Dss.shape) != (S, S) or tuple(Drr.shape) != (R, R):
        raise ValueError("sivae_hip.nn1_loo: expected Dss [S, S], Dsr [S, R], Drr [R, R], got %s, %s, %s"
                         % (tuple(Dss.shape), tuple(Dsr.shape), tuple(Drr.shape)))
    _require_f32(Dss, Dsr, Drr)
    if Dss.device != Dsr.device or Drr.device != Dsr.device:
        raise ValueError("sivae_hip.nn1_loo: the matrices are on %s, %s and %s" % (Dss.device, Dsr.device, Drr.device))
    T = S + R
    if T * T >= 0x7fffffff:
        raise ValueError("sivae_hip.nn1_loo: %d x %d item pairs do not fit an int32 index" % (T, T))
    nn_val = torch.empty(T, dtype=torch.float32, device=Dsr.device)
    nn_arg = torch.empty(T, dtype=torch.int32, device=Dsr.device)
    t0 = timer_begin()
    _lib.call("sivae_nn1_loo", _p(Dss), _p(Dsr), _p(Drr), S, R, _p(nn_val), _p(nn_arg), _s(Dsr))
    if t0 is not None:
        timer_end(t0, "nn1_loo_kernel", 2.0 * T * T)
    return nn_val, nn_arg


# ------------------------------------------------------------------------------------------------ MMD-EMD / COV-EMD
EMD_MAX_POINTS = 4096  # (both clouds of a pair are held in LDS)
# Point pairs (cloud pairs x M x N) one launch of emd_matrix may cover, as MATRIX_POINT_PAIRS_PER_LAUNCH above; a point pair
# is visited in thirty sweeps with an exponential each, against once for the Chamfer matrix.  A row of D longer than that
# goes in blocks of columns.  2^31 is 512 cloud pairs of 2048 points: one block per pair, two resident blocks on each of
# the 256 compute units, so a launch is one round of them.
# Measured on an MI355X (tools/bench_pc_emd.py, profiles/pc_emd_bench.txt), clouds of 2048 points: launches of
# 512 cloud pairs take 14.1 - 14.3 ms (64 x 64 clouds, 40 launches); 2400 x 800 clouds are 4800 launches of 512 and 288
# pairs, the longest 16.1 ms, the median 15.0 ms.  One whole row of 800 pairs in a launch took 28.9 ms.
EMD_POINT_PAIRS_PER_LAUNCH = 1 << 31


def emd_matrix(sample, ref, normalize=True):
    """All-pairs approximate-matching earth mover's distance (Fan, Su, Guibas; include/sivae_hip.h states the ten levels)
    of two sets of clouds, sample [S, M, 3] and ref [R, N, 3] (float32, any strides, at most 4096 points a cloud)
    -> D [S, R] float32 with D[s, r] = EMD(left = ref_r, right = sample_s): the cost of the matching, divided by
    max(M, N) when normalize.  Not symmetric in its arguments.  A cloud with a non-finite coordinate makes its row /
    column of D NaN."""
    S, M, sa, R, N, sb = _both_require_clouds(sample, ref, "emd_matrix", max_points=EMD_MAX_POINTS)
    D = torch.empty((S, R), dtype=torch.float32, device=sample.device)
    pairs = max(1, EMD_POINT_PAIRS_PER_LAUNCH // (M * N))    # cloud pairs one launch may cover:
    rows, cols = max(1, min(S, pairs // R)), min(R, pairs)   # a slab of whole rows, or ONE row in blocks of columns
    ws = workspace(_lib.load().sivae_emd_matrix_workspace_bytes(rows, cols, M, N), sample.device)
    for s0 in range(0, S, rows):
        s1 = min(S, s0 + rows)
        for r0 in range(0, R, cols):
            r1 = min(R, r0 + cols)
            # D[s0:s1, r0:r1] (whole rows, or a stretch of one) is contiguous: to the library it is the whole matrix of
            # sample[s0:s1] against ref[r0:r1]; an entry does not depend on which launch computes it
            t0 = timer_begin()
            _lib.call("sivae_emd_matrix", _p(sample[s0:s1]), sa[0], sa[1], sa[2], _p(ref[r0:r1]), sb[0], sb[1], sb[2],
                      _p(D[s0:s1, r0:r1]), s1 - s0, r1 - r0, M, N, 0, s1 - s0, int(bool(normalize)), _p(ws), ws.numel(),
                      _s(sample))
            if t0 is not None:
                # per point pair and sweep: the distance (6), its scaling, the exponential and the sum (9); the third
                # sweep of a level adds the root and the cost (12)
                timer_end(t0, "emd_matrix_kernel", 300.0 * (s1 - s0) * (r1 - r0) * M * N)
    return D


# ------------------------------------------------------------------------------------------------ the earth mover's loss
# Point pairs (cloud pairs x N x M) one launch of emd_loss_fwd may cover.  The loss kernel takes up to 256 registers a
# lane, so ONE block is resident on a compute unit: 2^30 is 256 cloud pairs of 2048 points, one round of resident blocks on
# the 256 compute units.  A training batch (32 - 64 pairs) is one launch.
# Measured on an MI355X (tools/bench_pc_emd.py --step loss, profiles/pc_emd_loss_bench.txt), 32 pairs of 2048 points:
# one launch, 7.72 ms for the cost alone, 11.55 ms with dright, 14.34 ms with both gradients; 256 pairs, one on every
# compute unit, both gradients: 14.47 ms at the longest (chamfer_matrix's launches take 19 - 22 ms).
EMD_LOSS_POINT_PAIRS_PER_LAUNCH = 1 << 30


def emd_loss_fwd(left, right, want_dleft, want_dright, normalize=False):
    """left [B, N, 3], right [B, M, 3] (float32, any strides, at most 4096 points a cloud) -> (cost [B], dleft [B, N, 3] or
    None, dright [B, M, 3] or None): cost[b] = EMD(left = left_b, right = right_b), the quantity of emd_matrix (bit for bit
    emd_matrix(right[b:b+1], left[b:b+1])[0, 0]), and matchcostgrad's gradients of it, the plan held constant
    (include/sivae_hip.h).  Only the gradients asked for are computed.  A pair with a non-finite coordinate gets a NaN
    cost and NaN gradient slices; no other pair changes."""
    for pcs in (left, right):  # (the shape error before the device's, as emd_matrix does)
        if pcs.dim() != 3 or pcs.shape[2] != 3:
            raise ValueError("sivae_hip.emd_loss: expected point clouds [B, N, 3], got %s" % (tuple(pcs.shape),))
    B, N, sl = _require_clouds(left, "emd_loss")
    Br, M, sr = _require_clouds(right, "emd_loss")
    if B != Br:
        raise ValueError("sivae_hip.emd_loss: %d left clouds against %d right clouds" % (B, Br))
    if left.device != right.device:
        raise ValueError("sivae_hip.emd_loss: left is on %s, right on %s" % (left.device, right.device))
    if N > EMD_MAX_POINTS or M > EMD_MAX_POINTS:
        raise ValueError("sivae_hip.emd_loss: clouds of %d and %d points, at most %d are supported" % (N, M, EMD_MAX_POINTS))
    if 3 * B * max(N, M) >= 0x7fffffff:
        raise ValueError("sivae_hip.emd_loss: %d clouds of %d points do not fit an int32 index" % (B, max(N, M)))
    cost = torch.empty(B, dtype=torch.float32, device=left.device)
    dleft = torch.empty((B, N, 3), dtype=torch.float32, device=left.device) if want_dleft else None
    dright = torch.empty((B, M, 3), dtype=torch.float32, device=left.device) if want_dright else None
    slab = max(1, min(B, EMD_LOSS_POINT_PAIRS_PER_LAUNCH // (N * M)))
    ws = workspace(_lib.load().sivae_emd_loss_workspace_bytes(slab, N, M), left.device)
    for b0 in range(0, B, slab):
        b1 = min(B, b0 + slab)
        # a pair's results do not depend on which launch computes them: to the library a slab is a batch of its own
        t0 = timer_begin()
        _lib.call("sivae_emd_loss", _p(left[b0:b1]), sl[0], sl[1], sl[2], _p(right[b0:b1]), sr[0], sr[1], sr[2],
                  _p(cost[b0:b1]), _p(dleft[b0:b1]) if want_dleft else None, _p(dright[b0:b1]) if want_dright else None,
                  b1 - b0, N, M, int(bool(normalize)), _p(ws), ws.numel(), _s(left))
        if t0 is not None:
            # per point pair: the thirty sweeps of emd_matrix (300), the left gradient on the third sweep of a level (7 a
            # level), the right gradient's fourth sweep (24 a level)
            timer_end(t0, "emd_loss_kernel", (300.0 + 70.0 * bool(want_dleft) + 240.0 * bool(want_dright)) * (b1 - b0) * N * M)
    return cost, dleft, dright


# ------------------------------------------------------------------------------------------------ autograd
class ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, gts):
        # (the training loop passes x.permute(0, 2, 1) + 0.5: not contiguous)
        preds, gts = preds.contiguous(), gts.contiguous()
        loss, idx_p, idx_g = chamfer_fwd(preds, gts)
        ctx.save_for_backward(preds, gts, idx_p, idx_g)
        ctx.mark_non_differentiable(idx_p, idx_g)
        return loss, idx_p, idx_g

    @staticmethod
    def backward(ctx, g, _gp, _gg):
        preds, gts, idx_p, idx_g = ctx.saved_tensors
        need = ctx.needs_input_grad
        return chamfer_bwd(g.contiguous(), preds, gts, idx_p, idx_g, need[0], need[1])


class EmdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, preds, gts, normalize):
        need = ctx.needs_input_grad
        # (any strides are read in place: the training loop passes x.permute(0, 2, 1) + 0.5 and the decoder's view)
        cost, dpreds, dgts = emd_loss_fwd(preds, gts, need[0], need[1], normalize)
        ctx.save_for_backward(dpreds, dgts)
        return cost

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dpreds, dgts = ctx.saved_tensors
        g = g.contiguous()
        _require_f32(g)
        g = g.view(-1, 1, 1)
        return (None if dpreds is None else g * dpreds), (None if dgts is None else g * dgts), None


def emd_distance(preds, gts, normalize=False):
    """per-cloud approximate-matching earth mover's distance [B] of preds [B, N, 3] (the matching's left side) and gts
    [B, M, 3] (its right side), the original's EMD()(preds, gts): emd_loss_fwd's cost, differentiable in both arguments
    with matchcostgrad's gradients (the plan held constant), divided by max(N, M) when normalize.  The forward computes the
    gradients the inputs need and the backward scales them by the upstream g[b]: a second derivative raises.
    torch.autograd.gradcheck does NOT apply: the plan moves with the points, so finite differences of the cost are not the
    gradient returned here."""
    return EmdFn.apply(preds, gts, bool(normalize))


def chamfer_distance(preds, gts, return_indices=False):
    """per-cloud Chamfer distance [B] (differentiable in both arguments); return_indices: also the nearest-neighbour
    indices (idx_p [B, M] into gts, idx_g [B, N] into preds)"""
    loss, idx_p, idx_g = ChamferFn.apply(preds, gts)
    return (loss, idx_p, idx_g) if return_indices else loss


def _bn_mean_invstd(a, st):
    """-> (mean, invstd): the batch's in training (the running buffers get their update), else the running buffers'"""
    if st.training:
        return relu_bn_stats(a, st.running_mean, st.running_var, st.num_batches_tracked, st.eps,
                             st.momentum if st.momentum is not None else 0.1)
    return st.running_mean, torch.rsqrt(st.running_var + st.eps)


class ReluBnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, weight, bias, st):
        a = a.contiguous()
        mean, invstd = _bn_mean_invstd(a, st)
        ctx.training = st.training
        ctx.save_for_backward(a, mean, invstd, weight)
        return relu_bn_apply(a, mean, invstd, weight.detach(), bias.detach())

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise RuntimeError(BN_EVAL_BWD_MSG)
        a, mean, invstd, weight = ctx.saved_tensors
        da, dgamma, dbeta = relu_bn_bwd(dy.contiguous(), a, mean, invstd, weight.detach())
        return da, dgamma, dbeta, None


def relu_bn(a, weight, bias, st):
    """BatchNorm1d(ReLU(a)) for a [B, C, N]; st: the BatchNorm module's `functional.BNState` (buffers + mode)"""
    return ReluBnFn.apply(a, weight, bias, st)


class MaxPointsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y):
        y = y.contiguous()
        vals, arg = max_points_fwd(y)
        ctx.save_for_backward(arg)
        ctx.N = y.shape[2]
        return vals

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        return max_points_bwd(g.contiguous(), arg, ctx.N)


def max_points(y):
    return MaxPointsFn.apply(y)


class ReluBnMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, weight, bias, st):
        a = a.contiguous()
        mean, invstd = _bn_mean_invstd(a, st)
        vals, arg = relu_bn_max_fwd(a, mean, invstd, weight.detach(), bias.detach())
        ctx.training = st.training
        ctx.save_for_backward(a, mean, invstd, weight, arg)
        return vals

    @staticmethod
    def backward(ctx, g):
        if not ctx.training:
            raise RuntimeError(BN_EVAL_BWD_MSG)
        a, mean, invstd, weight, arg = ctx.saved_tensors
        da, dgamma, dbeta = relu_bn_max_bwd(g.contiguous(), arg, a, mean, invstd, weight.detach())
        return da, dgamma, dbeta, None


def relu_bn_max(a, weight, bias, st):
    """max_points(relu_bn(a, weight, bias, st)) -> [B, C], the same values and buffer updates, in two tensor passes forward
    and two backward"""
    _bcn(a)  # (the shape error before anything else: a 2-D input would otherwise reach the statistics first)
    return ReluBnMaxFn.apply(a, weight, bias, st)


def _pack1(w, mode):
    """GEMM operand of a Conv1d(kernel_size=1) weight [Co, Ci, 1] through its 4-D view, cached ON the parameter under
    functional's tag (version counter, storage): an in-place step of a stock torch.optim optimizer invalidates it"""
    Co, Ci = w.shape[0], w.shape[1]
    return SF._cached_pack(w, ("conv1d", mode), lambda: ops.PackedW(w.detach().view(Co, Ci, 1, 1), mode))


class PointwiseConvFn(torch.autograd.Function):
    """nn.Conv1d(Ci, Co, kernel_size=1) (+ ReLU) over [B, Ci, N] as the ks = 1 convolution over [B, Ci, 1, N]"""

    @staticmethod
    def forward(ctx, x, w, bias, relu):
        x = x.contiguous()
        B, Ci, N = x.shape
        Co = w.shape[0]
        if w.dim() != 3 or w.shape[1] != Ci or w.shape[2] != 1:
            raise RuntimeError("sivae_hip: pointwise conv expects a [Co, %d, 1] weight, got %s" % (Ci, tuple(w.shape)))
        b_ = None if bias is None else bias.detach()
        y = ops.conv2d_fwd(x.view(B, Ci, 1, N), _pack1(w, 0), Co, 1, bias=b_).view(B, Co, N)
        if relu:
            ops.relu_fwd(y, inplace=True)
        ctx.relu = relu
        ctx.save_for_backward(x, w, y if relu else None, bias)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        dy = dy.contiguous()
        if ctx.relu:
            dy = ops.relu_bwd(dy, y)
        B, Ci, N = x.shape
        Co = w.shape[0]
        dy4 = dy.view(B, Co, 1, N)
        dw = ops.conv2d_wgrad(x.view(B, Ci, 1, N), dy4, 1).view(Co, Ci, 1) if need[1] else None
        db = ops.channel_sum(dy4) if (bias is not None and need[2]) else None
        dx = ops.conv2d_fwd(dy4, _pack1(w, 1), Ci, 1).view(B, Ci, N) if need[0] else None
        return dx, dw, db, None


def pointwise_conv(x, w, bias=None, relu=False):
    return PointwiseConvFn.apply(x, w, bias, relu)
