"""numpy float64 restatement of the 3-D variant's validation metric (reference: soft_intro_vae_3d/metrics/jsd.py), written
from the maths, without scipy or scikit-learn:

  grid               centres float32(i * (1 / (res - 1)) - 0.5) per axis, row-major over (i, j, k); clipping keeps a cell
                     where the float32 norm of its centre is <= 0.5
  occupancy          every point adds 1 to the counter of its nearest centre (brute force over the table, float64, in
                     chunks), every cloud adds 1 to `bernoulli` for each distinct cell it touched
  bernoulli_entropy  mean over the cells of the entropy (nats) of Bernoulli(bernoulli / S)
  js_divergence      H2((P + Q) / 2) - (H2(P) + H2(Q)) / 2 of the normalised count vectors, 0 log 0 = 0
  voxel_distribution int((clamp(x, -0.5, 0.4999) + 0.5) * n) per coordinate in float32 operations, linear index

`occupancy` also returns, per point, the relative gap (d2 - d1) / d2 between its nearest and second-nearest centre in
float64: a float32 kernel can only be asked for the same cell where that gap is far above float32's rounding error.
"""
import numpy as np

GAP = 2.0 ** -16  # 64 x the relative error 4 * 2^-24 of a direct-form float32 squared distance


def grid(resolution, clip_sphere=False):
    """-> (cells float32 [G, 3], mask bool [res^3], spacing)"""
    spacing = 1.0 / float(resolution - 1)
    axis = np.array([i * spacing - 0.5 for i in range(resolution)], dtype=np.float32)
    full = np.empty((resolution, resolution, resolution, 3), dtype=np.float32)
    full[..., 0] = axis[:, None, None]
    full[..., 1] = axis[None, :, None]
    full[..., 2] = axis[None, None, :]
    full = full.reshape(-1, 3)
    if clip_sphere:
        mask = np.sqrt(np.sum(full * full, axis=1, dtype=np.float32)) <= np.float32(0.5)
    else:
        mask = np.ones(len(full), dtype=bool)
    return full[mask], mask, spacing


def nearest(points, cells, chunk=256):
    """points [M, 3], cells [G, 3] -> (index of the nearest centre [M] (lowest on a tie), relative gap [M]) in float64"""
    p, c = np.asarray(points, dtype=np.float64), np.asarray(cells, dtype=np.float64)
    idx = np.empty(len(p), dtype=np.int64)
    gap = np.ones(len(p), dtype=np.float64)
    rows = np.arange(chunk)
    for m0 in range(0, len(p), chunk):
        q = p[m0:m0 + chunk]
        d = (q[:, None, 0] - c[None, :, 0]) ** 2
        d += (q[:, None, 1] - c[None, :, 1]) ** 2
        d += (q[:, None, 2] - c[None, :, 2]) ** 2
        i = d.argmin(axis=1)
        r = rows[:len(q)]
        d1 = d[r, i].copy()
        idx[m0:m0 + chunk] = i
        if len(c) > 1:
            d[r, i] = np.inf
            d2 = d.min(axis=1)
            gap[m0:m0 + chunk] = (d2 - d1) / d2
    return idx, gap


def occupancy(pcs, cells):
    """pcs [S, N, 3] -> (counters int64 [G], bernoulli int64 [G], gap [S, N])"""
    pcs = np.asarray(pcs)
    S, N = pcs.shape[:2]
    idx, gap = nearest(pcs.reshape(S * N, 3), cells)
    counters = np.zeros(len(cells), dtype=np.int64)
    np.add.at(counters, idx, 1)
    bernoulli = np.zeros(len(cells), dtype=np.int64)
    for s in range(S):
        np.add.at(bernoulli, np.unique(idx[s * N:(s + 1) * N]), 1)
    return counters, bernoulli, gap.reshape(S, N)


def bernoulli_entropy(bernoulli, n_clouds):
    p = np.asarray(bernoulli, dtype=np.float64) / float(n_clouds)
    acc = 0.0
    for g in p[p > 0]:
        for v in (g, 1.0 - g):
            if v > 0:
                acc -= v * np.log(v)
    return acc / len(p)


def entropy2(p):
    nz = p[p > 0]
    return float(-np.sum(nz * np.log2(nz)))


def js_divergence(P, Q):
    P, Q = np.asarray(P, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    P_, Q_ = P / P.sum(), Q / Q.sum()
    return entropy2((P_ + Q_) / 2.0) - (entropy2(P_) + entropy2(Q_)) / 2.0


def voxel_distribution(pc, n):
    """pc float32 [S, N, 3] -> int32 [n^3]"""
    pc = np.asarray(pc, dtype=np.float32)
    v = np.clip(pc, np.float32(-0.5), np.float32(0.4999)) + np.float32(0.5)
    v = (v * np.float32(n)).astype(np.int32).astype(np.int64)
    lin = (v[..., 0] * n * n + v[..., 1] * n + v[..., 2]).reshape(-1)
    out = np.zeros(n ** 3, dtype=np.int32)
    np.add.at(out, lin, 1)
    return out
