"""float64 restatement (numpy) of the 3-D variant's set-to-set evaluation: the all-pairs Chamfer matrix, minimum matching
distance and coverage.  The referee of tests/test_pc_eval_gpu.py; tests/test_pc_eval_host.py checks it against
hand-computed clouds.

For clouds P [M, 3] and Q [N, 3]:  a_j = min_i |P_j - Q_i|^2,  b_i = min_j |P_j - Q_i|^2  (direct form),
CD(P, Q) = sum_j f(a_j) / m + sum_i f(b_i) / n,  f(t) = t or sqrt(t),  m = M and n = N when normalised, else 1.
D[s, r] = CD(sample_s, ref_r);  MMD = mean_r min_s D[s, r];  COV = |{argmin_r D[s, r] : s}| / R;  numpy's argmin takes the
lowest index on a tie.  A NaN or infinite coordinate makes every entry of its row / column of D non-finite (NaN here).
"""
import numpy as np


def chamfer_matrix(sample, ref, normalize=True, use_sqrt=False):
    """sample [S, M, 3], ref [R, N, 3] (any float dtype; taken to float64) -> D [S, R] float64"""
    sample, ref = np.asarray(sample, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    S, M, _ = sample.shape
    R, N, _ = ref.shape
    D = np.empty((S, R), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            diff = sample[s][None, :, None, :] - ref[:, None, :, :]          # [R, M, N, 3]
            d = diff[..., 0] ** 2 + diff[..., 1] ** 2 + diff[..., 2] ** 2     # [R, M, N]
            a, b = d.min(axis=2), d.min(axis=1)                               # [R, M], [R, N]  (NaN propagates)
            if use_sqrt:
                a, b = np.sqrt(a), np.sqrt(b)
            D[s] = a.sum(axis=1) / (M if normalize else 1) + b.sum(axis=1) / (N if normalize else 1)
    D[~np.isfinite(D)] = np.nan
    return D


def match_min(D):
    """-> (row_min [S], row_arg [S], col_min [R], col_arg [R]) of a finite matrix, lowest index on a tie"""
    D = np.asarray(D, dtype=np.float64)
    return D.min(axis=1), D.argmin(axis=1), D.min(axis=0), D.argmin(axis=0)


def minimum_matching_distance(D):
    """-> (mmd, matched_dists [R], the sample index behind each [R])"""
    _, _, col_min, col_arg = match_min(D)
    return float(col_min.mean()), col_min, col_arg


def coverage(D):
    """-> (cov, matched_ref [S], matched_dist [S])"""
    row_min, row_arg, _, _ = match_min(D)
    return len(np.unique(row_arg)) / float(D.shape[1]), row_arg, row_min


def smallest_gap(D):
    """the smallest relative gap (d2 - d1) / d2 between the best and the second best entry over every row and every
    column of D (1.0 for a line of one entry): float32 can only be asked for the float64 argmin where this is large"""
    D = np.asarray(D, dtype=np.float64)
    worst = 1.0
    for X in (D, D.T):
        if X.shape[1] < 2:
            continue
        two = np.sort(X, axis=1)[:, :2]
        worst = min(worst, float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()))
    return worst
