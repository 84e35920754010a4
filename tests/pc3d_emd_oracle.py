"""numpy restatement of the approximate-matching earth mover's distance (Fan, Su and Guibas' approxmatch / matchcost pair)
that csrc/pc_emd.hip computes, with a `dtype` argument: float64 is the referee of tests/test_pc_emd_gpu.py, float32 the
yardstick its gate is taken from.  tests/test_pc_emd_host.py checks it against exact optimal matchings.

For a left cloud A [n, 3] and a right cloud B [m, 3], d2(k, l) = |A_k - B_l|^2 in the direct form:
    big = max(n, m);  remL[k] = big / n;  remR[l] = big / m;  cost = 0
    for j = 7, 6, ..., -2:   level = -4^j, and 0 at j = -2;   w(k, l) = exp(level d2(k, l))
        1. suml[k] = 1e-9 + sum_l w(k, l) remR[l];   ratioL[k] = remL[k] / suml[k]
        2. sumr[l] = remR[l] sum_k w(k, l) ratioL[k];   ratioR[l] = remR[l] min(remR[l] / (sumr[l] + 1e-9), 1);
           remR[l] = max(0, remR[l] - sumr[l])
        3. t(k, l) = w(k, l) ratioL[k] ratioR[l];   cost += sum_kl t(k, l) sqrt(d2(k, l));   remL[k] = max(0, remL[k] - sum_l t(k, l))
    EMD(A, B) = cost / big when normalised, cost otherwise.
D[s, r] = EMD(left = ref_r, right = sample_s); a cloud with a NaN or infinite coordinate makes its row / column NaN.
"""
import numpy as np

LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)  # j = 7 ... -1, then 0 at j = -2


def emd(left, right, normalize=True, dtype=np.float64, return_plan=False):
    """left [n, 3], right [m, 3] -> EMD(left, right) as `dtype` (every operation in it; the cost total in float64), or
    (EMD, plan [n, m] = sum over the levels of t) with return_plan"""
    f = np.dtype(dtype).type
    A, B = np.asarray(left, dtype=dtype), np.asarray(right, dtype=dtype)
    n, m = A.shape[0], B.shape[0]
    diff = A[:, None, :] - B[None, :, :]
    d2 = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]   # [n, m]
    dist = np.sqrt(d2)
    big = f(max(n, m))
    remL = np.full(n, big / f(n), dtype=dtype)
    remR = np.full(m, big / f(m), dtype=dtype)
    eps = f(1e-9)
    cost = 0.0
    plan = np.zeros((n, m), dtype=dtype) if return_plan else None
    with np.errstate(under="ignore"):
        for level in LEVELS:
            w = np.exp(f(level) * d2)
            ratioL = remL / (eps + (w * remR[None, :]).sum(axis=1, dtype=dtype))
            sumr = remR * (w * ratioL[:, None]).sum(axis=0, dtype=dtype)
            ratioR = remR * np.minimum(remR / (sumr + eps), f(1))
            remR = np.maximum(f(0), remR - sumr)
            t = (w * ratioL[:, None]) * ratioR[None, :]
            cost += float((t * dist).sum(dtype=np.float64))
            remL = np.maximum(f(0), remL - t.sum(axis=1, dtype=dtype))
            if return_plan:
                plan += t
    value = cost / float(big) if normalize else cost
    return (value, plan) if return_plan else value


def emd_matrix(sample, ref, normalize=True, dtype=np.float64):
    """sample [S, M, 3], ref [R, N, 3] -> D [S, R] float64, D[s, r] = emd(left = ref_r, right = sample_s)"""
    sample, ref = np.asarray(sample), np.asarray(ref)
    S, R = sample.shape[0], ref.shape[0]
    D = np.full((S, R), np.nan, dtype=np.float64)
    ok_s = [bool(np.isfinite(sample[s]).all()) for s in range(S)]
    ok_r = [bool(np.isfinite(ref[r]).all()) for r in range(R)]
    for s in range(S):
        for r in range(R):
            if ok_s[s] and ok_r[r]:
                D[s, r] = emd(ref[r], sample[s], normalize, dtype)
    return D
