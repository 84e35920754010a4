"""numpy restatement of the earth mover's reconstruction loss and its gradient (csrc/pc_emd.hip::emd_loss_kernel,
sivae_hip.pointcloud.emd_loss_fwd), with a `dtype` argument: float64 is the referee of tests/test_pc_emd_loss_gpu.py,
float32 the yardstick its gates are taken from.  tests/test_pc_emd_loss_host.py checks it against an exact matching.

The cost and the plan are pc3d_emd_oracle.emd's (plan(k, l) = sum over the ten levels of t_j(k, l)).  The gradient is
matchcostgrad's, the plan held constant (it is NOT the derivative through the ratios):
    dleft[k]  =   sum_l plan(k, l) (A_k - B_l) / sqrt(d2(k, l))
    dright[l] = - sum_k plan(k, l) (A_k - B_l) / sqrt(d2(k, l))
a pair with d2 == 0 contributing zero; both divided by big = max(n, m) when normalised.  With the plan fixed the cost is
1-homogeneous in the points and invariant under a common translation:
    sum_k A_k . dleft[k] + sum_l B_l . dright[l] = cost (unnormalised),     sum_k dleft[k] + sum_l dright[l] = 0.
"""
import numpy as np

import pc3d_emd_oracle as MO


def emd_grad(left, right, normalize=False, dtype=np.float64):
    """left [n, 3], right [m, 3] -> (cost, dleft [n, 3], dright [m, 3]), every operation in `dtype` (the cost total in
    float64, as pc3d_emd_oracle.emd forms it)"""
    f = np.dtype(dtype).type
    cost, plan = MO.emd(left, right, normalize=False, dtype=dtype, return_plan=True)
    A, B = np.asarray(left, dtype=dtype), np.asarray(right, dtype=dtype)
    n, m = A.shape[0], B.shape[0]
    dleft, dright = np.zeros((n, 3), dtype=dtype), np.zeros((m, 3), dtype=dtype)
    for k0 in range(0, n, 512):  # (rows of the left cloud in blocks: [512, m, 3] at a time)
        diff = A[k0:k0 + 512, None, :] - B[None, :, :]
        d2 = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
        with np.errstate(divide="ignore"):
            coef = np.where(d2 > 0, plan[k0:k0 + 512] / np.sqrt(d2), f(0))
        pull = coef[..., None] * diff
        dleft[k0:k0 + 512] = pull.sum(axis=1, dtype=dtype)
        dright -= pull.sum(axis=0, dtype=dtype)
    if normalize:
        big = f(max(n, m))
        return cost / float(big), dleft / big, dright / big
    return cost, dleft, dright


def homogeneity_defect(left, right, cost, dleft, dright):
    """|sum A . dleft + sum B . dright - cost| / cost in float64, from unnormalised outputs of any precision"""
    A, B = np.asarray(left, dtype=np.float64), np.asarray(right, dtype=np.float64)
    total = float((A * np.asarray(dleft, dtype=np.float64)).sum() + (B * np.asarray(dright, dtype=np.float64)).sum())
    return abs(total - float(cost)) / float(cost)


def momentum_defect(dleft, dright):
    """max over the coordinates of |sum dleft + sum dright| / (sum |dleft| + sum |dright|), in float64"""
    gl, gr = np.asarray(dleft, dtype=np.float64), np.asarray(dright, dtype=np.float64)
    return float((np.abs(gl.sum(axis=0) + gr.sum(axis=0)) / (np.abs(gl).sum(axis=0) + np.abs(gr).sum(axis=0))).max())
