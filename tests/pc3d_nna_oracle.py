"""float64 restatement (numpy) of 1-nearest-neighbour accuracy over two sets of clouds.  The referee of
tests/test_pc_nna_gpu.py; tests/test_pc_nna_host.py checks it against hand-computed matrices.

The T = S + R items are the samples 0 .. S - 1 and the references S .. T - 1.  Item t's distances are row t of the joint
matrix [[Dss, Dsr], [Dsr^T, Drr]]; the entry t itself is never a candidate, whatever it holds; +inf and NaN never win;
numpy's argmin takes the lowest index on a tie; an item with no candidate left gives (+inf, -1).
own[t] = (nn[t] < S) == (t < S);  acc = mean(own), acc_sample = mean(own[:S]), acc_ref = mean(own[S:]).
"""
import numpy as np


def joint_matrix(Dss, Dsr, Drr):
    """-> [T, T] float64 with +inf on the diagonal and in place of every NaN"""
    Dss, Dsr, Drr = (np.asarray(D, dtype=np.float64) for D in (Dss, Dsr, Drr))
    S, R = Dsr.shape
    assert Dss.shape == (S, S) and Drr.shape == (R, R)
    J = np.block([[Dss, Dsr], [Dsr.T, Drr]])
    J[np.isnan(J)] = np.inf
    np.fill_diagonal(J, np.inf)
    return J


def nn1_loo(Dss, Dsr, Drr):
    """-> (nn_val float64 [T], nn_arg int64 [T])"""
    J = joint_matrix(Dss, Dsr, Drr)
    arg = J.argmin(axis=1)
    val = J[np.arange(len(J)), arg]
    arg[np.isinf(val)] = -1
    return val, arg


def one_nn_accuracy(Dss, Dsr, Drr):
    """-> dict(acc, acc_sample, acc_ref, nn, nn_dist)"""
    val, arg = nn1_loo(Dss, Dsr, Drr)
    S = np.shape(Dsr)[0]
    own = (arg < S) == (np.arange(len(arg)) < S)
    return dict(acc=float(own.mean()), acc_sample=float(own[:S].mean()), acc_ref=float(own[S:].mean()), nn=arg, nn_dist=val)


def smallest_gap(Dss, Dsr, Drr):
    """the smallest relative gap (d2 - d1) / d2 between the best and the second-best candidate over all items (1.0 where an
    item has a single candidate): float32 matrices can only be asked for the float64 neighbour where this is large"""
    J = joint_matrix(Dss, Dsr, Drr)
    if J.shape[0] < 3:
        return 1.0
    d1, d2 = np.sort(J, axis=1)[:, :2].T
    gap = np.ones(len(J))
    some = np.isfinite(d2) & (d2 > 0)
    gap[some] = (d2[some] - d1[some]) / d2[some]
    gap[d2 == 0] = 0.0                      # (two candidates at distance 0: a tie)
    return float(gap.min())
