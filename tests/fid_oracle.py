"""float64 numpy restatement of the FID arithmetic (csrc/fid.hip, sivae_hip/fid.py), independent of both: the centred
moments the reference takes (np.mean / np.cov, soft_intro_vae/metrics/fid_score.py:349-350), the uncentred formula of the
finalize kernel, and the Frechet distance in its symmetric eigenvalue form."""
import numpy as np


def centred_moments(act):
    """what the reference computes from its activation array: (np.mean, np.cov) in float64"""
    act = np.asarray(act, dtype=np.float64)
    return np.mean(act, axis=0), np.atleast_2d(np.cov(act, rowvar=False))


def moment_state(act):
    """(n, s, G): the additive state, s = column sums, G = A^T A, float64"""
    act = np.asarray(act, dtype=np.float64)
    return act.shape[0], act.sum(axis=0), act.T @ act


def uncentred_moments(act):
    """the finalize kernel's formula on the additive state: mu = s / n, sigma = (G - s s^T / n) / (n - 1)"""
    n, s, G = moment_state(act)
    with np.errstate(invalid="ignore", divide="ignore"):
        return s / n, (G - np.outer(s, s) / n) / (n - 1)


def uncentred_deviation(act):
    """worst deviation of the uncentred sigma from the centred one, relative to max|sigma|: what a different summation
    order of the same fp64 arithmetic may cost on these inputs (the gates of the GPU tests are 16 times this)"""
    sigma = centred_moments(act)[1]
    return float(np.abs(uncentred_moments(act)[1] - sigma).max() / np.abs(sigma).max())


def sqrt_psd(sigma):
    """the symmetric square root through the eigen-decomposition, eigenvalues clamped at 0"""
    w, v = np.linalg.eigh(np.asarray(sigma, dtype=np.float64))
    x = (v * np.maximum(w, 0.0) ** 0.25).T          # diag(max(w, 0)^(1/4)) V^T
    return x.T @ x


def inner_matrix(sigma1, sigma2):
    """M = R sigma2 R with R = sigma1^(1/2), symmetrised the way the kernel's mirror does (upper triangle wins)"""
    r = sqrt_psd(sigma1)
    m = r.T @ (np.asarray(sigma2, dtype=np.float64).T @ r)
    return np.triu(m) + np.triu(m, 1).T


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + Tr sigma1 + Tr sigma2 - 2 sum sqrt(max(lambda_i, 0)), lambda = eigenvalues of R sigma2 R"""
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, np.float64)), np.atleast_1d(np.asarray(mu2, np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, np.float64)), np.atleast_2d(np.asarray(sigma2, np.float64))
    lam = np.linalg.eigvalsh(inner_matrix(sigma1, sigma2))
    diff = mu1 - mu2
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())
