"""float64 numpy restatement of the pairwise figures on the FID features (csrc/feat_pairs.hip, sivae_hip/fidelity.py),
independent of both: direct-form squared distances sum_k (x_k - y_k)^2, k nearest neighbours by sorting, ball counts,
precision / recall / density / coverage, polynomial-kernel sums and KID.  Everything is done on the whole matrix: the
oracle is for the small shapes of the tests."""
import numpy as np

EPS64 = 2.0 ** -53


def sqdist(x, y):
    """[nx, ny] float64: sum_k (x_ik - y_jk)^2, the direct form (no cancellation)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    out = np.empty((x.shape[0], y.shape[0]))
    for i in range(x.shape[0]):
        diff = y - x[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def sqdist_bound(x, y):
    """the distance gate: the expanded form's three length-d fp64 accumulations against the direct form,
    |got - ref| <= 2 (d + 3) 2^-53 (max|x| + max|y|)^2"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = np.sqrt((x * x).sum(axis=1).max()), np.sqrt((y * y).sum(axis=1).max())
    return 2.0 * (x.shape[1] + 3) * EPS64 * (nx + ny) ** 2


def knn(x, y=None, k=3):
    """[n, k] ascending: the k smallest squared distances of every row of x to the rows of y, or (y None) to the OTHER
    rows of x (the row itself left out by index)"""
    d2 = sqdist(x, x if y is None else y)
    if y is None:
        d2[np.arange(d2.shape[0]), np.arange(d2.shape[0])] = np.inf
    return np.sort(d2, axis=1)[:, :k]


def count_within(q, x, radii):
    """int64 [nq]: count[j] = #{ i : sqdist(q_j, x_i) <= radii[i] }"""
    return (sqdist(q, x) <= np.asarray(radii, np.float64)[None, :]).sum(axis=1)


def membership_gap(q, x, radii):
    """the smallest |sqdist(q_j, x_i) - radii[i]| over all pairs with a finite radius: the membership tests are exact
    while this stays above the distance gate"""
    radii = np.asarray(radii, np.float64)
    gap = np.abs(sqdist(q, x) - radii[None, :])[:, np.isfinite(radii)]
    return float(gap.min()) if gap.size else np.inf


def prdc(real, fake, k=3):
    """-> dict(precision, recall, density, coverage, radii_real, radii_fake, gap): gap is the smallest distance of any
    compared pair (sqdist, radius) over the four figures, to be held against the distance gate"""
    radii_real, radii_fake = knn(real, None, k)[:, k - 1], knn(fake, None, k)[:, k - 1]
    in_real, in_fake = count_within(fake, real, radii_real), count_within(real, fake, radii_fake)
    nearest_fake = knn(real, fake, 1)[:, 0]
    n_real, n_fake = len(radii_real), len(radii_fake)
    gap = min(membership_gap(fake, real, radii_real), membership_gap(real, fake, radii_fake),
              float(np.abs(nearest_fake - radii_real).min()))
    return dict(precision=int((in_real > 0).sum()) / n_fake, recall=int((in_fake > 0).sum()) / n_real,
                density=int(in_real.sum()) / (k * n_fake), coverage=int((nearest_fake <= radii_real).sum()) / n_real,
                radii_real=radii_real, radii_fake=radii_fake, gap=gap)


def knn_gap(x, y=None, k=3):
    """the smallest difference between the k-th and the (k + 1)-th smallest distance of a row (inf when there is no
    (k + 1)-th): above twice the gate the k-th neighbour is the same for both forms"""
    d2 = sqdist(x, x if y is None else y)
    if y is None:
        d2[np.arange(d2.shape[0]), np.arange(d2.shape[0])] = np.inf
    s = np.sort(d2, axis=1)
    return float((s[:, k] - s[:, k - 1]).min()) if s.shape[1] > k else np.inf


def poly_kernel(x, y, gamma, coef0=1.0, degree=3):
    """[m, n] float64: (gamma x_i . y_j + coef0)^degree"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return (gamma * (x @ y.T) + coef0) ** degree


def poly_sum(x, y, gamma, coef0=1.0, degree=3, skip_diag=False):
    """-> (sum of the kernel over all pairs (i != j with skip_diag), sum of its absolute values, number of addends)"""
    kmat = poly_kernel(x, y, gamma, coef0, degree)
    if skip_diag:
        kmat = kmat[~np.eye(kmat.shape[0], kmat.shape[1], dtype=bool)]
    return float(kmat.sum()), float(np.abs(kmat).sum()), int(kmat.size)


def poly_sum_bound(d, addends, sum_abs):
    """2 (d + 3 + number of addends) 2^-53 sum |k_ij|"""
    return 2.0 * (d + 3 + addends) * EPS64 * sum_abs


def kid(real, fake, real_index, fake_index, degree=3, gamma=None, coef0=1.0):
    """-> (mean, population std, bound on |mean| and on every subset's MMD^2 from the three sum bounds) of the unbiased
    MMD^2 over the subsets real[real_index[s]], fake[fake_index[s]]"""
    real, fake = np.asarray(real, np.float64), np.asarray(fake, np.float64)
    d = real.shape[1]
    gamma = 1.0 / d if gamma is None else gamma
    vals, bounds = [], []
    for ri, fi in zip(np.asarray(real_index), np.asarray(fake_index)):
        x, y = real[ri], fake[fi]
        m = len(ri)
        (sxx, axx, cxx), (syy, ayy, cyy), (sxy, axy, cxy) = (poly_sum(x, x, gamma, coef0, degree, True),
                                                             poly_sum(y, y, gamma, coef0, degree, True),
                                                             poly_sum(x, y, gamma, coef0, degree, False))
        vals.append(sxx / (m * (m - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (m * m))
        bounds.append(poly_sum_bound(d, cxx, axx) / (m * (m - 1)) + poly_sum_bound(d, cyy, ayy) / (m * (m - 1))
                      + 2.0 * poly_sum_bound(d, cxy, axy) / (m * m))
    vals = np.array(vals)
    return float(vals.mean()), float(vals.std()), float(max(bounds))


def construction(n_real, n_fake, d, seed):
    """the test sets: real rows N(0, 1); the first half of the fake rows are real rows (the first ones, cyclically) plus
    0.05 N(0, 1), the second half 1.5 N(0, 1) + 0.5; float32"""
    g = np.random.default_rng(seed)
    real = g.standard_normal((n_real, d)).astype(np.float32)
    half = n_fake // 2
    near = real[np.arange(half) % n_real] + np.float32(0.05) * g.standard_normal((half, d)).astype(np.float32)
    far = np.float32(1.5) * g.standard_normal((n_fake - half, d)).astype(np.float32) + np.float32(0.5)
    fake = np.concatenate([near, far]).astype(np.float32)
    real.setflags(write=False)
    fake.setflags(write=False)
    return real, fake
