"""Fidelity and diversity figures on the FID features, on the device: improved precision / recall (Kynkaanniemi et al.
2019), density / coverage (Naeem et al. 2020) and KID (Binkowski et al. 2018).

FID is one number; these separate sharp samples (precision, density) from samples that cover the data (recall,
coverage), and KID stays unbiased on sets of a few thousand images.  All of them come from the Inception rows the FID pass
already produces:

    bank = FeatureBank(dims, device, capacity)          # keeps the rows an ActivationStatistics reduces to moments
    bank.update(act)                                    # what ActivationStatistics.update accepts
    d2 = sqdist_matrix(x, y)                            # [nx, ny] fp64, for sets small enough to hold it
    nn = knn_sqdist(x, y=None, k=3)                     # [n, k] fp64 ascending; y=None: the other rows of x
    cnt = count_within(q, x, radii)                     # int32 [nq]: in how many balls (x_i, radii[i]) q_j lies
    figures = prdc(real, fake, k=3)                     # precision, recall, density, coverage (+ the radii)
    mean, std = kid(real, fake, subsets=100, subset_size=1000)
    figures = calculate_fidelity_given_dataset(loader, model_s, batch_size, True, 2048, device, 50000)

Every distance is the squared distance max(0, |x|^2 + |y|^2 - 2 x.y) in fp64 (csrc/feat_pairs.hip), every comparison is
`<=` on squared distances.  Two equal rows are at a distance within 2 (d + 3) 2^-53 (|x| + |y|)^2 of 0, not exactly 0;
a row is never its own neighbour (left out by index).  The N x N matrices are never stored: the kernels reduce them tile
by tile, and `plan_slabs` cuts the columns into launches of at most FEAT_MACS_PER_LAUNCH multiply-adds.  The results do
not depend on the cutting.  The same-set matrices are computed whole (no use of their symmetry).  There is no CPU path.
"""
import torch

from . import fid as _fid
from . import infer, ops

# rows x columns x d of one launch of the strip kernels (knn / within); the column slabs are whole 64-column tiles.
# Set from profiles/fidelity_bench.txt: at 50 000 x 50 000 x 2048 a launch of 41 column tiles (the 2^38 this started
# from) took 17.1 ms, 0.418 ms a tile; 49 tiles keep the longest launch inside the 19 to 22 ms this project keeps to.
FEAT_MACS_PER_LAUNCH = 49 * 64 * 50000 * 2048
TILE = 64


def plan_slabs(nrows, ncols, d, macs=None):
    """-> [(c0, c1), ...]: [0, ncols) cut into launches of whole 64-column tiles (the last one may end inside a tile) of
    at most `macs` (default FEAT_MACS_PER_LAUNCH) multiply-adds nrows x (c1 - c0) x d each, and never less than one
    tile.  A pure function of its arguments."""
    macs = FEAT_MACS_PER_LAUNCH if macs is None else int(macs)
    nrows, ncols, d = int(nrows), int(ncols), int(d)
    if nrows < 1 or ncols < 1 or d < 1 or macs < 1:
        raise ValueError("plan_slabs: positive sizes, got rows %d, columns %d, d %d, budget %d" % (nrows, ncols, d, macs))
    width = max(1, macs // (nrows * d * TILE)) * TILE
    return [(c0, min(c0 + width, ncols)) for c0 in range(0, ncols, width)]


def _features(who, *xs):
    """float32 [n, d] device rows of one d, unit column stride (made contiguous otherwise)"""
    out = []
    for x in xs:
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("sivae_hip.fidelity.%s: features are on %s — the feature kernels need a ROCm device tensor "
                               "and have no CPU fallback" % (who, getattr(x, "device", type(x).__name__)))
        if x.dtype != torch.float32 or x.dim() != 2:
            raise TypeError("sivae_hip.fidelity.%s: features must be float32 [n, d], got %s %s"
                            % (who, x.dtype, tuple(x.shape)))
        if x.shape[1] != xs[0].shape[1]:
            raise ValueError("sivae_hip.fidelity.%s: feature dimensions differ: %d and %d"
                             % (who, xs[0].shape[1], x.shape[1]))
        if x.shape[0] < 1:
            raise ValueError("sivae_hip.fidelity.%s: no rows" % who)
        if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            x = x.contiguous()
        out.append(x)
    return out


def _norms(who, x):
    """squared row norms; the one check for non-finite features (an inf or NaN element makes its row's norm so)"""
    nrm = ops.feat_row_sqnorm(x)
    if not bool(torch.isfinite(nrm).all()):
        raise ValueError("sivae_hip.fidelity.%s: non-finite features" % who)
    return nrm


def _check_k(who, k, n_other):
    k = int(k)
    if not 1 <= k <= ops.FEAT_MAX_K:
        raise ValueError("sivae_hip.fidelity.%s: k must be in 1 .. %d, got %d" % (who, ops.FEAT_MAX_K, k))
    if n_other < k:
        raise ValueError("sivae_hip.fidelity.%s: %d neighbours asked for among %d other rows" % (who, k, n_other))
    return k


def _knn(x, nx, y, ny, k, self_pairs):
    best = ops.feat_knn_state(x.shape[0], k, x.device)
    for c0, c1 in plan_slabs(x.shape[0], y.shape[0], x.shape[1]):
        ops.feat_knn_update(x, nx, y, ny, best, c0, c1, self_pairs=self_pairs)
    return best


def _within(q, nq, x, nx, radii):
    count = ops.feat_within_state(q.shape[0], q.device)
    for c0, c1 in plan_slabs(q.shape[0], x.shape[0], q.shape[1]):
        ops.feat_within_update(q, nq, x, nx, radii, count, c0, c1)
    return count


@torch.no_grad()
def sqdist_matrix(x, y=None):
    """-> [nx, ny] fp64 squared distances (y=None: of x to itself; the diagonal is then within the bound of 0)"""
    x, y = _features("sqdist_matrix", x, x if y is None else y)
    nx = _norms("sqdist_matrix", x)
    return ops.feat_sqdist(x, nx, y, nx if y is x else _norms("sqdist_matrix", y))


@torch.no_grad()
def knn_sqdist(x, y=None, k=3):
    """-> [n, k] fp64, ascending: per row of x the k smallest squared distances to the rows of y, or (y=None) to the
    OTHER rows of x"""
    if y is None:
        x, = _features("knn_sqdist", x)
        k = _check_k("knn_sqdist", k, x.shape[0] - 1)
        nx = _norms("knn_sqdist", x)
        return _knn(x, nx, x, nx, k, True)
    x, y = _features("knn_sqdist", x, y)
    k = _check_k("knn_sqdist", k, y.shape[0])
    return _knn(x, _norms("knn_sqdist", x), y, _norms("knn_sqdist", y), k, False)


def _radii(who, radii, n, device):
    if not isinstance(radii, torch.Tensor) or not radii.is_cuda:
        raise RuntimeError("sivae_hip.fidelity.%s: radii are not on a ROCm device (no CPU fallback)" % who)
    if radii.dtype != torch.float64 or tuple(radii.shape) != (n,):
        raise ValueError("sivae_hip.fidelity.%s: radii must be float64 [%d], got %s %s"
                         % (who, n, radii.dtype, tuple(radii.shape)))
    if bool(torch.isnan(radii).any()):
        raise ValueError("sivae_hip.fidelity.%s: NaN radius" % who)
    return radii.contiguous()


@torch.no_grad()
def count_within(q, x, radii):
    """-> int32 [nq]: count[j] = #{ i : sqdist(q_j, x_i) <= radii[i] }; radii fp64 [nx] are SQUARED distances (+inf
    and negative values are allowed)"""
    q, x = _features("count_within", q, x)
    radii = _radii("count_within", radii, x.shape[0], x.device)
    return _within(q, _norms("count_within", q), x, _norms("count_within", x), radii)


@torch.no_grad()
def prdc(real, fake, k=3):
    """-> dict(precision, recall, density, coverage: Python floats; radii_real, radii_fake: fp64 device vectors)

    radii: the k-th smallest squared distance of a row to the other rows of its own set.
    precision = share of fake rows inside at least one real ball, recall = the same with the roles swapped,
    density = (number of (fake row, real ball) memberships) / (k n_fake), coverage = share of real rows whose nearest fake
    row lies inside their own ball."""
    real, fake = _features("prdc", real, fake)
    k = _check_k("prdc", k, min(real.shape[0], fake.shape[0]) - 1)
    nr, nf = _norms("prdc", real), _norms("prdc", fake)
    radii_real = _knn(real, nr, real, nr, k, True)[:, k - 1].contiguous()
    radii_fake = _knn(fake, nf, fake, nf, k, True)[:, k - 1].contiguous()
    in_real = _within(fake, nf, real, nr, radii_real)      # per fake row: the real balls it lies in
    in_fake = _within(real, nr, fake, nf, radii_fake)      # per real row: the fake balls it lies in
    nearest_fake = _knn(real, nr, fake, nf, 1, False)[:, 0]
    n_real, n_fake = real.shape[0], fake.shape[0]
    counts = torch.stack([(in_real > 0).sum(), (in_fake > 0).sum(), in_real.sum(dtype=torch.int64),
                          (nearest_fake <= radii_real).sum()]).tolist()  # (one read-back)
    return dict(precision=counts[0] / n_fake, recall=counts[1] / n_real, density=counts[2] / (k * n_fake),
                coverage=counts[3] / n_real, radii_real=radii_real, radii_fake=radii_fake)


def kid_indices(n_real, n_fake, subsets=100, subset_size=1000, seed=0):
    """-> (real_index, fake_index): int64 [subsets, subset_size] CPU tensors, every row drawn without replacement from
    a CPU torch.Generator seeded with `seed` (real row, fake row, real row, ... in subset order)"""
    subsets, m = int(subsets), int(subset_size)
    if subsets < 1 or m < 2 or m > min(int(n_real), int(n_fake)):
        raise ValueError("sivae_hip.fidelity.kid: %d subsets of %d rows out of %d real and %d fake rows"
                         % (subsets, m, n_real, n_fake))
    g = torch.Generator().manual_seed(int(seed))
    ri, fi = [], []
    for _ in range(subsets):
        ri.append(torch.randperm(int(n_real), generator=g)[:m])
        fi.append(torch.randperm(int(n_fake), generator=g)[:m])
    return torch.stack(ri), torch.stack(fi)


@torch.no_grad()
def kid_sums(real, fake, indices, degree=3, gamma=None, coef0=1.0):
    """-> (sxx, syy, sxy): fp64 [S] device vectors, per subset the sums of the polynomial kernel over i != j of the real
    rows, over i != j of the fake rows, and over all pairs (real, fake)"""
    real, fake = _features("kid", real, fake)
    _norms("kid", real), _norms("kid", fake)
    ri, fi = indices
    ri, fi = torch.as_tensor(ri, dtype=torch.int64), torch.as_tensor(fi, dtype=torch.int64)
    if ri.dim() != 2 or fi.shape != ri.shape or ri.shape[1] < 2:
        raise ValueError("sivae_hip.fidelity.kid: indices must be two int64 [subsets, subset_size >= 2] of one shape")
    if int(ri.min()) < 0 or int(ri.max()) >= real.shape[0] or int(fi.min()) < 0 or int(fi.max()) >= fake.shape[0]:
        raise ValueError("sivae_hip.fidelity.kid: index out of range")
    S, m = ri.shape
    d = real.shape[1]
    gamma = 1.0 / d if gamma is None else float(gamma)
    xs, ys = ops.feat_gather(real, ri.to(real.device)), ops.feat_gather(fake, fi.to(fake.device))  # [S, m, d], once
    step = max(1, FEAT_MACS_PER_LAUNCH // (m * m * d))
    parts = [[], [], []]
    for s0 in range(0, S, step):
        x, y = xs[s0:s0 + step], ys[s0:s0 + step]
        parts[0].append(ops.feat_poly_sums(x, x, gamma, coef0, degree, skip_diag=True))
        parts[1].append(ops.feat_poly_sums(y, y, gamma, coef0, degree, skip_diag=True))
        parts[2].append(ops.feat_poly_sums(x, y, gamma, coef0, degree, skip_diag=False))
    return tuple(torch.cat(p) for p in parts)


@torch.no_grad()
def kid(real, fake, subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1.0, seed=0, indices=None):
    """-> (mean, std): the kernel inception distance, the unbiased MMD^2 under k(x, y) = (gamma x.y + coef0)^degree
    (gamma defaults to 1 / d) averaged over `subsets` subsets of `subset_size` rows of each side, and its population
    deviation over the subsets.  indices: (real_index, fake_index), int64 [subsets, subset_size], instead of the seeded
    draw of `kid_indices`."""
    if indices is None:
        indices = kid_indices(real.shape[0], fake.shape[0], subsets, subset_size, seed)
    sxx, syy, sxy = kid_sums(real, fake, indices, degree, gamma, coef0)
    m = int(indices[0].shape[1])
    mmd2 = sxx / (m * (m - 1)) + syy / (m * (m - 1)) - 2.0 * sxy / (m * m)
    return float(mmd2.mean().item()), float(mmd2.std(unbiased=False).item())


class FeatureBank:
    """The first `capacity` feature rows seen, fp32 on the device (what ActivationStatistics reduces to moments, kept)."""

    def __init__(self, dims, device, capacity):
        self.dims, self.device, self.capacity = int(dims), torch.device(device), int(capacity)
        if self.device.type != "cuda":
            raise RuntimeError("sivae_hip.fidelity.FeatureBank: device %s is not a ROCm device (no CPU fallback)"
                               % self.device)
        if self.capacity < 1:
            raise ValueError("capacity must be positive")
        self._rows = ops.feat_bank(self.capacity, self.dims, self.device)
        self.rows_seen = 0

    @torch.no_grad()
    def update(self, act):
        if act.shape[0] == 0:
            return self
        act = _fid.activation_rows(act, self.dims)
        take = min(act.shape[0], self.capacity - min(self.rows_seen, self.capacity))
        if take > 0:
            self._rows[self.rows_seen:self.rows_seen + take].copy_(act[:take])
        self.rows_seen += act.shape[0]
        return self

    def rows(self, num=None):
        """-> the first `num` rows seen (all kept rows by default), a view [num, dims]"""
        kept = min(self.rows_seen, self.capacity)
        num = kept if num is None else int(num)
        if not 0 <= num <= kept:
            raise ValueError("sivae_hip.fidelity.FeatureBank: %d rows asked for, %d kept" % (num, kept))
        return self._rows[:num]


@torch.no_grad()
def real_features(dataloader, inception, dims, device, num_images, cuda=True):
    """fid.real_statistics that also keeps the rows -> ((mu, sigma), rows [num_images, dims])"""
    device = torch.device(device)
    stats, bank = _fid.ActivationStatistics(dims, device), FeatureBank(dims, device, num_images)
    for batch in dataloader:
        if isinstance(batch, (list, tuple)) and len(batch) in (2, 3):
            batch = batch[0]
        if cuda:
            batch = batch.to(device)
        act = inception(batch)[0][:num_images - stats.rows_seen]
        stats.update(act)
        bank.update(act)
        if stats.rows_seen >= num_images:
            break
    print("total real activations: ", (stats.rows_seen, dims))
    return stats.finalize(), bank.rows()


@torch.no_grad()
def calculate_fidelity_given_dataset(dataloader, model_s, batch_size, cuda, dims, device, num_images, inception=None,
                                     k=3, kid_subsets=100, kid_subset_size=1000, real=None):
    """fid.calculate_fid_given_dataset with the rows kept: one Inception pass per side feeds an ActivationStatistics and
    a FeatureBank -> dict(fid, precision, recall, density, coverage, kid_mean, kid_std) of Python floats.  `fid` is what
    calculate_fid_given_dataset returns on the same inputs.  KID subsets are cut to the rows there are.
    real: what `real_features` returned, which then skips the real side."""
    device = torch.device(device)
    if inception is None:
        inception = _fid.reference_inception(dims)
    if cuda:
        inception.to(device)
    if real is None:
        real = real_features(dataloader, inception, dims, device, num_images, cuda=cuda)
    (m1, s1), real_rows = real
    stats, bank = _fid.ActivationStatistics(dims, device), FeatureBank(dims, device, num_images)
    for images in infer.generate(model_s, num_images, batch_size, as_uint8=True, eval_mode=None):
        act = inception(ops.u8_to_f32(images))[0][:num_images - stats.rows_seen]
        stats.update(act)
        bank.update(act)
    print("total generated activations: ", (stats.rows_seen, dims))
    m2, s2 = stats.finalize()
    fake_rows = bank.rows()
    out = dict(fid=_fid.frechet_distance(m1, s1, m2, s2))
    figures = prdc(real_rows, fake_rows, k=k)
    out.update({name: figures[name] for name in ("precision", "recall", "density", "coverage")})
    size = min(int(kid_subset_size), real_rows.shape[0], fake_rows.shape[0])
    out["kid_mean"], out["kid_std"] = kid(real_rows, fake_rows, subsets=kid_subsets, subset_size=size)
    return out
