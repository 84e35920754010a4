"""GPU checks of the branches of csrc/pointcloud.hip and csrc/pc_jsd.hip that the small shapes of
tests/test_pointcloud_gpu.py and tests/test_pc_jsd_gpu.py never enter, at the smallest shapes that enter them:

  ReLU -> BatchNorm with S > 1 slices per channel (blockIdx.y > 0, seams inside a [b][c] row, the slice-order folds),
  the scalar (VEC = false) kernels for N % 4 != 0 and for pointers that are not 16-byte aligned,
  Chamfer with more than one LDS chunk of 2048 targets (c0 > 0) and with B > 64 (second block of the fold),
  the occupancy grid with more clouds than blocks (a block clears its bitmap between the clouds it owns),
  the grid-stride loop of the voxel histogram, js_divergence with fewer elements than threads,
  Conv1d(kernel_size=1) on one-row maps of odd width (the direct ks = 1 kernels with a ragged pixel tile),
  NaN propagation: relu keeps a NaN, the max over points lets a NaN win, Chamfer's loss stops being finite.

References are computed here in float64 from tests/pc3d_oracle.py / tests/pc3d_jsd_oracle.py; helpers and tolerances are
the ones of the two files above (imported, not restated).  tests/test_pointcloud_host.py asserts on the host that the
ReLU -> BatchNorm shapes below really give S > 1.
"""
import functools

import numpy as np
import pytest
import torch

import pc3d_jsd_oracle as JO
import pc3d_oracle as O
from support.pc import DEV, _BN, _PC, _chamfer_case, _check_indices_by_distance, _np, put, viol

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ ReLU -> BatchNorm
# the number of slices S of each shape is in O.RELU_BN_SLICED; tests/test_pointcloud_host.py::test_relu_bn_slice_counts
# asserts it on the host
RELU_BN_SLICED = list(O.RELU_BN_SLICED)


def _relu_bn_inputs(B, C, N):
    """test_relu_bn's construction: exact zeros, channel 0 dead everywhere"""
    g = torch.Generator().manual_seed(B * 1000 + C + N)
    a = torch.randn(B, C, N, generator=g)
    a[torch.rand(B, C, N, generator=g) < 0.1] = 0.0
    a[:, 0] = -a[:, 0].abs() - 0.1
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    dy = torch.randn(B, C, N, generator=g)
    return a, gamma, beta, dy


def _relu_bn_reference(a, gamma, beta, dy, bn):
    """fp64: O.relu_bn plus autograd -> dict of y, rm, rv, da, dgamma, dbeta"""
    a64 = a.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64, rm64, rv64 = O.relu_bn(a64, g64, b64, bn.running_mean.double().cpu(), bn.running_var.double().cpu(), True)
    (y64 * dy.double()).sum().backward()
    return dict(y=y64.detach(), rm=rm64, rv=rv64, da=a64.grad, dgamma=g64.grad, dbeta=b64.grad)


def _relu_bn_check(label, a, gamma, beta, dy, put_a=lambda t: t.to(DEV)):
    """the autograd Function on `put_a(a)` against fp64: test_relu_bn's assertions (training mode)"""
    PC = _PC()
    from sivae_hip import functional as SF
    C = a.shape[1]
    bn = _BN(C, True, 5)
    ref = _relu_bn_reference(a, gamma, beta, dy, bn)
    ad = put_a(a).requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    y = PC.relu_bn(ad, gd, bd, SF.BNState(bn))
    (y * dy.to(DEV)).sum().backward()
    got = dict(y=y, rm=bn.running_mean, rv=bn.running_var, da=ad.grad, dgamma=gd.grad, dbeta=bd.grad)
    figs = {k: viol(got[k], ref[k]) for k in ref}
    print("relu_bn %s %s: violation ratios %s" % (label, tuple(a.shape), {k: "%.3f" % v for k, v in figs.items()}))
    assert all(v <= 1.0 for v in figs.values()), figs
    assert int(bn.num_batches_tracked) == 4
    assert bool((ad.grad[a.to(DEV) == 0] == 0).all()) and bool((ad.grad[:, 0] == 0).all())
    return got, ref


@pytest.mark.parametrize("B,C,N", RELU_BN_SLICED)
def test_relu_bn_sliced(B, C, N):
    _relu_bn_check("S > 1", *_relu_bn_inputs(B, C, N))


@pytest.mark.parametrize("B,C,N,slice_len", [(3, 5, 1368, 3072), (3, 7, 2731, 3072)])
def test_relu_bn_slices_beyond_the_first_carry_the_mean(B, C, N, slice_len):
    """every value of channel 2 from the first seam on is 50 (the channel's index space is n = b N + i): a slice that is
    dropped, counted twice or read from the wrong row moves that channel's mean by tens of units — nothing rests on
    random values cancelling"""
    a, gamma, beta, dy = _relu_bn_inputs(B, C, N)
    ch = a[:, 2].reshape(-1).clone()
    assert ch.numel() > slice_len
    ch[slice_len:] = 50.0
    a[:, 2] = ch.view(B, N)
    got, ref = _relu_bn_check("seam", a, gamma, beta, dy)
    assert float(ref["rm"][2]) > 1.0  # (the planted slices dominate the channel's mean)


@pytest.mark.parametrize("B,C,N", [(2, 6, 64), (3, 5, 1368)])
def test_relu_bn_misaligned(B, C, N):
    """N % 4 == 0 but a pointer 4 bytes off a 16-byte boundary: the scalar kernels (the second shape with S = 2).
    Forward and backward through the Function with a misaligned `a`; then the tensor-level backward where ONLY dy is
    misaligned (the mixed case)."""
    PC = _PC()
    assert N % 4 == 0
    a, gamma, beta, dy = _relu_bn_inputs(B, C, N)
    got, ref = _relu_bn_check("misaligned a", a, gamma, beta, dy, put_a=functools.partial(put, misaligned=True))
    ad, dyd = a.to(DEV), put(dy, misaligned=True)
    assert ad.data_ptr() % 16 == 0 and dyd.data_ptr() % 16 == 4
    mean, invstd = PC.relu_bn_stats(ad)
    da, dgamma, dbeta = PC.relu_bn_bwd(dyd, ad, mean, invstd, gamma.to(DEV))
    figs = dict(da=viol(da, ref["da"]), dgamma=viol(dgamma, ref["dgamma"]), dbeta=viol(dbeta, ref["dbeta"]))
    print("relu_bn_bwd misaligned dy %s: violation ratios %s" % ((B, C, N), {k: "%.3f" % v for k, v in figs.items()}))
    assert all(v <= 1.0 for v in figs.values()), figs
    assert bool((da[ad == 0] == 0).all()) and bool((da[:, 0] == 0).all())


def test_relu_bn_propagates_nan():
    """one NaN in channel 1 (torch's relu keeps it): that channel's output, running statistics and dgamma are NaN, the
    other channels are untouched — 16-byte path, scalar path and S = 2"""
    PC = _PC()
    from sivae_hip import functional as SF
    for B, C, N in [(2, 4, 36), (2, 4, 33), (3, 5, 1368)]:
        a, gamma, beta, dy = _relu_bn_inputs(B, C, N)
        a[B - 1, 1, N - 3] = float("nan")
        bn = _BN(C, True, 5)
        ref = _relu_bn_reference(a, gamma, beta, dy, bn)
        assert bool(ref["y"][:, 1].isnan().all()) and bool(ref["rm"][1].isnan()) and bool(ref["dgamma"][1].isnan())
        ad = a.to(DEV).requires_grad_(True)
        gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
        y = PC.relu_bn(ad, gd, bd, SF.BNState(bn))
        (y * dy.to(DEV)).sum().backward()
        assert bool(y[:, 1].isnan().all())
        # da of the NaN channel: NaN wherever the gate a > 0 is open (mean and dgamma are NaN), 0 where it is closed —
        # which includes the NaN element itself (NaN > 0 is false; torch would pass a NaN there)
        ac, dac = a[:, 1], ad.grad[:, 1].cpu()
        assert bool(dac[ac > 0].isnan().all()) and bool((dac[~(ac > 0)] == 0).all())
        assert bool(bn.running_mean[1].isnan()) and bool(bn.running_var[1].isnan()) and bool(gd.grad[1].isnan())
        keep = torch.tensor([c for c in range(C) if c != 1])
        got = dict(y=y, rm=bn.running_mean, rv=bn.running_var, da=ad.grad, dgamma=gd.grad, dbeta=bd.grad)
        figs = {}
        for k, v in got.items():
            dim = 1 if v.dim() == 3 else 0
            figs[k] = viol(v.detach().cpu().index_select(dim, keep), ref[k].index_select(dim, keep))
        print("relu_bn with a NaN %s: violation ratios of the other channels %s"
              % ((B, C, N), {k: "%.3f" % v for k, v in figs.items()}))
        assert all(v <= 1.0 for v in figs.values()), figs


# ------------------------------------------------------------------------------------------------ max over points
def _first_index_of_max(x):
    want = x.max(dim=2)[0]
    N = x.shape[2]
    return want, torch.where(x == want[:, :, None], torch.arange(N)[None, None, :], N).min(dim=2)[0]


def _max_points_check(x, put=lambda t: t.to(DEV)):
    """test_max_points' assertions: values equal x.max(2), the lowest index on ties, the scatter gradient"""
    PC = _PC()
    B, C, N = x.shape
    want, first = _first_index_of_max(x)
    vals, arg = PC.max_points_fwd(put(x))
    assert torch.equal(vals.cpu(), want)
    assert torch.equal(arg.cpu().long(), first)
    gy = torch.randn(B, C, generator=torch.Generator().manual_seed(N))
    xd = put(x).requires_grad_(True)
    out = PC.max_points(xd)
    assert torch.equal(out, vals)
    (out * gy.to(DEV)).sum().backward()
    scatter = torch.zeros(B, C, N).scatter_(2, first[:, :, None], gy[:, :, None])
    assert torch.equal(xd.grad.cpu(), scatter)
    return vals, arg


def _max_points_rows(B, C, N, k):
    """random rows with: row 0 all equal, row 1 the maximum twice in different lanes (i and i + 64 k + 1), row 2 all -inf,
    row 3 the maximum twice in one lane (i and i + 64), row 4 the maximum in the last element"""
    x = torch.randn(B, C, N, generator=torch.Generator().manual_seed(B + C + N))
    rows = x.view(B * C, N)
    rows[0] = 0.25
    rows[1, 5] = rows[1, 5 + 64 * k + 1] = 9.0
    rows[2] = float("-inf")
    rows[3, 3] = rows[3, 3 + 64] = 8.0
    rows[4, N - 1] = 7.0
    return x


@pytest.mark.parametrize("B,C,N,k", [(3, 5, 101, 1), (2, 3, 257, 3), (1, 7, 131, 1)])
def test_max_points_scalar_path(B, C, N, k):
    assert N % 4 != 0 and N > 64 and (B * C) % 4 != 0 and 5 + 64 * k + 1 < N
    x = _max_points_rows(B, C, N, k)
    vals, arg = _max_points_check(x)
    arg = arg.view(-1).tolist()
    assert arg[:5] == [0, 5, 0, 3, N - 1]
    assert float(vals.view(-1)[2]) == float("-inf")


def test_max_points_misaligned():
    """N % 4 == 0 with x 4 bytes off a 16-byte boundary: the scalar kernel"""
    x = _max_points_rows(3, 5, 132, 1)
    vals, arg = _max_points_check(x, put=functools.partial(put, misaligned=True))
    assert arg.view(-1).tolist()[:5] == [0, 5, 0, 3, 131]


@pytest.mark.parametrize("N", [132, 101])
def test_max_points_propagates_nan(N):
    """a row with a NaN has the value NaN; index and gradient position are those of torch.max on the CPU for the same
    row (computed here); rows without a NaN are unaffected.  16-byte path (N = 132) and scalar path (N = 101)."""
    PC = _PC()
    B, C = 2, 5
    x = torch.randn(B, C, N, generator=torch.Generator().manual_seed(N))
    nan, inf = float("nan"), float("inf")
    rows = x.view(B * C, N)
    rows[0, 70] = nan                    # one NaN
    rows[1, 97] = rows[1, 30] = nan      # two, in different lanes: the lower index
    rows[2, 3] = nan
    rows[2, 90] = 1e30                   # a larger number behind the NaN does not take over
    rows[3, 2] = inf
    rows[3, 66] = nan                    # nor does +inf in front of it keep the lead
    rows[4] = nan                        # a row of NaNs
    rows[5, 7] = rows[5, 7 + 64] = nan   # two in one lane (scalar path) / in different lanes (16-byte path)
    want, widx = torch.max(x, dim=2)
    has_nan = x.isnan().any(dim=2)
    assert bool(want[has_nan].isnan().all()) and int(has_nan.sum()) == 6
    vals, arg = PC.max_points_fwd(x.to(DEV))
    vals, arg = vals.cpu(), arg.cpu().long()
    print("max_points with NaNs, N = %d: indices %s, torch.max on the CPU %s"
          % (N, arg.view(-1).tolist(), widx.view(-1).tolist()))
    assert torch.equal(vals.isnan(), has_nan) and torch.equal(vals[~has_nan], want[~has_nan])
    assert torch.equal(arg, widx)
    gy = torch.randn(B, C, generator=torch.Generator().manual_seed(1)) + 3.0
    xd = x.to(DEV).requires_grad_(True)
    out = PC.max_points(xd)
    assert torch.equal(out.isnan().cpu(), has_nan)
    out.backward(gy.to(DEV))
    scatter = torch.zeros(B, C, N).scatter_(2, widx[:, :, None], gy[:, :, None])
    assert torch.equal(xd.grad.cpu(), scatter)


# ------------------------------------------------------------------------------------------------ Chamfer
# (B, N, M, seed): more than one chunk of 2048 targets in one or both directions; B > 64.  Seed 995 is the first seed of
# _chamfer_case's draw for which one of the 5 predictions has ground-truth point 2048 — the only one of the second
# chunk — as its nearest neighbour, with a relative gap above 1e-2 to the second nearest (re-asserted in the test).
CHAMFER_CHUNKED = [(1, 2049, 5, 995), (2, 4100, 300, 1), (1, 300, 4100, 2), (70, 3, 2, 3)]


def _chamfer_check(preds, gts, P, want, seed):
    """loss 1e-5 relative, indices by distance, backward (both sides, one side only) against the formula evaluated with
    the kernel's own indices -> (idx_p, idx_g, dP, dG) of the kernel"""
    PC = _PC()
    B, M, N = preds.shape[0], preds.shape[1], gts.shape[1]
    p, q = preds.to(DEV), gts.to(DEV)
    loss, idx_p, idx_g = PC.chamfer_fwd(p, q)
    assert loss.shape == (B,) and idx_p.shape == (B, M) and idx_g.shape == (B, N)
    err = float(((loss.double().cpu() - want).abs() / want).max())
    print("chamfer fwd (%d, %d, %d): rel err %.3e" % (B, N, M, err))
    assert err <= 1e-5
    _check_indices_by_distance(P, idx_p, idx_g)
    w = torch.rand(B, generator=torch.Generator().manual_seed(seed + 100)) + 0.5
    dP, dG = O.chamfer_grads_from_indices(w.double(), preds.double(), gts.double(), idx_p.cpu(), idx_g.cpu())
    both = PC.chamfer_bwd(w.to(DEV), p, q, idx_p, idx_g, True, True)
    only_p = PC.chamfer_bwd(w.to(DEV), p, q, idx_p, idx_g, True, False)
    only_g = PC.chamfer_bwd(w.to(DEV), p, q, idx_p, idx_g, False, True)
    assert only_p[1] is None and only_g[0] is None
    assert torch.equal(only_p[0], both[0]) and torch.equal(only_g[1], both[1])
    for got, ref in ((both[0], dP), (both[1], dG)):
        err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
        print("chamfer bwd (%d, %d, %d): max err / max|grad| %.3e" % (B, N, M, err))
        assert err <= 1e-5
    return idx_p.cpu().long(), idx_g.cpu().long(), both[0].double().cpu(), both[1].double().cpu(), dP, dG


@pytest.mark.parametrize("B,N,M,seed", CHAMFER_CHUNKED)
def test_chamfer_beyond_one_chunk(B, N, M, seed):
    preds, gts, P, want = _chamfer_case(B, N, M, seed)
    # the second chunk holds a winner by a margin float32 cannot miss, in each direction with more than 2048 targets
    for dim, n_targets in ((1, N), (2, M)):
        if n_targets > 2048:
            s, i = P.sort(dim=dim)
            far = i.select(dim, 0) >= 2048
            gap = ((s.select(dim, 1) - s.select(dim, 0)) / s.select(dim, 1))[far]
            assert far.any() and float(gap.max()) >= 1e-2
    idx_p, idx_g = _chamfer_check(preds, gts, P, want, seed)[:2]
    if N > 2048:
        assert int(idx_p.max()) >= 2048
    if M > 2048:
        assert int(idx_g.max()) >= 2048


def test_chamfer_tie_across_the_chunk_seam():
    """an exact copy of target 10 at index 2058 (second chunk) and a query exactly on it, in both directions: the index
    is 10, and the gradients of the three points involved follow the formula (both copies chose the query)"""
    B, N, M = 1, 2100, 2100
    g = torch.Generator().manual_seed(17)
    gts = torch.rand(B, N, 3, generator=g, dtype=torch.float64).float()
    preds = torch.rand(B, M, 3, generator=g, dtype=torch.float64).float()
    gts[:, 2058] = gts[:, 10]
    preds[:, 0] = gts[:, 10]
    preds[:, 2058] = preds[:, 10]
    gts[:, 1] = preds[:, 10]
    P = O.pairwise_sqdist(preds.double(), gts.double())
    want = P.min(dim=1)[0].sum(1) + P.min(dim=2)[0].sum(1)
    idx_p, idx_g, gP, gG, dP, dG = _chamfer_check(preds, gts, P, want, 17)
    assert int(idx_p[0, 0]) == 10 and int(idx_g[0, 1]) == 10
    assert int(idx_g[0, 10]) == 0 and int(idx_g[0, 2058]) == 0 and int(idx_p[0, 10]) == 1 and int(idx_p[0, 2058]) == 1
    for got, ref, pts in ((gP, dP, (0, 10, 2058)), (gG, dG, (1, 10, 2058))):
        for j in pts:
            assert float((got[0, j] - ref[0, j]).abs().max()) <= 1e-5 * float(ref.abs().max()), j


def test_chamfer_nan_poisons_its_own_batch_element_only():
    PC = _PC()
    preds, gts, P, want = _chamfer_case(3, 70, 33, 2)
    clean = PC.chamfer_fwd(preds.to(DEV), gts.to(DEV))[0]
    for side in (0, 1):
        p, q = preds.clone(), gts.clone()
        (p if side == 0 else q)[1, 4, 1] = float("nan")
        loss = PC.chamfer_fwd(p.to(DEV), q.to(DEV))[0]
        print("chamfer with a NaN in %s of element 1: loss %s" % (("preds", "gts")[side], loss.tolist()))
        assert not bool(torch.isfinite(loss[1]))
        assert torch.equal(loss[[0, 2]], clean[[0, 2]])


# ------------------------------------------------------------------------------------------------ the JSD metric
def _draw_clouds(seed, shape, scale, cells, shared_point=False):
    """(u - 0.5) * scale from PCG64(seed); a point whose nearest / second-nearest gap is under JO.GAP is replaced by
    0.01 (test_many_tiles_and_list_flushes); shared_point: point 0 of EVERY cloud is 0.01, so one cell is touched by all
    of them -> (x, counters, bernoulli, points replaced)"""
    g = np.random.Generator(np.random.PCG64(seed))
    x = ((g.random(size=shape, dtype=np.float32) - np.float32(0.5)) * np.float32(scale)).astype(np.float32)
    if shared_point:
        x[:, 0] = 0.01
    counters, bernoulli, gap = JO.occupancy(x, cells)
    bad = gap < JO.GAP
    if bad.any():
        x[bad] = 0.01
        counters, bernoulli, gap = JO.occupancy(x, cells)
    assert gap.min() >= JO.GAP
    return x, counters, bernoulli, int(bad.sum())


@functools.lru_cache(maxsize=None)
def _many_clouds_case(clip):
    if clip:
        return _draw_clouds(7, (600, 40, 3), 1.6, JO.grid(8, True)[0])
    # N = 3, not 8: the float64 reference is brute force over 64 000 cells, 1.5 ms of host time per point (3.5 s at N = 8,
    # 1.3 s here).  What the case is for does not depend on N: 300 clouds on fewer blocks, global atomics per point, and
    # point 0 of every cloud in one cell, so that two clouds of one block always share a cell.
    return _draw_clouds(7, (300, 3, 3), 1.1, JO.grid(40, False)[0], shared_point=True)


@pytest.mark.parametrize("clip,res", [(True, 8), (False, 40)])
def test_occupancy_grid_many_clouds_per_block(clip, res):
    """more clouds than blocks (one block per CU at most): a block owns several clouds, clears its per-cloud bitmap
    between them and accumulates its per-cloud histogram across them.  Resolution 8 clipped: the LDS histograms and the
    exhaustive route; resolution 40 unclipped: global atomics per point.  Some cell is touched by more clouds than
    there are blocks (asserted), so two clouds of one block share a cell whatever the CU count: a bitmap that is not
    cleared between them loses a count."""
    PC = _PC()
    x, counters, bernoulli, replaced = _many_clouds_case(clip)
    S, N = x.shape[:2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("S = %d clouds of %d points on %d CUs, %d points replaced for the gap, largest per-cell cloud count %d"
          % (S, N, cus, replaced, int(bernoulli.max())))
    assert S > cus and int(bernoulli.max()) > cus, (
        "the case needs more clouds (%d), and more clouds touching one cell (%d), than the device has CUs (%d): the "
        "kernel launches one block per CU at most; on a larger part raise S" % (S, int(bernoulli.max()), cus))
    xd = torch.from_numpy(x).to(DEV)
    view = xd.permute(0, 2, 1).contiguous().transpose(1, 2)  # [S, 3, N] in memory, read in place
    assert not view.is_contiguous() and view.shape == (S, N, 3) and view.stride() == (3 * N, 1, N)
    for t in (xd, view):
        c, b, status = PC.occupancy_grid(t, res, clip, return_status=True)
        assert (int(status[1]) > 0) == clip
        assert np.array_equal(_np(c), counters) and np.array_equal(_np(b), bernoulli)
        c2, b2 = PC.occupancy_grid(t, res, clip)
        assert torch.equal(c2, c) and torch.equal(b2, b)
        c3, b3 = PC.occupancy_grid(t, res, clip, want_bernoulli=False)
        assert b3 is None and torch.equal(c3, c)


def test_voxel_histogram_grid_stride():
    """540 000 points: more than the 2048 x 256 threads of the largest grid, so threads take a second point"""
    PC = _PC()
    g = np.random.Generator(np.random.PCG64(9))
    x = ((g.random(size=(3, 180000, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
    assert x.shape[0] * x.shape[1] > 2048 * 256
    want = JO.voxel_distribution(x, 28)
    got = PC.voxel_histogram(torch.from_numpy(x).to(DEV), 28)
    assert got.dtype == torch.int32 and int(got.sum()) == 540000 and np.array_equal(_np(got), want)


@pytest.mark.parametrize("n", [1, 5, 63, 1025])
def test_js_divergence_short_vectors(n):
    """fewer elements than the 1024 threads (idle waves in both block sums), and one more than that"""
    PC = _PC()
    g = np.random.Generator(np.random.PCG64(n))
    for kind in ("int32", "float64"):
        if kind == "int32":
            P, Q = g.integers(0, 50, size=n).astype(np.int32), g.integers(0, 50, size=n).astype(np.int32)
        else:
            P, Q = g.random(size=n) * 7.3, g.random(size=n) * 0.9
            P[n // 2] = 0.0  # (0 log 0 = 0)
        P[0] += 1  # (no all-zero vector)
        Q[n - 1] += 2
        got = float(PC.js_divergence(torch.from_numpy(P).to(DEV), torch.from_numpy(Q).to(DEV)))
        want = JO.js_divergence(P, Q)
        print("js_divergence n = %d %s: %.15g, |error| %.3e" % (n, kind, got, abs(got - want)))
        assert abs(got - want) <= 1e-10


# ------------------------------------------------------------------------------------------------ Conv1d(kernel_size=1)
POINTWISE = [(2, 3, 64, 101), (3, 64, 128, 33), (2, 128, 256, 1), (1, 256, 512, 2049)]


@functools.lru_cache(maxsize=None)
def _pointwise_case(B, Ci, Co, N):
    g = torch.Generator().manual_seed(B + Ci + Co + N)
    x = torch.randn(B, Ci, N, generator=g)
    w = torch.randn(Co, Ci, 1, generator=g) / Ci ** 0.5
    bias = torch.randn(Co, generator=g) * 0.5
    dy = torch.randn(B, Co, N, generator=g)
    return x, w, bias, dy


def _pointwise_reference(x, w, bias, dy, relu, dtype):
    # (clones: .to() of a float32 tensor to float32 is the cached input itself, which must stay a plain leaf)
    xs, ws = x.clone().to(dtype).requires_grad_(True), w.clone().to(dtype).requires_grad_(True)
    bs = None if bias is None else bias.clone().to(dtype).requires_grad_(True)
    pre = torch.nn.functional.conv1d(xs, ws, bs)
    y = torch.relu(pre) if relu else pre
    (y * dy.to(dtype)).sum().backward()
    return dict(y=y.detach(), pre=pre.detach(), dx=xs.grad, dw=ws.grad, db=None if bs is None else bs.grad)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("B,Ci,Co,N", POINTWISE)
def test_pointwise_conv_one_row_maps(B, Ci, Co, N, with_bias, relu):
    """PC.pointwise_conv against an fp64 conv1d on [B, Ci, 1, N] maps of odd width: forward by the element-wise
    criterion, dx / dw / db by relative L2 against fp64 with the gate max(4 e32, 1e-5), e32 the error of the same
    restatement in fp32 on the CPU.

    With the fused ReLU the gradient is only well-conditioned away from the kink: where the fp64 pre-activation is within
    1e-4 of 0 (100 x the fp32 error of these sums of <= 256 O(1) terms) the upstream gradient is set to 0, so that a
    float32 run that lands on the other side of 0 there changes nothing; the forward check keeps those elements."""
    from sivae_hip import ops
    PC = _PC()
    x, w, bias, dy = _pointwise_case(B, Ci, Co, N)
    bias = bias if with_bias else None
    if relu:
        pre = _pointwise_reference(x, w, bias, dy, False, torch.float64)["pre"]
        near = pre.abs() < 1e-4
        dy = torch.where(near, torch.zeros(()), dy)
        print("pointwise %s: %d of %d pre-activations within 1e-4 of the kink" % ((B, Ci, Co, N), int(near.sum()), near.numel()))
        assert int(near.sum()) <= 0.001 * near.numel()  # (the mask must stay negligible: the gradient check is about the rest)
    ref = _pointwise_reference(x, w, bias, dy, relu, torch.float64)
    r32 = _pointwise_reference(x, w, bias, dy, relu, torch.float32)
    print("pointwise %s bias %s relu %s: routes forward %s, data gradient %s, weight gradient %s"
          % ((B, Ci, Co, N), with_bias, relu,
             ops.conv2d_fwd_route(B, Ci, Co, 1, N, 1, packed=True, mode=0, bias=with_bias).family,
             ops.conv2d_fwd_route(B, Co, Ci, 1, N, 1, packed=True, mode=1).family,
             ops.conv2d_wgrad_route(B, Ci, Co, 1, N, 1).family))
    xd, wd = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    bd = None if bias is None else bias.to(DEV).requires_grad_(True)
    y = PC.pointwise_conv(xd, wd, bd, relu=relu)
    assert y.shape == (B, Co, N)
    (y * dy.to(DEV)).sum().backward()
    v = viol(y, ref["y"])
    print("  y: %.3f of the element-wise criterion" % v)
    assert v <= 1.0
    bad = []
    for k, t in (("dx", xd), ("dw", wd), ("db", bd)):
        if t is None:
            continue
        e_gpu, e32 = O.rel_l2(t.grad, ref[k]), O.rel_l2(r32[k], ref[k])
        gate = max(4 * e32, 1e-5)
        print("  %s: gpu %.3e  cpu-fp32 %.3e  gate %.3e" % (k, e_gpu, e32, gate))
        if not e_gpu <= gate:
            bad.append((k, e_gpu, gate))
    assert not bad, bad
