"""GPU checks of the 3-D variant's earth mover's reconstruction loss: sivae_emd_loss (csrc/pc_emd.hip::emd_loss_kernel),
sivae_hip.pointcloud.emd_loss_fwd / EmdFn / emd_distance and the drop-in
soft_intro_vae_3d/losses/earth_mover_distance.py::EMD, against the existing emd_matrix (the cost, bit for bit) and the
float64 restatement tests/pc3d_emd_grad_oracle.py on the same float32 inputs (the gradients).  Clouds are seeded PCG64,
uniform in the cube of side 1 about the origin, except where said.

Gates: every gate is 16 x the worst error of the FLOAT32 ORACLE over its own class of cases, computed here (the yardstick
is the restatement, never the kernel; the factor covers the hardware exp2, sqrt and rsq, flushed denormals and another
summation shape).  The gradient's measure is max|g - g64| / max|g64| per pair and side, in two classes that differ by two
orders of magnitude: with N = M the remainders run to zero and single plan entries flip between near-equidistant
neighbours.  Measured on the CPU when the cases were chosen:
    unequal sizes: float32 oracle worst 4.94e-5 -> gate 7.9e-4        (the condition on the yardstick: worst < 1e-4)
    equal sizes:   float32 oracle worst 7.00e-4 -> gate 1.1e-2        (worst < 2e-3)
    homogeneity:   float32 oracle worst 4.80e-7 -> gate 7.7e-6
    momentum:      float32 oracle worst 3.87e-7 -> gate 6.2e-6
Shapes (N left points, M right points): 512 threads own up to 8 points of either cloud each, in 1 .. 4 register pairs; both
clouds are staged whole in LDS, (N + M) 16 bytes of it: (1025, 2049) / (2049, 1025) reach two and three pairs with a ragged
last one, (4096, 3) / (3, 3073) the fourth pair on either side, (2048, 2048) the model's size, (4096, 4095) all 128 KB.
"""
import functools

import numpy as np
import pytest
import torch

import pc3d_emd_grad_oracle as GO
from support.pc import DEV, _PC, put

pytestmark = pytest.mark.gpu
# (N, M, B)
COST_CASES = [(1, 1, 2), (5, 7, 3), (64, 64, 3), (257, 300, 2), (1025, 2049, 1), (2049, 1025, 1), (4096, 3, 2),
              (3, 3073, 1), (2048, 2048, 2), (4096, 4095, 1)]
UNEQUAL = [(5, 7), (48, 80), (257, 300), (300, 513), (1025, 2049), (2049, 1025), (4096, 3), (3, 3073)]
EQUAL = [(1, 1), (64, 64), (257, 257), (1030, 1030), (2048, 2048)]
WANTS = [(False, False), (True, False), (False, True), (True, True)]


@functools.lru_cache(maxsize=None)
def _clouds(B, N, M, seed=None):
    """float32 numpy inputs (never modified by a test): left [B, N, 3], right [B, M, 3]"""
    rng = np.random.default_rng(B * 1000003 + N * 101 + M * 10007 if seed is None else seed)
    left = (rng.random((B, N, 3)) - 0.5).astype(np.float32)
    right = (rng.random((B, M, 3)) - 0.5).astype(np.float32)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


@functools.lru_cache(maxsize=None)
def _oracle(N, M, dtype=np.float64):
    """(cost, dleft, dright) of the one pair _clouds(1, N, M), unnormalised, computed once"""
    left, right = _clouds(1, N, M)
    cost, dl, dr = GO.emd_grad(left[0], right[0], normalize=False, dtype=dtype)
    dl.setflags(write=False)
    dr.setflags(write=False)
    return cost, dl, dr


def _rel(g, g64):
    return float(np.abs(np.asarray(g, dtype=np.float64) - g64).max() / np.abs(g64).max())


@functools.lru_cache(maxsize=None)
def _gate(cls):
    """16 x the float32 oracle's worst max|g - g64| / max|g64| over the class's cases and both sides"""
    cases, bound = (UNEQUAL, 1e-4) if cls == "unequal" else (EQUAL, 2e-3)
    worst = 0.0
    for N, M in cases:
        _, l64, r64 = _oracle(N, M)
        _, l32, r32 = _oracle(N, M, np.float32)
        worst = max(worst, _rel(l32, l64), _rel(r32, r64))
    assert 0 < worst < bound, worst
    print("gradient, %s sizes: float32 oracle against float64 oracle, worst %.3e -> gate %.3e" % (cls, worst, 16 * worst))
    return 16 * worst


@functools.lru_cache(maxsize=None)
def _identity_gates():
    """(homogeneity, momentum): 16 x the float32 oracle's worst defect over the gradient cases"""
    h = p = 0.0
    for N, M in UNEQUAL + EQUAL:
        left, right = _clouds(1, N, M)
        c32, l32, r32 = _oracle(N, M, np.float32)
        h = max(h, GO.homogeneity_defect(left[0], right[0], c32, l32, r32))
        p = max(p, GO.momentum_defect(l32, r32))
    assert 0 < h < 1e-5 and 0 < p < 1e-5, (h, p)
    print("float32 oracle: homogeneity worst %.3e -> gate %.3e, momentum worst %.3e -> gate %.3e" % (h, 16 * h, p, 16 * p))
    return 16 * h, 16 * p


def _np(t):
    return t.double().cpu().numpy()


# ------------------------------------------------------------------------------------------------ the cost
@pytest.mark.parametrize("N,M,B", COST_CASES)
def test_cost_is_the_matrix_entry_bit_for_bit(N, M, B):
    """cost[b] = emd_matrix(sample = right_b, ref = left_b)[0, 0], whichever gradients are asked for, normalised or not;
    the gradients asked for do not depend on the other side being asked for either"""
    PC = _PC()
    left, right = (put(a) for a in _clouds(B, N, M))
    for normalize in (False, True):
        want = torch.stack([PC.emd_matrix(right[b:b + 1], left[b:b + 1], normalize=normalize)[0, 0] for b in range(B)])
        got = {w: PC.emd_loss_fwd(left, right, w[0], w[1], normalize) for w in WANTS}
        for (wl, wr), (cost, dl, dr) in got.items():
            assert cost.shape == (B,) and cost.dtype == torch.float32
            assert torch.equal(cost, want), (wl, wr, normalize)
            assert (dl is None) == (not wl) and (dr is None) == (not wr)
            if wl:
                assert dl.shape == (B, N, 3) and dl.is_contiguous() and torch.equal(dl, got[(True, True)][1])
            if wr:
                assert dr.shape == (B, M, 3) and dr.is_contiguous() and torch.equal(dr, got[(True, True)][2])


# ------------------------------------------------------------------------------------------------ the gradients
@pytest.mark.parametrize("N,M,cls", [(n, m, "unequal") for n, m in UNEQUAL] + [(n, m, "equal") for n, m in EQUAL])
def test_gradients_against_the_float64_oracle(N, M, cls):
    """both gradients within the class's gate of the float64 oracle; the homogeneity and momentum identities, evaluated in
    float64 on the host from the kernel's own outputs, within theirs"""
    PC = _PC()
    left, right = _clouds(1, N, M)
    cost, dl, dr = PC.emd_loss_fwd(put(left), put(right), True, True)
    cost, dl, dr = float(cost[0]), _np(dl[0]), _np(dr[0])
    assert np.isfinite(dl).all() and np.isfinite(dr).all()
    c64, l64, r64 = _oracle(N, M)
    el, er = _rel(dl, l64), _rel(dr, r64)
    hg, pg = _identity_gates()
    h, p = GO.homogeneity_defect(left[0], right[0], cost, dl, dr), GO.momentum_defect(dl, dr)
    print("emd_loss N=%d M=%d: dleft %.3e dright %.3e (gate %.3e); homogeneity %.3e (gate %.3e); momentum %.3e (gate %.3e)"
          % (N, M, el, er, _gate(cls), h, hg, p, pg))
    assert el <= _gate(cls) and er <= _gate(cls)
    assert h <= hg
    assert p <= pg


# ------------------------------------------------------------------------------------------------ coincident points
@functools.lru_cache(maxsize=None)
def _coincident(how, n):
    base = _clouds(1, n, n, 77)[0][0]
    rng = np.random.default_rng(n)
    if how == "itself":
        left, right = base, base
    elif how == "permuted":
        left, right = base, base[rng.permutation(n)]
    else:  # every point of the left cloud twice, the right cloud holding each of them once among other points
        h = n // 2
        left = np.concatenate([base[:h], base[:h]])[rng.permutation(2 * h)]
        right = np.concatenate([base[:h], _clouds(1, n, n, 78)[1][0][:h - 20]])[rng.permutation(2 * h - 20)]
    left, right = np.ascontiguousarray(left[None]), np.ascontiguousarray(right[None])
    return left, right, GO.emd_grad(left[0], right[0])


@pytest.mark.parametrize("how,n", [("itself", 64), ("permuted", 64), ("itself", 300), ("permuted", 300), ("duplicated", 300)])
def test_coincident_points(how, n):
    """pairs with d2 == 0 contribute zero: every element finite, and within the equal-size gate of the float64 oracle as
    an ABSOLUTE value (unit vectors bound the scale).  Against themselves 64 points have max|g64| = 1.6e-5, where a
    relative measure means nothing; 300 points share more mass with their neighbours (max|g64| 0.12)."""
    PC = _PC()
    left, right, (c64, l64, r64) = _coincident(how, n)
    cost, dl, dr = PC.emd_loss_fwd(put(left), put(right), True, True)
    assert bool(torch.isfinite(cost).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dr).all())
    el, er = float(np.abs(_np(dl[0]) - l64).max()), float(np.abs(_np(dr[0]) - r64).max())
    print("coincident (%s, %d): |dleft - g64| %.3e, |dright - g64| %.3e (gate %.3e), max|g64| %.3e"
          % (how, n, el, er, _gate("equal"), max(np.abs(l64).max(), np.abs(r64).max())))
    assert el <= _gate("equal") and er <= _gate("equal")


# ------------------------------------------------------------------------------------------------ NaN, inf
@pytest.mark.parametrize("normalize", [False, True])
def test_non_finite_coordinates_stay_in_their_pair(normalize):
    PC = _PC()
    B, N, M = 5, 33, 70
    left, right = (np.array(a) for a in _clouds(B, N, M))
    clean = PC.emd_loss_fwd(put(left), put(right), True, True, normalize)
    assert all(bool(torch.isfinite(t).all()) for t in clean)
    left[1, 17, 2] = np.nan
    right[3, 69, 0] = np.inf
    got = PC.emd_loss_fwd(put(left), put(right), True, True, normalize)
    bad = torch.tensor([False, True, False, True, False], device=DEV)
    for t, c in zip(got, clean):
        assert bool(torch.isnan(t[bad]).all())
        assert torch.equal(t[~bad], c[~bad])
    only_r = PC.emd_loss_fwd(put(left), put(right), False, True, normalize)
    assert only_r[1] is None and torch.equal(torch.isnan(only_r[2]), torch.isnan(got[2]))


# ------------------------------------------------------------------------------------------------ bit identity
def _all_equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("B,N,M", [(3, 33, 70), (1, 2049, 1025)])
def test_two_runs_are_bit_identical(B, N, M):
    PC = _PC()
    left, right = (put(a) for a in _clouds(B, N, M))
    for normalize in (False, True):
        assert _all_equal(PC.emd_loss_fwd(left, right, True, True, normalize),
                          PC.emd_loss_fwd(left, right, True, True, normalize))


def _transposed_view(a):
    """the [B, N, 3] view of [B, 3, N] storage: the decoder's output .permute(0, 2, 1)"""
    v = put(a).permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert not v.is_contiguous() and v.stride(2) == a.shape[1]
    return v


@pytest.mark.parametrize("B,N,M", [(3, 33, 70), (2, 1030, 300)])
def test_layouts_change_no_bit(B, N, M):
    PC = _PC()
    left, right = _clouds(B, N, M)
    base = PC.emd_loss_fwd(put(left), put(right), True, True)
    for name, l, r in (("left transposed", _transposed_view(left), put(right)),
                       ("right transposed", put(left), _transposed_view(right)),
                       ("both transposed", _transposed_view(left), _transposed_view(right))):
        got = PC.emd_loss_fwd(l, r, True, True)
        assert _all_equal(got, base), name
        assert got[1].is_contiguous() and got[2].is_contiguous()


def _count_launches(monkeypatch, PC):
    calls = []
    real = PC._lib.call
    monkeypatch.setattr(PC._lib, "call", lambda name, *a: (calls.append((name, a)), real(name, *a))[1])
    return calls


def _launches(calls):
    return sum(1 for name, _ in calls if name == "sivae_emd_loss")


def test_slabs_change_no_bit(monkeypatch):
    """(4, 33, 70) in one launch, in two launches of two pairs and in four of one"""
    PC = _PC()
    B, N, M = 4, 33, 70
    left, right = (put(a) for a in _clouds(B, N, M))
    calls = _count_launches(monkeypatch, PC)
    whole = PC.emd_loss_fwd(left, right, True, True)
    assert _launches(calls) == 1
    for pairs, launches in ((2, 2), (1, 4)):
        del calls[:]
        monkeypatch.setattr(PC, "EMD_LOSS_POINT_PAIRS_PER_LAUNCH", pairs * N * M)
        assert _all_equal(PC.emd_loss_fwd(left, right, True, True), whole)
        assert _launches(calls) == launches


def test_more_pairs_than_blocks_against_slabs(monkeypatch):
    """1030 pairs of 16-point clouds on a grid capped at 1024 blocks (six blocks walk two pairs) against the same pairs in
    slabs of 515 (one pair a block)"""
    PC = _PC()
    B, N, M = 1030, 16, 16
    left, right = (put(a) for a in _clouds(B, N, M))
    calls = _count_launches(monkeypatch, PC)
    whole = PC.emd_loss_fwd(left, right, True, True)
    assert _launches(calls) == 1
    monkeypatch.setattr(PC, "EMD_LOSS_POINT_PAIRS_PER_LAUNCH", 515 * N * M)
    slabs = PC.emd_loss_fwd(left, right, True, True)
    assert _launches(calls) == 3
    assert _all_equal(slabs, whole)
    assert all(bool(torch.isfinite(t).all()) for t in whole)


# ------------------------------------------------------------------------------------------------ autograd
def test_autograd_scales_the_unit_gradients(monkeypatch):
    PC = _PC()
    B, N, M = 3, 48, 80
    left, right = (put(a) for a in _clouds(B, N, M))
    cost, dl, dr = PC.emd_loss_fwd(left, right, True, True)
    w = torch.tensor([0.25, -3.0, 1.7], device=DEV)
    p, g = left.clone().requires_grad_(True), right.clone().requires_grad_(True)
    out = PC.emd_distance(p, g)
    assert torch.equal(out.detach(), cost) and out.requires_grad
    (out * w).sum().backward()
    assert torch.equal(p.grad, w.view(-1, 1, 1) * dl) and torch.equal(g.grad, w.view(-1, 1, 1) * dr)
    # an input that does not require grad gets None, and the kernel is not asked for its gradient
    calls = _count_launches(monkeypatch, PC)
    for need_p, need_g in ((False, True), (True, False)):
        del calls[:]
        p, g = left.clone().requires_grad_(need_p), right.clone().requires_grad_(need_g)
        (PC.emd_distance(p, g) * w).sum().backward()
        asked = [a for name, a in calls if name == "sivae_emd_loss"]
        assert len(asked) == 1
        assert (asked[0][9] is None) == (not need_p) and (asked[0][10] is None) == (not need_g)
        assert (p.grad is None) == (not need_p) and (g.grad is None) == (not need_g)
        if need_g:
            assert torch.equal(g.grad, w.view(-1, 1, 1) * dr)
        else:
            assert torch.equal(p.grad, w.view(-1, 1, 1) * dl)
    del calls[:]
    assert not PC.emd_distance(left, right).requires_grad
    assert [a[9:11] for name, a in calls if name == "sivae_emd_loss"] == [(None, None)]


def test_autograd_normalize_and_double_backward():
    """normalize=True divides the cost and both gradients by max(N, M) = 80: one rounding each, 2^-23 of the value at the
    most (the cost's division is taken in float64 before it is rounded)"""
    PC = _PC()
    B, N, M = 3, 48, 80
    left, right = (put(a) for a in _clouds(B, N, M))
    cost, dl, dr = PC.emd_loss_fwd(left, right, True, True)
    p, g = left.clone().requires_grad_(True), right.clone().requires_grad_(True)
    out = PC.emd_distance(p, g, normalize=True)
    out.sum().backward()
    for got, unit in ((out.detach(), cost), (p.grad, dl), (g.grad, dr)):
        want = unit.double() / 80.0
        assert bool(((got.double() - want).abs() <= 2.0 ** -23 * want.abs()).all())
    p, g = left.clone().requires_grad_(True), right.clone().requires_grad_(True)
    # (upstream weights that require grad: the backward's result is then part of a graph, the one that must refuse)
    w = torch.ones(B, device=DEV, requires_grad=True)
    gp, = torch.autograd.grad((PC.emd_distance(p, g) * w).sum(), p, create_graph=True)
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gp.sum().backward()


def test_drop_in_module_on_the_training_loop_views():
    """EMD()(x.permute(0, 2, 1) + 0.5, decoder(z).permute(0, 2, 1) + 0.5), as the reference's loop calls its loss: the
    module's value is emd_distance's, and the decoder's weight gradients are finite and not all zero"""
    import pc3d_oracle as O
    import soft_intro_vae_3d.models.vae as V
    from soft_intro_vae_3d.losses.earth_mover_distance import EMD
    PC = _PC()
    torch.manual_seed(5)
    z, B = 16, 2
    dec = V.Decoder(O.config(z)).to(DEV).train()
    x = put(np.ascontiguousarray(_clouds(B, 2048, 2048, 11)[0].transpose(0, 2, 1)))   # [B, 3, 2048]
    rec = dec(torch.randn(B, z, device=DEV))
    assert rec.shape == (B, 3, 2048)
    loss = EMD()(x.permute(0, 2, 1) + 0.5, rec.permute(0, 2, 1) + 0.5)
    assert loss.shape == (B,) and bool(torch.isfinite(loss).all()) and bool((loss > 0).all())
    assert torch.equal(loss.detach(), PC.emd_loss_fwd(x.permute(0, 2, 1) + 0.5, rec.detach().permute(0, 2, 1) + 0.5,
                                                      False, False)[0])
    (loss.mean() / (3 * 2048)).backward()
    grads = [q.grad for q in dec.parameters()]
    assert all(t is not None and bool(torch.isfinite(t).all()) for t in grads)
    assert all(float(t.abs().max()) > 0 for t in grads if t.dim() == 2)
    assert x.grad is None


# ------------------------------------------------------------------------------------------------ guarded
@pytest.mark.parametrize("B,N,M", [(2, 257, 300), (1, 2049, 1025)])
def test_guarded(B, N, M):
    """on guarded, poisoned outputs and an exact workspace (no size uses one: a one-byte view of the guard): nothing
    written outside a tensor, no element left at the poison value (finite inputs: an unwritten element reads as NaN), the
    unguarded results"""
    from sivae_hip import ops, pointcloud
    from support.guard import describe, guarded
    left, right = (put(a) for a in _clouds(B, N, M))
    base = pointcloud.emd_loss_fwd(left, right, True, True)
    for mods in ((pointcloud,), (pointcloud, ops)):  # (pointcloud's torch; `workspace` is ops' and needs ops in the list)
        with guarded(*mods) as g:
            got = pointcloud.emd_loss_fwd(left, right, True, True)
            damage = g.verify()
            assert not damage, "guard damage:\n%s" % describe(damage)
        for t, b in zip(got, base):
            assert bool(torch.isfinite(t).all()) and torch.equal(t, b)
