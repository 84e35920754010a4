"""GPU checks of the fused last encoder stage, sivae_relu_bn_max_fwd / _bwd (csrc/pointcloud.hip) and
sivae_hip.pointcloud.relu_bn_max, against (a) the composition it replaces — relu_bn_stats, relu_bn_apply, max_points_fwd,
max_points_bwd, relu_bn_bwd on the same device — and (b) the float64 restatement tests/pc3d_oracle.py::relu_bn on the CPU.

Shapes (B, C, N) and what each covers
  (3, 5, 100)    16-byte path; 15 rows, so the last block of 4 waves is partial; lanes 25-63 hold no element
  (2, 3, 33)     scalar path (a lane owns ONE index: no same-lane duplicate exists at this length)
  (1, 7, 1)      one point per row
  (2, 6, 260)    16-byte path; lane 0 makes two trips, the others one
  (2, 5, 2048)   the workload's row length at a tiny batch
  (3, 5, 132)*   `a` one element behind an aligned start: the scalar route on an N % 4 == 0 shape

Every shape: channel 0 has a <= 0 everywhere (variance 0, all y equal), gamma[1] < 0 (the max of y sits where relu(a) is
smallest: every a <= 0 of the row ties), gamma[2] == 0 exactly (all y equal beta), exact zeros in a.  Where C > 3 and N
allows, the last row has its maximum at two indices of one lane and at one index of another lane (16-byte path: a lane
owns 4 i .. 4 i + 3; scalar path: i and i + 64).

Forward values and indices are compared with torch.equal: the fused kernel forms y with the function relu_bn_apply_kernel
stores (one multiply for gamma invstd, one FMA for the shift, one FMA per element), so nothing may differ.
Element-wise gate: |x - ref| <= 1e-4 |ref| + 1e-5 max|ref| (support.pc.viol <= 1).  dgamma / dbeta against
fp64: relative L2 <= max(4 e32, 1e-5), e32 the error of the fp32 run of the same restatement on the CPU.
"""
import functools

import pytest
import torch

import pc3d_oracle as O
from support.pc import DEV, _BN, _PC, _grad_report, _load, put, viol

pytestmark = pytest.mark.gpu
CASES = [(3, 5, 100, False), (2, 3, 33, False), (1, 7, 1, False), (2, 6, 260, False), (2, 5, 2048, False),
         (3, 5, 132, True)]
EPS = 1e-5


def _dup_indices(N, vec):
    """two indices of one lane and one of another lane, or None where the row is too short"""
    if vec:
        return (4, 5, 40) if N > 40 else None
    return (3, 67, 10) if N > 67 else None


@functools.lru_cache(maxsize=None)
def _case(B, C, N, misaligned):
    """-> dict of the CPU inputs (never modified by a test) and the fp64 forward reference"""
    g = torch.Generator().manual_seed(B * 1000 + C * 10 + N)
    a = torch.randn(B, C, N, generator=g)
    a[torch.rand(B, C, N, generator=g) < 0.1] = 0.0
    a[:, 0] = -a[:, 0].abs()                      # dead everywhere (zeros included): variance 0
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    gamma[1] = -gamma[1]
    gamma[2] = 0.0
    dup = _dup_indices(N, N % 4 == 0 and not misaligned) if C > 3 else None
    if dup is not None:
        for i in dup:
            a[B - 1, C - 1, i] = 9.0
    gy = torch.randn(B, C, generator=g)
    gy[0, C - 1] = 0.0                            # exact zeros in the upstream gradient
    gy[B - 1, 0] = 0.0
    rm0, rv0 = torch.rand(C, generator=g) * 0.2 - 0.1, torch.rand(C, generator=g) + 0.5
    y64, rm64, rv64 = O.relu_bn(a.double(), gamma.double(), beta.double(), rm0.double(), rv0.double(), True)
    ye64, _, _ = O.relu_bn(a.double(), gamma.double(), beta.double(), rm0.double(), rv0.double(), False)
    return dict(a=a, gamma=gamma, beta=beta, gy=gy, rm0=rm0, rv0=rv0, dup=dup, vals64=y64.max(dim=2)[0],
                vals64_eval=ye64.max(dim=2)[0])


def _device(case, misaligned):
    PC = _PC()
    a = put(case["a"], misaligned)
    gamma, beta = case["gamma"].to(DEV), case["beta"].to(DEV)
    mean, invstd = PC.relu_bn_stats(a)
    return a, gamma, beta, mean, invstd


@pytest.mark.parametrize("B,C,N,misaligned", CASES)
def test_forward_equals_the_composition_bit_for_bit(B, C, N, misaligned):
    PC = _PC()
    case = _case(B, C, N, misaligned)
    a, gamma, beta, mean, invstd = _device(case, misaligned)
    rm, rv = case["rm0"].to(DEV), case["rv0"].to(DEV)
    for mode, (m, s) in (("train", (mean, invstd)), ("eval", (rm, torch.rsqrt(rv + EPS)))):
        v0, i0 = PC.max_points_fwd(PC.relu_bn_apply(a, m, s, gamma, beta))
        v1, i1 = PC.relu_bn_max_fwd(a, m, s, gamma, beta)
        assert v1.shape == (B, C) and i1.shape == (B, C) and i1.dtype == torch.int32
        assert torch.equal(v1, v0), (mode, float((v1 - v0).abs().max()))
        assert torch.equal(i1, i0), mode
        v2, i2 = PC.relu_bn_max_fwd(a, m, s, gamma, beta)  # determinism
        assert torch.equal(v2, v1) and torch.equal(i2, i1)
    if case["dup"] is not None:
        assert int(i1[B - 1, C - 1]) == min(case["dup"])
    assert bool((i1[:, 0] == 0).all()) and bool((i1[:, 2] == 0).all())  # all-equal rows: index 0
    # against fp64
    v_t, _ = PC.relu_bn_max_fwd(a, mean, invstd, gamma, beta)
    figs = dict(train=viol(v_t, case["vals64"]), eval=viol(v1, case["vals64_eval"]))
    print("relu_bn_max fwd [%d, %d, %d]: violation ratios vs fp64 %s" % (B, C, N, {k: "%.3f" % v for k, v in figs.items()}))
    assert all(v <= 1.0 for v in figs.values()), figs


@pytest.mark.parametrize("B,C,N,misaligned", CASES)
def test_autograd_function_equals_the_composition(B, C, N, misaligned):
    """relu_bn_max against max_points(relu_bn(...)): outputs and the three BatchNorm buffers, training and eval mode"""
    PC = _PC()
    from sivae_hip import functional as SF
    case = _case(B, C, N, misaligned)
    gamma, beta = case["gamma"].to(DEV), case["beta"].to(DEV)
    for training in (True, False):
        bn0, bn1 = _BN(C, training, 5), _BN(C, training, 5)
        out0 = PC.max_points(PC.relu_bn(put(case["a"], misaligned), gamma, beta, SF.BNState(bn0)))
        out1 = PC.relu_bn_max(put(case["a"], misaligned), gamma, beta, SF.BNState(bn1))
        assert torch.equal(out1, out0)
        assert torch.equal(bn1.running_mean, bn0.running_mean) and torch.equal(bn1.running_var, bn0.running_var)
        assert int(bn1.num_batches_tracked) == int(bn0.num_batches_tracked) == (4 if training else 3)


def _fp64_backward(case, arg, dtype):
    """autograd of the restatement in `dtype`, the max taken as a gather at the kernel's indices (by value, never by
    identity: ties make nothing ambiguous) -> (da, dgamma, dbeta)"""
    # (clones: .to(float32) of a float32 tensor is the tensor itself, and the case is shared)
    a = case["a"].clone().to(dtype).requires_grad_(True)
    ga, be = case["gamma"].clone().to(dtype).requires_grad_(True), case["beta"].clone().to(dtype).requires_grad_(True)
    y, _, _ = O.relu_bn(a, ga, be, case["rm0"].to(dtype), case["rv0"].to(dtype), True)
    out = y.gather(2, arg.cpu().long()[:, :, None])[:, :, 0]
    (out * case["gy"].to(dtype)).sum().backward()
    return a.grad, ga.grad, be.grad


@pytest.mark.parametrize("B,C,N,misaligned", CASES)
def test_backward(B, C, N, misaligned):
    PC = _PC()
    case = _case(B, C, N, misaligned)
    a, gamma, beta, mean, invstd = _device(case, misaligned)
    gy = case["gy"].to(DEV)
    vals, arg = PC.relu_bn_max_fwd(a, mean, invstd, gamma, beta)
    da, dgamma, dbeta = PC.relu_bn_max_bwd(gy, arg, a, mean, invstd, gamma)
    assert da.shape == (B, C, N) and dgamma.shape == (C,) and dbeta.shape == (C,)
    # fp64, the kernel's own indices
    da64, dg64, db64 = _fp64_backward(case, arg, torch.float64)
    _, dg32, db32 = _fp64_backward(case, arg, torch.float32)
    v_da = viol(da, da64)
    print("relu_bn_max bwd [%d, %d, %d]: da %.3f of the element-wise criterion" % (B, C, N, v_da))
    assert v_da <= 1.0
    for name, got, ref, r32 in (("dgamma", dgamma, dg64, dg32), ("dbeta", dbeta, db64, db32)):
        e_gpu, e32 = O.rel_l2(got, ref), O.rel_l2(r32, ref)
        print("relu_bn_max bwd [%d, %d, %d]: %s gpu %.3e  cpu-fp32 %.3e  gate %.3e" % (B, C, N, name, e_gpu, e32,
                                                                                     max(4 * e32, 1e-5)))
        assert e_gpu <= max(4 * e32, 1e-5), (name, e_gpu, e32)
    # the composition's backward on the same g and arg
    da_c, dg_c, db_c = PC.relu_bn_bwd(PC.max_points_bwd(gy, arg, N), a, mean, invstd, gamma)
    figs = dict(da=viol(da, da_c), dgamma=viol(dgamma, dg_c), dbeta=viol(dbeta, db_c))
    print("relu_bn_max bwd [%d, %d, %d]: violation ratios vs the composition %s"
          % (B, C, N, {k: "%.3f" % v for k, v in figs.items()}))
    assert all(v <= 1.0 for v in figs.values()), figs
    # ReLU's gate: a row whose maximum sits on an element with a <= 0 gets exactly 0 there (and everywhere a <= 0)
    at_arg = a.gather(2, arg.long()[:, :, None])[:, :, 0]
    closed = at_arg <= 0
    assert bool(closed.any())  # (channel 0, and the negative-gamma channel's rows)
    assert bool((da.gather(2, arg.long()[:, :, None])[:, :, 0][closed] == 0).all())
    assert bool((da[a <= 0] == 0).all())
    # determinism
    da2, dgamma2, dbeta2 = PC.relu_bn_max_bwd(gy, arg, a, mean, invstd, gamma)
    assert torch.equal(da2, da) and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)
    # through autograd
    from sivae_hip import functional as SF
    ad = put(case["a"], misaligned).requires_grad_(True)
    gd, bd = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = PC.relu_bn_max(ad, gd, bd, SF.BNState(_BN(C, True, 5)))
    assert torch.equal(out, vals)
    out.backward(gy)
    assert torch.equal(ad.grad, da) and torch.equal(gd.grad, dgamma) and torch.equal(bd.grad, dbeta)


@pytest.mark.parametrize("N", [100, 33])
def test_nan(N):
    """one NaN in a row: with statistics taken before it was planted only that row's value is NaN and arg is its index;
    with the NaN in the statistics the whole channel is NaN (index 0 elsewhere) — mask, indices and the finite values
    are the composition's in both"""
    PC = _PC()
    B, C = 2, 4
    g = torch.Generator().manual_seed(N)
    a = torch.randn(B, C, N, generator=g)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) - 0.5).to(DEV)
    clean = a.to(DEV)
    mean, invstd = PC.relu_bn_stats(clean)
    k = N - 3
    a[1, 2, k] = float("nan")
    a[0, 1, 7] = a[0, 1, 20] = float("nan")      # two NaNs in different lanes: the lower index
    ad = a.to(DEV)
    vals, arg = PC.relu_bn_max_fwd(ad, mean, invstd, gamma, beta)
    want = torch.zeros(B, C, dtype=torch.bool)
    want[1, 2] = want[0, 1] = True
    assert torch.equal(vals.isnan().cpu(), want)
    assert int(arg[1, 2]) == k and int(arg[0, 1]) == 7
    v0, i0 = PC.max_points_fwd(PC.relu_bn_apply(ad, mean, invstd, gamma, beta))
    assert torch.equal(vals.isnan(), v0.isnan()) and torch.equal(arg, i0)
    assert torch.equal(vals[~vals.isnan()], v0[~v0.isnan()])
    # the NaN inside the statistics
    mean_n, invstd_n = PC.relu_bn_stats(ad)
    vals, arg = PC.relu_bn_max_fwd(ad, mean_n, invstd_n, gamma, beta)
    want = torch.zeros(B, C, dtype=torch.bool)
    want[:, 1] = want[:, 2] = True
    assert torch.equal(vals.isnan().cpu(), want)
    assert arg[:, 1].tolist() == [0, 0] and arg[:, 2].tolist() == [0, 0]
    v0, i0 = PC.max_points_fwd(PC.relu_bn_apply(ad, mean_n, invstd_n, gamma, beta))
    assert torch.equal(vals.isnan(), v0.isnan()) and torch.equal(arg, i0)
    assert torch.equal(vals[~vals.isnan()], v0[~v0.isnan()])


@pytest.mark.parametrize("B,C,N", [(3, 5, 100), (2, 3, 33)])
def test_guarded(B, C, N):
    """forward and backward on guarded, poisoned outputs: nothing written outside a tensor, no output element left at the
    poison value (0xFF bytes: NaN as fp32, -1 as int32), the unguarded results"""
    from sivae_hip import ops, pointcloud
    from support.guard import describe, guarded
    PC = pointcloud
    case = _case(B, C, N, False)
    a, gamma, beta, mean, invstd = _device(case, False)
    gy = case["gy"].to(DEV)
    vals0, arg0 = PC.relu_bn_max_fwd(a, mean, invstd, gamma, beta)
    da0, dgamma0, dbeta0 = PC.relu_bn_max_bwd(gy, arg0, a, mean, invstd, gamma)
    with guarded(pointcloud, ops) as g:
        mean_g, invstd_g = PC.relu_bn_stats(a)
        vals, arg = PC.relu_bn_max_fwd(a, mean_g, invstd_g, gamma, beta)
        da, dgamma, dbeta = PC.relu_bn_max_bwd(gy, arg, a, mean_g, invstd_g, gamma)
        damage = g.verify()
        assert not damage, "guard damage:\n%s" % describe(damage)
    for t in (vals, da, dgamma, dbeta):
        assert bool(torch.isfinite(t).all())
    assert int(arg.min()) >= 0 and int(arg.max()) < N
    assert torch.equal(mean_g, mean) and torch.equal(invstd_g, invstd)
    assert torch.equal(vals, vals0) and torch.equal(arg, arg0)
    assert torch.equal(da, da0) and torch.equal(dgamma, dgamma0) and torch.equal(dbeta, dbeta0)


def test_encoder_with_and_without_the_fused_stage(monkeypatch):
    """V.Encoder at B = 3, N = 100, z = 8, weights by the recipe: the switch changes no output bit and no buffer bit; the
    fused run's parameter gradients pass test_encoder's gate against the fp64 restatement"""
    import soft_intro_vae_3d.models.vae as V
    PC = _PC()
    B, N, z = 3, 100, 8
    specs = O.encoder_specs(z)
    g = torch.Generator().manual_seed(B + N)
    x = torch.rand(B, 3, N, generator=g) - 0.5
    r1, r2 = torch.randn(B, z, generator=g), torch.randn(B, z, generator=g)
    sds = {}
    for dt in (torch.float64, torch.float32):
        sd = O.leaves(O.recipe_state_dict(specs, 7, dt))
        mu, lv = O.encoder(sd, x.to(dt), True)
        ((mu * r1.to(dt)).sum() + (lv * r2.to(dt)).sum()).backward()
        sds[dt] = sd
    runs = {}
    for fused in (False, True):
        monkeypatch.setattr(PC, "RELU_BN_MAX", fused)
        enc = _load(V.Encoder(O.config(z)), sds[torch.float64]).train()
        mu, lv = enc(x.to(DEV))
        ((mu * r1.to(DEV)).sum() + (lv * r2.to(DEV)).sum()).backward()
        runs[fused] = (enc, mu, lv)
    (enc0, mu0, lv0), (enc1, mu1, lv1) = runs[False], runs[True]
    assert torch.equal(mu1, mu0) and torch.equal(lv1, lv0)
    buffers0, buffers1 = dict(enc0.named_buffers()), dict(enc1.named_buffers())
    assert len(buffers1) == 15
    for k, v in buffers1.items():
        assert torch.equal(v, buffers0[k]), k
    assert int(buffers1["conv.14.num_batches_tracked"]) == 1
    _grad_report("encoder fused[%d,%d]" % (B, N), enc1.named_parameters(), sds[torch.float64], sds[torch.float32])
    # eval mode: forward works, the backward is refused
    from sivae_hip import functional as SF
    case = _case(3, 5, 100, False)
    ad = case["a"].to(DEV).requires_grad_(True)
    out = PC.relu_bn_max(ad, case["gamma"].to(DEV), case["beta"].to(DEV), SF.BNState(_BN(5, False, 6)))
    with pytest.raises(RuntimeError, match="eval-mode BatchNorm"):
        out.sum().backward()
