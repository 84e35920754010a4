"""GPU checks of the 3-D point-cloud slice (csrc/pointcloud.hip, sivae_hip/pointcloud.py, soft_intro_vae_3d/) against
the float64 restatement of tests/pc3d_oracle.py computed in the test.

Chamfer inputs: `torch.rand(B, N, 3)` then `torch.rand(B, M, 3)` drawn as DOUBLES from one `torch.Generator` seeded per
case and rounded to float32 (the draw that reproduces the nearest / second-nearest gaps 1.7e-2 / 6.8e-3 / 2.2e-3 of
the first three cases); the reference is evaluated on the rounded values the kernel sees.

Tolerances
  Chamfer loss 1e-5 relative: direct-form terms carry a few ulp each, the block-wise sums about (N / 256 + 8) 2^-24.
  Chamfer indices by DISTANCE (|P_j - G_idx|^2 within 1e-5 of the fp64 minimum), never by identity.
  Element-wise "1e-4 relative": |a - b| <= 1e-4 |b| + 1e-5 max|b| (the project's criterion, test_e2e_gpu._allclose_viol).
  Parameter gradients: relative L2 against fp64, gate max(4 e32, 1e-5) per tensor with e32 the error of the fp32 run of
  the SAME restatement on the CPU (the factor 4: MFMA K-chunk order and split reductions accumulate differently).
"""
import pytest
import torch

import pc3d_oracle as O
from support.pc import DEV, _BN, _PC, _chamfer_case, _check_indices_by_distance, _grad_report, _load, viol

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ Chamfer
CHAMFER_CASES = [(2, 64, 64, 2), (3, 70, 33, 2), (2, 257, 130, 3), (2, 2048, 2048, 0), (1, 1, 5, 0)]


@pytest.mark.parametrize("B,N,M,seed", CHAMFER_CASES)
def test_chamfer_forward(B, N, M, seed):
    PC = _PC()
    preds, gts, P, want = _chamfer_case(B, N, M, seed)
    loss, idx_p, idx_g = PC.chamfer_fwd(preds.to(DEV), gts.to(DEV))
    assert loss.shape == (B,) and idx_p.shape == (B, M) and idx_g.shape == (B, N) and idx_p.dtype == torch.int32
    err = float(((loss.double().cpu() - want).abs() / want).max())
    print("chamfer fwd (%d, %d, %d): rel err %.3e" % (B, N, M, err))
    assert err <= 1e-5
    _check_indices_by_distance(P, idx_p, idx_g)
    # the module, on the training loop's non-contiguous views
    from soft_intro_vae_3d.losses.chamfer_loss import ChamferLoss
    v = ChamferLoss()(preds.to(DEV).permute(0, 2, 1).contiguous().permute(0, 2, 1), gts.to(DEV))
    assert torch.equal(v, loss)


@pytest.mark.parametrize("B,N,M,seed", CHAMFER_CASES)
def test_chamfer_backward_formula_with_kernel_indices(B, N, M, seed):
    """dP only, dG only and both against the analytic formula in fp64 evaluated with the kernel's OWN indices"""
    PC = _PC()
    preds, gts, P, _ = _chamfer_case(B, N, M, seed)
    p, q = preds.to(DEV), gts.to(DEV)
    loss, idx_p, idx_g = PC.chamfer_fwd(p, q)
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


@pytest.mark.parametrize("B,N,M,seed", CHAMFER_CASES[:3])
def test_chamfer_backward_against_autograd(B, N, M, seed):
    """torch autograd of the fp64 restatement; meaningful because no point's nearest neighbour is nearly tied: the
    relative gap between nearest and second-nearest distance is re-asserted for EVERY point first"""
    PC = _PC()
    preds, gts, P, _ = _chamfer_case(B, N, M, seed)
    for dim in (1, 2):
        s = P.sort(dim=dim)[0]
        d1, d2 = s.select(dim, 0), s.select(dim, 1)
        gap = float(((d2 - d1) / d2).min())
        print("gap (%d, %d, %d) dim %d: %.3e" % (B, N, M, dim, gap))
        assert gap >= 1e-3
    w = torch.rand(B, generator=torch.Generator().manual_seed(seed + 100)) + 0.5
    p64, q64 = preds.double().requires_grad_(True), gts.double().requires_grad_(True)
    (O.chamfer(p64, q64) * w.double()).sum().backward()
    for need_p, need_g in ((True, True), (True, False), (False, True)):
        p = preds.to(DEV).requires_grad_(need_p)
        q = gts.to(DEV).requires_grad_(need_g)
        (PC.chamfer_distance(p, q) * w.to(DEV)).sum().backward()
        for t, ref, need in ((p, p64.grad, need_p), (q, q64.grad, need_g)):
            if not need:
                assert t.grad is None
                continue
            err = float((t.grad.double().cpu() - ref).abs().max() / ref.abs().max())
            assert err <= 1e-5, err


def test_chamfer_ties_lowest_index_and_determinism():
    PC = _PC()
    g = torch.Generator().manual_seed(11)
    B, N, M = 2, 300, 270
    gts = torch.rand(B, N, 3, generator=g, dtype=torch.float64).float()
    preds = torch.rand(B, M, 3, generator=g, dtype=torch.float64).float()
    gts[:, 20:30] = gts[:, 5:6]          # ten exact copies of point 5 ...
    gts[:, 280] = gts[:, 5]              # ... and one in the second block of lanes
    preds[:, 0] = gts[:, 5]              # predictions that sit exactly on / next to the duplicated point
    preds[:, 1] = gts[:, 5] + 1e-3
    preds[:, 260] = gts[:, 5] - 1e-3
    preds[:, 100:104] = preds[:, 40:41]  # duplicated predictions
    gts[:, 7] = preds[:, 40] + 1e-3      # a ground-truth point whose nearest prediction is a duplicated one
    P = O.pairwise_sqdist(preds.double(), gts.double())
    want = P.min(dim=1)[0].sum(1) + P.min(dim=2)[0].sum(1)
    p, q = preds.to(DEV).requires_grad_(True), gts.to(DEV).requires_grad_(True)
    loss, idx_p, idx_g = PC.chamfer_distance(p, q, return_indices=True)
    assert float(((loss.detach().double().cpu() - want).abs() / want).max()) <= 1e-5
    _check_indices_by_distance(P, idx_p, idx_g)
    # every index is the LOWEST among the exact copies of the point it names
    for idx, cloud in ((idx_p.cpu().long(), gts), (idx_g.cpu().long(), preds)):
        for b in range(B):
            chosen = cloud[b][idx[b]]                                       # [Q, 3]
            same = (cloud[b][None, :, :] == chosen[:, None, :]).all(-1)     # [Q, points]
            first = torch.where(same, torch.arange(cloud.shape[1])[None, :], cloud.shape[1]).min(dim=1)[0]
            assert torch.equal(first, idx[b])
    assert int(idx_p[0, 0]) == 5 and int(idx_p[0, 1]) == 5 and int(idx_p[0, 260]) == 5 and int(idx_g[0, 7]) == 40
    loss.sum().backward()
    p2, q2 = preds.to(DEV).requires_grad_(True), gts.to(DEV).requires_grad_(True)
    loss2, idx_p2, idx_g2 = PC.chamfer_distance(p2, q2, return_indices=True)
    loss2.sum().backward()
    assert torch.equal(loss, loss2) and torch.equal(idx_p, idx_p2) and torch.equal(idx_g, idx_g2)
    assert torch.equal(p.grad, p2.grad) and torch.equal(q.grad, q2.grad)
    dP, dG = O.chamfer_grads_from_indices(torch.ones(B, dtype=torch.float64), preds.double(), gts.double(), idx_p.cpu(),
                                          idx_g.cpu())
    assert float((p.grad.double().cpu() - dP).abs().max() / dP.abs().max()) <= 1e-5
    assert float((q.grad.double().cpu() - dG).abs().max() / dG.abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ ReLU -> BatchNorm
@pytest.mark.parametrize("B,C,N", [(3, 64, 100), (2, 512, 2048), (4, 5, 1), (1, 7, 33)])
def test_relu_bn(B, C, N):
    PC = _PC()
    from sivae_hip import functional as SF
    g = torch.Generator().manual_seed(B * 1000 + C + N)
    a = torch.randn(B, C, N, generator=g)
    a[torch.rand(B, C, N, generator=g) < 0.1] = 0.0          # exact zeros: ReLU's derivative there is 0
    a[:, 0] = -a[:, 0].abs() - 0.1                           # a channel that is dead everywhere
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    dy = torch.randn(B, C, N, generator=g)
    bn = _BN(C, True, 5)
    rm0, rv0 = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
    a64 = a.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64, rm64, rv64 = O.relu_bn(a64, g64, b64, rm0, rv0, True)
    (y64 * dy.double()).sum().backward()
    ad = a.to(DEV).requires_grad_(True)
    gd, bd = gamma.to(DEV).requires_grad_(True), beta.to(DEV).requires_grad_(True)
    y = PC.relu_bn(ad, gd, bd, SF.BNState(bn))
    (y * dy.to(DEV)).sum().backward()
    figs = dict(y=viol(y, y64), rm=viol(bn.running_mean, rm64), rv=viol(bn.running_var, rv64),
                da=viol(ad.grad, a64.grad), dgamma=viol(gd.grad, g64.grad), dbeta=viol(bd.grad, b64.grad))
    print("relu_bn [%d, %d, %d]: violation ratios %s" % (B, C, N, {k: "%.3f" % v for k, v in figs.items()}))
    assert all(v <= 1.0 for v in figs.values()), figs
    assert int(bn.num_batches_tracked) == 4
    assert bool((ad.grad[a.to(DEV) == 0] == 0).all()) and bool((ad.grad[:, 0] == 0).all())
    # eval mode: the running buffers, no update; its backward is refused
    bn_e = _BN(C, False, 6)
    rm, rv = bn_e.running_mean.clone(), bn_e.running_var.clone()
    ae = a.to(DEV).requires_grad_(True)
    ye = PC.relu_bn(ae, gd, bd, SF.BNState(bn_e))
    ye64, _, _ = O.relu_bn(a.double(), gamma.double(), beta.double(), rm.double().cpu(), rv.double().cpu(), False)
    assert viol(ye, ye64) <= 1.0
    assert torch.equal(bn_e.running_mean, rm) and torch.equal(bn_e.running_var, rv) and int(bn_e.num_batches_tracked) == 3
    with pytest.raises(RuntimeError, match="eval-mode BatchNorm"):
        ye.sum().backward()


# ------------------------------------------------------------------------------------------------ max over points
@pytest.mark.parametrize("B,C,N", [(3, 512, 100), (2, 512, 2048), (2, 3, 1)])
def test_max_points(B, C, N):
    PC = _PC()
    g = torch.Generator().manual_seed(B + C + N)
    x = torch.randn(B, C, N, generator=g)
    x[0, 1] = 0.25                                   # an all-equal channel: index 0 wins
    if N > 40:
        x[1, 2, 37] = x[1, 2, 5] = 9.0               # the maximum twice: the lower index wins
    vals, arg = PC.max_points_fwd(x.to(DEV))
    want = x.max(dim=2)[0]
    assert torch.equal(vals.cpu(), want)
    first = torch.where(x == want[:, :, None], torch.arange(N)[None, None, :], N).min(dim=2)[0]
    assert torch.equal(arg.cpu().long(), first)
    assert int(arg[0, 1]) == 0 and (N <= 40 or int(arg[1, 2]) == 5)
    gy = torch.randn(B, C, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    out = PC.max_points(xd)
    assert torch.equal(out, vals)
    (out * gy.to(DEV)).sum().backward()
    scatter = torch.zeros(B, C, N).scatter_(2, first[:, :, None], gy[:, :, None])
    assert torch.equal(xd.grad.cpu(), scatter)


# ------------------------------------------------------------------------------------------------ encoder / model
@pytest.mark.parametrize("B,N", [(3, 100), (2, 2048)])
def test_encoder(B, N):
    import soft_intro_vae_3d.models.vae as V
    z = 128
    specs = O.encoder_specs(z)
    g = torch.Generator().manual_seed(B + N)
    x = torch.rand(B, 3, N, generator=g) - 0.5
    r1, r2 = torch.randn(B, z, generator=g), torch.randn(B, z, generator=g)
    runs = {}
    for dt in (torch.float64, torch.float32):
        sd = O.leaves(O.recipe_state_dict(specs, 7, dt))
        upd = {}
        mu, lv = O.encoder(sd, x.to(dt), True, update=upd)
        ((mu * r1.to(dt)).sum() + (lv * r2.to(dt)).sum()).backward()
        runs[dt] = (sd, mu, lv, upd)
    sd64, mu64, lv64, upd64 = runs[torch.float64]
    enc = _load(V.Encoder(O.config(z)), sd64).train()
    mu, lv = enc(x.to(DEV))
    ((mu * r1.to(DEV)).sum() + (lv * r2.to(DEV)).sum()).backward()
    v_mu, v_lv = viol(mu, mu64), viol(lv, lv64)
    print("encoder B=%d N=%d: mu %.3f logvar %.3f of the element-wise criterion" % (B, N, v_mu, v_lv))
    assert v_mu <= 1.0 and v_lv <= 1.0
    for k, v in upd64.items():
        got = enc.state_dict()[k]
        assert (viol(got, v) <= 1.0) if v.is_floating_point() else (int(got) == int(v)), k
    _grad_report("encoder[%d,%d]" % (B, N), enc.named_parameters(), sd64, runs[torch.float32][0])


def test_model_vae_objective_and_adam_steps():
    """SoftIntroVAE, B = 2, N = 2048: one vanilla-VAE objective against fp64, then two stock torch.optim.Adam steps
    against the fp32 restatement on the CPU — the packed weight operands must follow the in-place updates"""
    import soft_intro_vae_3d.models.vae as V
    from soft_intro_vae_3d.losses.chamfer_loss import ChamferLoss
    from sivae_hip import functional as SF
    z, B, N = 128, 2, 2048
    specs = O.model_specs(z)
    g = torch.Generator().manual_seed(21)
    x = torch.rand(B, 3, N, generator=g) - 0.5
    eps = torch.randn(B, z, generator=g)
    sd64 = O.leaves(O.recipe_state_dict(specs, 9, torch.float64))
    out64 = O.vae_objective(sd64, x.double(), eps.double())
    out64["loss"].backward()
    sd32 = O.leaves(O.recipe_state_dict(specs, 9, torch.float32))
    model = _load(V.SoftIntroVAE(O.config(z)), sd32).train()
    chamfer = ChamferLoss()
    xd, epsd = x.to(DEV), eps.to(DEV)

    def objective():
        mu, logvar = model.encode(xd)
        rec = model.decode(V.reparameterize(mu, logvar, epsd))
        ch = chamfer(xd.permute(0, 2, 1) + 0.5, rec.permute(0, 2, 1) + 0.5)
        k = SF.kl(logvar, mu, 0.0, O.PRIOR_LOGVAR, "mean")
        return dict(mu=mu, logvar=logvar, rec=rec, chamfer=ch, kl=k, loss=20.0 * ch.mean() + 1.0 * k.reshape(()))

    opt_gpu = torch.optim.Adam(model.parameters(), lr=5e-4)
    params32 = [v for v in sd32.values() if v.requires_grad]
    opt_cpu = torch.optim.Adam(params32, lr=5e-4)
    losses = []
    for step in range(2):
        opt_gpu.zero_grad()
        opt_cpu.zero_grad()
        out = objective()
        out["loss"].backward()
        upd = {}
        out32 = O.vae_objective(sd32, x, eps, update=upd)
        out32["loss"].backward()
        if step == 0:
            figs = {k: viol(out[k], out64[k]) for k in ("mu", "logvar", "rec", "chamfer", "kl", "loss")}
            print("model: violation ratios vs fp64 %s" % {k: "%.3f" % v for k, v in figs.items()})
            assert all(v <= 1.0 for v in figs.values()), figs
            _grad_report("model", model.named_parameters(), sd64, sd32)
        opt_gpu.step()
        opt_cpu.step()
        sd32.update(upd)
        losses.append((float(out["loss"].detach()), float(out32["loss"].detach())))
    print("model: losses (gpu, cpu fp32) per Adam step: %s" % (losses,))
    assert abs(losses[0][0] - losses[1][0]) > 1e-4 * abs(losses[0][0])  # (the step changed the loss at all)
    assert abs(losses[1][0] - losses[1][1]) <= 1e-4 * abs(losses[1][1])
    # a batch of one decodes (the reference squeezes z to 1-D)
    y1 = model.decode(torch.zeros(1, z, device=DEV))
    assert y1.shape == (1, 3, 2048)
    y, mu, logvar = model(xd, deterministic=True)
    assert y.shape == (B, 3, 2048) and mu.shape == (B, z) and torch.equal(model.sample(mu), model.decode(mu))


def test_bootstrap_and_no_batchnorm_forward():
    import soft_intro_vae_3d.models.vae as V
    z, B, N = 16, 3, 100
    g = torch.Generator().manual_seed(31)
    x = torch.rand(B, 3, N, generator=g) - 0.5
    sd = O.recipe_state_dict(O.model_specs(z, bootstrap=True), 12, torch.float64)
    model = _load(V.SoftIntroVAEBootstrap(O.config(z)), sd).train()
    mu64, lv64 = O.encoder(sd, x.double(), True, prefix="encoder.")
    for use_target, prefix in ((True, "target_decoder."), (False, "decoder.")):
        model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)  # (fresh BatchNorm buffers per pass)
        y, mu, lv = model(x.to(DEV), deterministic=True, use_target_decoder=use_target)
        assert viol(mu, mu64) <= 1.0 and viol(lv, lv64) <= 1.0
        assert viol(y, O.decoder(sd, mu64, prefix=prefix)) <= 1.0
        assert viol(model.sample(mu, use_target_decoder=use_target), O.decoder(sd, mu64, prefix=prefix)) <= 1.0
    assert not torch.equal(model.decode(mu), model.decode_target(mu))
    for use_bias in (True, False):
        sdn = O.recipe_state_dict(O.encoder_specs(z, bn=False, use_bias=use_bias), 13, torch.float64)
        enc = _load(V.EncoderNoBatchNorm(O.config(z, use_bias_e=use_bias)), sdn)
        mu, lv = enc(x.to(DEV))
        m64, l64 = O.encoder(sdn, x.double(), bn=False)
        assert viol(mu, m64) <= 1.0 and viol(lv, l64) <= 1.0
