"""torch-CPU restatement of the 3-D point-cloud Soft-IntroVAE (reference: soft_intro_vae_3d/models/vae.py,
losses/chamfer_loss.py, train_soft_intro_vae_3d.py:88-108), written from the maths, parametrised by dtype:

  encoder   five stages Conv1d(k=1) -> ReLU -> BatchNorm1d (3-64-128-256-256-512), max over the points,
            Linear(512, 256) + ReLU, two heads Linear(256, z)
  decoder   Linear z-64-128-512-1024-6144 with ReLU between, viewed as [B, 3, 2048]
  chamfer   sum_j min_i |G_i - P_j|^2 + sum_i min_j |G_i - P_j|^2, distances in the DIRECT form
  kl        -0.5 sum(1 + lv - lv_o - exp(lv) / exp(lv_o) - (mu - mu_o)^2 / exp(lv_o))

Parameters live in a plain dict with the reference's state_dict keys.  Weights are never stored in fixtures: both
sides rebuild them with `recipe_state_dict` (uniform doubles of numpy's PCG64, in state_dict order, scaled to each
layer's default-init bound) — no library's random stream has to stay put.
"""
import math

import numpy as np
import torch

WIDTHS_E = (3, 64, 128, 256, 256, 512)
N_OUT = 2048
BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def config(z_size, use_bias_d=True, use_bias_e=True):
    return {"z_size": z_size, "model": {"D": {"use_bias": use_bias_d, "relu_slope": 0.2},
                                        "E": {"use_bias": use_bias_e, "relu_slope": 0.2}}}


def decoder_specs(z, use_bias=True, prefix=""):
    w = (z, 64, 128, 512, 1024, N_OUT * 3)
    out = []
    for i in range(5):
        out.append((prefix + "model.%d.weight" % (2 * i), (w[i + 1], w[i]), "w", w[i]))
        if use_bias:
            out.append((prefix + "model.%d.bias" % (2 * i), (w[i + 1],), "w", w[i]))
    return out


def encoder_specs(z, bn=True, use_bias=True, prefix=""):
    """(key, shape, kind, fan_in) in state_dict order; bn=False: EncoderNoBatchNorm (conv bias from use_bias)"""
    out = []
    step = 3 if bn else 2
    for i in range(5):
        ci, co = WIDTHS_E[i], WIDTHS_E[i + 1]
        out.append((prefix + "conv.%d.weight" % (step * i), (co, ci, 1), "w", ci))
        if bn:
            k = prefix + "conv.%d." % (3 * i + 2)
            out += [(k + "weight", (co,), "gamma", 0), (k + "bias", (co,), "beta", 0), (k + "running_mean", (co,), "rm", 0),
                    (k + "running_var", (co,), "rv", 0), (k + "num_batches_tracked", (), "nbt", 0)]
        elif use_bias:
            out.append((prefix + "conv.%d.bias" % (step * i), (co,), "w", ci))
    for name, co, ci in (("fc.0", 256, 512), ("mu_layer", z, 256), ("std_layer", z, 256)):
        out += [(prefix + name + ".weight", (co, ci), "w", ci), (prefix + name + ".bias", (co,), "w", ci)]
    return out


def model_specs(z, bootstrap=False, use_bias_d=True):
    s = encoder_specs(z, prefix="encoder.") + decoder_specs(z, use_bias_d, prefix="decoder.")
    if bootstrap:
        s += decoder_specs(z, use_bias_d, prefix="target_decoder.")
    return s


def recipe_state_dict(specs, seed, dtype=torch.float64):
    """weights / biases uniform in +-1/sqrt(fan_in) (the default-init bound of nn.Linear / nn.Conv1d); BatchNorm gamma in
    [0.5, 1.5], beta in [-0.1, 0.1], running_mean in [-0.1, 0.1], running_var in [0.5, 1.5] (so that eval mode and
    the affine part are exercised), num_batches_tracked 0; all from one PCG64 stream in spec order"""
    g = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for key, shape, kind, fan_in in specs:
        if kind == "nbt":
            sd[key] = torch.zeros((), dtype=torch.int64)
            continue
        u = torch.from_numpy(g.random(size=shape))  # doubles in [0, 1)
        if kind == "w":
            v = (2.0 * u - 1.0) / math.sqrt(fan_in)
        elif kind in ("gamma", "rv"):
            v = 0.5 + u
        else:
            v = 0.1 * (2.0 * u - 1.0)
        sd[key] = v.to(dtype)
    return sd


def leaves(sd, prefix=""):
    """the differentiable entries of sd (everything but BatchNorm buffers) as fresh leaf tensors, in place"""
    for k, v in sd.items():
        if k.startswith(prefix) and v.is_floating_point() and "running_" not in k:
            sd[k] = v.detach().clone().requires_grad_(True)
    return sd


def _conv1(x, w, b=None):
    y = torch.einsum("oc,bcn->bon", w[:, :, 0], x)
    return y if b is None else y + b[None, :, None]


def relu_bn(a, gamma, beta, running_mean, running_var, training):
    """BatchNorm1d(ReLU(a)) over [B, C, N] -> (y, new running_mean, new running_var)"""
    r = torch.relu(a)
    if training:
        m = r.shape[0] * r.shape[2]
        mean = r.mean(dim=(0, 2))
        var = ((r - mean[None, :, None]) ** 2).mean(dim=(0, 2))
        unb = var * m / (m - 1) if m > 1 else var
        running_mean = (1 - BN_MOMENTUM) * running_mean + BN_MOMENTUM * mean.detach()
        running_var = (1 - BN_MOMENTUM) * running_var + BN_MOMENTUM * unb.detach()
    else:
        mean, var = running_mean, running_var
    y = (r - mean[None, :, None]) / torch.sqrt(var[None, :, None] + BN_EPS) * gamma[None, :, None] + beta[None, :, None]
    return y, running_mean, running_var


def encoder(sd, x, training=True, prefix="", bn=True, update=None):
    """-> (mu, logvar); update: a dict that receives the new BatchNorm buffers (training mode)"""
    step = 3 if bn else 2
    for i in range(5):
        a = _conv1(x, sd[prefix + "conv.%d.weight" % (step * i)], sd.get(prefix + "conv.%d.bias" % (step * i)) if not bn else None)
        if bn:
            k = prefix + "conv.%d." % (3 * i + 2)
            x, rm, rv = relu_bn(a, sd[k + "weight"], sd[k + "bias"], sd[k + "running_mean"], sd[k + "running_var"], training)
            if update is not None and training:
                update[k + "running_mean"], update[k + "running_var"] = rm, rv
                update[k + "num_batches_tracked"] = sd[k + "num_batches_tracked"] + 1
        else:
            x = torch.relu(a) if i < 4 else a
    pooled = x.max(dim=2)[0]
    h = torch.relu(pooled @ sd[prefix + "fc.0.weight"].T + sd[prefix + "fc.0.bias"])
    return (h @ sd[prefix + "mu_layer.weight"].T + sd[prefix + "mu_layer.bias"],
            h @ sd[prefix + "std_layer.weight"].T + sd[prefix + "std_layer.bias"])


def decoder(sd, z, prefix=""):
    h = z.reshape(-1, z.shape[-1])
    for i in range(5):
        h = h @ sd[prefix + "model.%d.weight" % (2 * i)].T
        b = sd.get(prefix + "model.%d.bias" % (2 * i))
        if b is not None:
            h = h + b
        if i < 4:
            h = torch.relu(h)
    return h.view(-1, 3, N_OUT)


def pairwise_sqdist(preds, gts):
    """[B, N, M]: |G_i - P_j|^2 in the direct form"""
    d = gts[:, :, None, :] - preds[:, None, :, :]
    return (d * d).sum(-1)


def chamfer(preds, gts, return_indices=False):
    """preds [B, M, 3], gts [B, N, 3] -> [B] (and idx_p [B, M] into gts, idx_g [B, N] into preds)"""
    P = pairwise_sqdist(preds, gts)
    m1, i1 = P.min(dim=1)  # over the ground truth, per prediction
    m2, i2 = P.min(dim=2)  # over the predictions, per ground-truth point
    loss = m1.sum(1) + m2.sum(1)
    return (loss, i1, i2) if return_indices else loss


def chamfer_grads_from_indices(g, preds, gts, idx_p, idx_g):
    """the analytic gradient for GIVEN nearest-neighbour indices:
    dP_j = 2 g (P_j - G_a(j)) + sum_{i: c(i) = j} 2 g (P_j - G_i), dG symmetric"""
    B, M, N = preds.shape[0], preds.shape[1], gts.shape[1]
    dP, dG = torch.zeros_like(preds), torch.zeros_like(gts)
    for b in range(B):
        a, c = idx_p[b].long(), idx_g[b].long()
        own_p = preds[b] - gts[b][a]      # [M, 3]
        own_g = gts[b] - preds[b][c]      # [N, 3]
        dP[b] = own_p
        dP[b].index_add_(0, c, -own_g)    # (P_c(i) - G_i) for every i
        dG[b] = own_g
        dG[b].index_add_(0, a, -own_p)
        dP[b] *= 2 * g[b]
        dG[b] *= 2 * g[b]
    return dP, dG


def kl(logvar, mu, mu_o=0.0, logvar_o=0.0, reduce="sum"):
    lo = torch.as_tensor(logvar_o, dtype=mu.dtype)
    mo = torch.as_tensor(mu_o, dtype=mu.dtype)
    v = -0.5 * (1 + logvar - lo - logvar.exp() / torch.exp(lo) - (mu - mo) ** 2 / torch.exp(lo)).sum(1)
    if reduce == "sum":
        return v.sum()
    if reduce == "mean":
        return v.mean()
    return v


def reparameterize(mu, logvar, eps):
    return mu + eps * torch.exp(0.5 * logvar)


PRIOR_LOGVAR = math.log(0.2 ** 2)


def vae_objective(sd, x, eps, beta_rec=20.0, beta_kl=1.0, training=True, update=None):
    """the vanilla-VAE iteration of train_soft_intro_vae_3d.py:225-231 -> dict(mu, logvar, rec, chamfer, kl, loss)"""
    mu, logvar = encoder(sd, x, training, prefix="encoder.", update=update)
    rec = decoder(sd, reparameterize(mu, logvar, eps), prefix="decoder.")
    ch = chamfer(x.permute(0, 2, 1) + 0.5, rec.permute(0, 2, 1) + 0.5)
    k = kl(logvar, mu, logvar_o=PRIOR_LOGVAR, reduce="mean")
    return dict(mu=mu, logvar=logvar, rec=rec, chamfer=ch, kl=k, loss=beta_rec * ch.mean() + beta_kl * k)


# [B, C, N] -> number of slices a channel's B * N values are cut into by the ReLU -> BatchNorm kernels: the shapes of
# tests/test_pointcloud_paths_gpu.py::test_relu_bn_sliced, pinned on the host by test_pointcloud_host.py
RELU_BN_SLICED = {(3, 5, 1368): 2, (3, 7, 2731): 3, (9, 3, 1001): 3, (4, 1024, 2052): 2, (32, 64, 2048): 16}


def rel_l2(a, b):
    """|a - b|_2 / |b|_2 in fp64"""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))
