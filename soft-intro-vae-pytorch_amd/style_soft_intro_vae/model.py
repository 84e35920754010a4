"""Drop-in model of the style variant (reference: style_soft_intro_vae/model.py) on the HIP kernels.

The third drop-in file, next to net.py and blocks.py: put this directory in front of the reference's style_soft_intro_vae
directory on PYTHONPATH and the reference's training script builds SoftIntroVAEModelTL from here.  set_model_require_grad,
reparameterize, calc_kl, calc_reconstruction_loss, DLatent and SoftIntroVAEModelTL keep the reference's signatures,
constructor arguments and defaults, attribute names, construction order, state_dict keys and order (dlatent_avg.buff
included), initial values for a seed, the places and order of the Python `random` calls and the requires_grad flags each
branch of forward leaves behind.

Deliberate differences (FUSED = True):
  * generate draws z (and z2) on the model's device instead of the default device;
  * generate calls mapping_fl.map (the un-repeated rows [B, Z], one autograd node: sivae_hip.style.mapping) when the mapping
    has one, and falls back to the reference's mapping_fl(z)[:, 0];
  * the repeat over the layers, the running average of the styles, style mixing and the truncation trick
    (model.py:176-200) are sivae_hip.style.styles: one node, the average updated in place before the truncation;
  * encode takes mapping_tl.map's rows [B, 2 Z] apart into mu and logvar (the same memory as the reference's view) and
    samples with sivae_hip.functional.reparameterize from ONE torch.randn_like, at the reference's point in the draw order;
  * the losses are sivae_hip.functional.kl, ReconFn ('rows', or 'total' with the scale 1 / B), functional.expelbo and
    functional.lincomb instead of eager torch;
  * last_rec_loss, last_real_kl, last_fake_kl, last_kl_diff, last_expelbo_fake and last_expelbo_rec are detached 0-dim
    DEVICE tensors: forward synchronises with the host nowhere (the training script's `.data.cpu()` and the tracker work
    on them as before);
  * lerp(other, betta) is sivae_hip.lreq_adam.lerp_parameters over the reference's parameter list (model.py:324-327), one
    multi-tensor launch.  That list holds no buffer, so dlatent_avg.buff is not averaged, as in the reference.

FUSED = False selects the torch restatement of the same flow: the per-layer mapping chain, torch's repeat / mean / lerp_ /
where / lerp and torch losses (last_* are still device tensors).  Tensors that are not float32 take it whatever the switch
says; CPU tensors are refused by the kernels ("no CPU fallback") and accepted by the restatement's helpers.
"""
import random

import numpy as np  # noqa: F401  (the reference's namespace)
import torch
from torch import nn
from torch.nn import functional as F

from net import *  # noqa: F401,F403
from net import ENCODERS, GENERATORS, MAPPINGS
from sivae_hip import functional as SF
from sivae_hip import lreq_adam, style

FUSED = True  # a module switch like sivae_hip.nn.DEFER_UPSAMPLE: False = the torch restatement (see above)


def _kernels(*tensors):
    """do these tensors take the kernels: the switch, and float32 (a CPU tensor does too, and is refused there)"""
    return FUSED and all(t.dtype == torch.float32 for t in tensors)


def set_model_require_grad(model, val):
    for param in model.parameters():
        param.requires_grad = val


def reparameterize(mu, logvar):
    """z = mu + exp(logvar / 2) eps with ONE standard-normal draw eps of mu's shape"""
    if _kernels(mu, logvar):
        return SF.reparameterize(mu, logvar, torch.randn_like(mu).contiguous())
    std = torch.exp(0.5 * logvar)
    return mu + torch.randn_like(std) * std


def calc_kl(logvar, mu, mu_o=10, is_outlier=False, reduce='sum'):
    """KL(N(mu, exp(logvar)) || N(0, I)) per sample [B] (with is_outlier: the reference's shifted form, torch only),
    reduced over the batch by 'sum' or 'mean'; any other `reduce` leaves the per-sample values"""
    if not is_outlier and _kernels(logvar, mu):
        return SF.kl(logvar, mu, 0.0, 0.0, reduce if reduce in ('sum', 'mean') else 'none')
    inner = 1 + logvar - mu.pow(2) - logvar.exp()
    if is_outlier:
        inner = inner + 2 * mu * mu_o - mu_o.pow(2)
    kl = -0.5 * inner.sum(1)
    return {'sum': torch.sum, 'mean': torch.mean}.get(reduce, lambda t: t)(kl)


def calc_reconstruction_loss(x, recon_x, loss_type='mse', reduction='sum'):
    """loss_type 'mse': the squared error summed per sample [B], then 'sum' / 'mean' over the batch or 'none';
    'l1' / 'bce': torch's F.l1_loss / F.binary_cross_entropy of the flattened samples with that reduction"""
    if reduction not in ('sum', 'mean', 'none') or loss_type not in ('mse', 'l1', 'bce'):
        raise NotImplementedError
    if loss_type == 'mse' and _kernels(x, recon_x):
        if reduction == 'none':
            return SF.ReconFn.apply(x, recon_x, 'mse', 'rows', 1.0)
        return SF.ReconFn.apply(x, recon_x, 'mse', 'total', 1.0 if reduction == 'sum' else 1.0 / x.size(0))
    recon_x, x = recon_x.view(recon_x.size(0), -1), x.view(x.size(0), -1)
    if loss_type == 'l1':
        return F.l1_loss(recon_x, x, reduction=reduction)
    if loss_type == 'bce':
        return F.binary_cross_entropy(recon_x, x, reduction=reduction)
    rows = F.mse_loss(recon_x, x, reduction='none').sum(1)
    return {'sum': rows.sum, 'mean': rows.mean}.get(reduction, lambda: rows)()


def _expelbo(rec_rows, kl_rows, scale, beta_rec, beta_neg):
    """mean_i exp(-2 scale (beta_rec L_i + beta_neg KL_i))  (model.py:251-252)"""
    if _kernels(rec_rows, kl_rows):
        return SF.expelbo(rec_rows, kl_rows, scale, beta_rec, beta_neg)
    return (-2 * scale * (beta_rec * rec_rows + beta_neg * kl_rows)).exp().mean()


def _lincomb(terms, weights):
    """sum_i weights[i] terms[i] over 0-dim losses: one launch each way"""
    if _kernels(*terms):
        return SF.lincomb(terms, weights)
    return sum(w * t for t, w in zip(terms, weights))


class DLatent(nn.Module):
    def __init__(self, dlatent_size, layer_count):
        super().__init__()
        self.register_buffer('buff', torch.zeros(layer_count, dlatent_size, dtype=torch.float32))


class SoftIntroVAEModelTL(nn.Module):
    def __init__(self, startf=32, maxf=256, layer_count=3, latent_size=128, mapping_layers=5, dlatent_avg_beta=None,
                 truncation_psi=None, truncation_cutoff=None, style_mixing_prob=None, channels=3, generator="",
                 encoder="", beta_kl=1.0, beta_rec=1.0, beta_neg=1.0, scale=1 / (3 * 256 ** 2), gamma_r=1e-8):
        super().__init__()
        self.layer_count = layer_count
        self.beta_kl, self.beta_rec, self.beta_neg = beta_kl, beta_rec, beta_neg
        self.scale, self.gamma_r = scale, gamma_r
        for name in ("last_kl_diff", "last_rec_loss", "last_real_kl", "last_fake_kl", "last_expelbo_fake",
                     "last_expelbo_rec"):
            setattr(self, name, torch.tensor(0.0))
        # (the reference's order of construction: it fixes the order of the state dict and of the initial draws)
        width = dict(latent_size=latent_size, dlatent_size=latent_size, mapping_fmaps=latent_size)
        self.mapping_tl = MAPPINGS["MappingToLatent"](mapping_layers=3, **width)
        self.mapping_fl = MAPPINGS["MappingFromLatent"](num_layers=2 * layer_count, mapping_layers=mapping_layers, **width)
        net = dict(startf=startf, layer_count=layer_count, maxf=maxf, latent_size=latent_size, channels=channels)
        self.decoder = GENERATORS[generator](**net)
        self.encoder = ENCODERS[encoder](**net)
        self.dlatent_avg = DLatent(latent_size, self.mapping_fl.num_layers)
        self.latent_size = latent_size
        self.dlatent_avg_beta = dlatent_avg_beta
        self.truncation_psi, self.truncation_cutoff = truncation_psi, truncation_cutoff
        self.style_mixing_prob = style_mixing_prob

    def _map_from_latent(self, z, fused):
        """the un-repeated styles [B, Z] of z"""
        if hasattr(self.mapping_fl, "map"):
            return self.mapping_fl.map(z, fused=fused)
        return self.mapping_fl(z)[:, 0]

    def _mixing_source(self, lod, count, device, fused):
        """style mixing (model.py:185-193), the Python `random` calls and the draw of z2 in the reference's order ->
        (the second latent's styles [B, Z], the first layer that takes them), or (None, None) when it is not taken"""
        if self.style_mixing_prob is None or not random.random() < self.style_mixing_prob:
            return None, None
        z2 = torch.randn(count, self.latent_size, device=device)
        return self._map_from_latent(z2, fused), random.randint(1, (lod + 1) * 2)

    def generate(self, lod, blend_factor, z=None, count=32, mixing=True, noise=True, return_styles=False,
                 no_truncation=False):
        """an image batch from z (drawn from the prior when None) -> rec, or (s [B, 1, Z], rec) with return_styles"""
        avg = self.dlatent_avg.buff.data
        device, num_layers = avg.device, self.mapping_fl.num_layers
        if z is None:
            z = torch.randn(count, self.latent_size, device=device)
        fused = _kernels(z)
        s = self._map_from_latent(z, fused)
        psi = None if no_truncation else self.truncation_psi
        if fused:
            s2, mix_cutoff = self._mixing_source(lod, count, device, fused) if mixing else (None, None)
            styles = style.styles(s, num_layers, s2=s2, cutoff=mix_cutoff,
                                  avg=None if (self.dlatent_avg_beta is None and psi is None) else avg,
                                  beta=self.dlatent_avg_beta, psi=psi,
                                  trunc_cutoff=None if psi is None else self.truncation_cutoff)
        else:
            styles = s.unsqueeze(1).repeat(1, num_layers, 1)
            layer = torch.arange(num_layers, device=device).view(1, -1, 1)
            if self.dlatent_avg_beta is not None:  # (before the truncation, which reads the updated average)
                with torch.no_grad():
                    avg.lerp_(styles.detach().mean(dim=0), 1.0 - self.dlatent_avg_beta)
            s2, mix_cutoff = self._mixing_source(lod, count, device, fused) if mixing else (None, None)
            if s2 is not None:
                styles = torch.where(layer < mix_cutoff, styles, s2.unsqueeze(1).repeat(1, num_layers, 1))
            if psi is not None:
                ones = torch.ones(layer.shape, dtype=styles.dtype, device=device)
                styles = torch.lerp(avg, styles, torch.where(layer < self.truncation_cutoff, psi * ones, ones))
        rec = self.decoder.forward(styles, lod, blend_factor, noise)
        return (s.view(s.shape[0], 1, s.shape[1]), rec) if return_styles else rec

    def encode(self, x, lod, blend_factor):
        y = self.encoder(x, lod, blend_factor)
        if hasattr(self.mapping_tl, "map"):
            y = self.mapping_tl.map(y, fused=_kernels(y))  # [B, 2 Z]: the memory the reference views as [B, 2, Z]
            half = y.shape[1] // 2
            mu, logvar = y[:, :half], y[:, half:]
        else:
            y = self.mapping_tl(y)
            mu, logvar = y[:, 0, :], y[:, 1, :]
        return reparameterize(mu, logvar), mu, logvar

    def _train_only(self, encoder_side, decoder_side):
        set_model_require_grad(self.encoder, encoder_side)
        set_model_require_grad(self.mapping_tl, encoder_side)
        set_model_require_grad(self.decoder, decoder_side)
        set_model_require_grad(self.mapping_fl, decoder_side)

    def _decode(self, z, lod, blend_factor):
        return self.generate(lod, blend_factor, z=z, mixing=False, noise=True, return_styles=True, no_truncation=True)[1]

    def forward(self, x, lod, blend_factor, d_train, e_train, fake_rec_coef=1e-8):
        """the loss of one branch: e_train (the encoder's step, model.py:216-263), else d_train (the decoder's, :265-299),
        else the plain VAE (:300-318)"""
        if e_train:
            return self._encoder_loss(x, lod, blend_factor)
        if d_train:
            return self._decoder_loss(x, lod, blend_factor)
        self._train_only(True, True)
        z_real, mu_real, logvar_real = self.encode(x, lod, blend_factor)
        rec = self._decode(z_real, lod, blend_factor)
        loss_rec = calc_reconstruction_loss(x, rec, loss_type="mse", reduction="mean")
        loss_kl = calc_kl(logvar_real, mu_real, reduce="mean")
        self.last_rec_loss, self.last_real_kl = loss_rec.detach(), loss_kl.detach()
        return _lincomb([loss_rec, loss_kl], [self.beta_rec, self.beta_kl])

    def _encoder_loss(self, x, lod, blend_factor):
        self._train_only(True, False)
        fake = self.generate(lod, blend_factor, count=x.shape[0], noise=True, no_truncation=True)
        z_real, mu_real, logvar_real = self.encode(x, lod, blend_factor)
        rec = self._decode(z_real, lod, blend_factor)
        loss_rec = calc_reconstruction_loss(x, rec, loss_type="mse", reduction="mean")
        kl_real = calc_kl(logvar_real, mu_real, reduce="mean")
        z_rec, mu_rec, logvar_rec = self.encode(rec.detach(), lod, blend_factor)
        rec_rec = self._decode(z_rec, lod, blend_factor)
        z_fake, mu_fake, logvar_fake = self.encode(fake.detach(), lod, blend_factor)
        rec_fake = self._decode(z_fake, lod, blend_factor)
        kl_rec = calc_kl(logvar_rec, mu_rec, reduce="none")
        kl_fake = calc_kl(logvar_fake, mu_fake, reduce="none")
        rows_rec = calc_reconstruction_loss(rec, rec_rec, loss_type="mse", reduction="none")
        rows_fake = calc_reconstruction_loss(fake, rec_fake, loss_type="mse", reduction="none")
        expelbo_rec = _expelbo(rows_rec, kl_rec, self.scale, self.beta_rec, self.beta_neg)
        expelbo_fake = _expelbo(rows_fake, kl_fake, self.scale, self.beta_rec, self.beta_neg)
        self.last_rec_loss, self.last_real_kl = loss_rec.detach(), kl_real.detach()
        self.last_expelbo_fake, self.last_expelbo_rec = expelbo_fake.detach(), expelbo_rec.detach()
        # scale (beta_rec loss_rec + beta_kl kl_real) + 0.25 (expelbo_rec + expelbo_fake)
        return _lincomb([loss_rec, kl_real, expelbo_rec, expelbo_fake],
                        [self.scale * self.beta_rec, self.scale * self.beta_kl, 0.25, 0.25])

    def _decoder_loss(self, x, lod, blend_factor):
        self._train_only(False, True)
        fake = self.generate(lod, blend_factor, count=x.shape[0], noise=True, no_truncation=True)
        z_real, _, _ = self.encode(x, lod, blend_factor)
        rec = self._decode(z_real.detach(), lod, blend_factor)
        loss_rec = calc_reconstruction_loss(x, rec, loss_type="mse", reduction="mean")
        z_rec, mu_rec, logvar_rec = self.encode(rec, lod, blend_factor)
        z_fake, mu_fake, logvar_fake = self.encode(fake, lod, blend_factor)
        rec_rec = self._decode(z_rec.detach(), lod, blend_factor)
        rec_fake = self._decode(z_fake.detach(), lod, blend_factor)
        loss_rec_rec = calc_reconstruction_loss(rec.detach(), rec_rec, loss_type="mse", reduction="mean")
        loss_fake_rec = calc_reconstruction_loss(fake.detach(), rec_fake, loss_type="mse", reduction="mean")
        kl_rec = calc_kl(logvar_rec, mu_rec, reduce="mean")
        kl_fake = calc_kl(logvar_fake, mu_fake, reduce="mean")
        self.last_rec_loss = loss_rec.detach()
        self.last_kl_diff = self.last_fake_kl - self.last_real_kl  # (the PREVIOUS fake KL, as in the reference)
        self.last_fake_kl = kl_fake.detach()
        # scale (beta_rec loss_rec + 0.5 beta_kl (kl_rec + kl_fake) + 0.5 gamma_r beta_rec (loss_rec_rec + loss_fake_rec))
        w_kl = self.scale * 0.5 * self.beta_kl
        w_rr = self.scale * self.gamma_r * 0.5 * self.beta_rec
        return _lincomb([loss_rec, kl_rec, kl_fake, loss_rec_rec, loss_fake_rec],
                        [self.scale * self.beta_rec, w_kl, w_kl, w_rr, w_rr])

    def _averaged(self):
        """what lerp walks (model.py:324-327): parameters only, so dlatent_avg (a buffer) adds nothing"""
        return [p for m in (self.mapping_tl, self.mapping_fl, self.decoder, self.encoder, self.dlatent_avg)
                for p in m.parameters()]

    def lerp(self, other, betta):
        other = getattr(other, "module", other)
        lreq_adam.lerp_parameters(self._averaged(), other._averaged(), 1.0 - betta)
