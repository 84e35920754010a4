"""float64 torch restatement, on the CPU, of the four ops of csrc/mapping.hip and the LeakyReLU epilogue of
csrc/linear.hip (reference: style_soft_intro_vae/net.py:29-30, :748-751 and model.py:176-200), and the shapes the GPU
tests run them at.

    python tests/style_model_oracle.py      prints fp32_loss(): what a float32 restatement loses against float64

The gates of tests/test_style_model_gpu.py come from here: the forward gate is the project's element-wise criterion
(style_oracle.viol <= 1), the gradient gate min(4 x the printed fp32 figure, 1e-4) in style_oracle.nerr.  The figure is
measured against this restatement, never against the kernels.
"""
import itertools

import torch
from torch.nn import functional as F

from style_oracle import nerr, viol  # noqa: F401  (the tests take them from here)

SLOPE, EPS = 0.2, 1e-8

# ---- shapes: the smallest at which each kernel can still go wrong ---------------------------------------------------------
# pixel-norm (B, Z): a wave owns a row and walks it in trips of 256 elements (64 lanes x 4), 4 rows to a block
PN_CASES = [(1, 1), (2, 3), (2, 8), (3, 64), (3, 65), (5, 255), (4, 256), (2, 257), (130, 512), (2, 1027), (1, 4100)]
# linear + LeakyReLU (B, K, N): S == 1 below K = 128 (the epilogue in the GEMM kernel), S > 1 from there (in the reduce
# kernel); N not a multiple of 32; more than one 32-row block; the 256-row chunking
LIN_CASES = [(1, 8, 12), (2, 12, 8), (2, 64, 32), (2, 128, 36), (33, 512, 512), (130, 512, 1024), (257, 128, 64)]
# the same shapes serve the LeakyReLU backward (B, N): a block owns 64 columns x 16 row groups of ceil(B / 16) rows
# styles (B, L, Z): one thread per (sample, quad)
ST_SHAPES = [(1, 2, 1), (2, 6, 8), (3, 6, 7), (4, 14, 512), (130, 18, 512), (2, 6, 1027)]


def st_variants(L):
    """(mixing cutoff or None, truncation cutoff or None, beta or None): plain; mixing cutoff 1, middle, L; truncation
    cutoff 0, middle, L at psi 0.7; beta None, 0.995 and 0.0 (the average becomes the batch mean: an update placed behind
    the truncation is visible)"""
    mid = max(1, L // 2)
    out = [(None, None, None)]
    out += [(c, None, None) for c in sorted({1, mid, L})]
    out += [(None, t, b) for t in sorted({0, mid, L}) for b in (None, 0.995, 0.0)]
    out += [(mid, mid, 0.0), (1, L, 0.995), (None, None, 0.995), (None, None, 0.0)]
    return out


PSI = 0.7
ST_CASES = [(shape, var) for shape in ST_SHAPES for var in st_variants(shape[1])]
CASES = dict(pixel_norm=PN_CASES[:8], linear=LIN_CASES[:4], styles=[c for c in ST_CASES if c[0][0] * c[0][2] < 4096])
EDGE_CASES = dict(pixel_norm=PN_CASES[8:], linear=LIN_CASES[4:], styles=[c for c in ST_CASES if c[0][0] * c[0][2] >= 4096])


def rand(*shape, seed, dtype=torch.float64):
    """values exact in float32"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).float().to(dtype)


# ---- the four ops ---------------------------------------------------------------------------------------------------------
def pixel_norm(x, eps=EPS):
    return x * torch.rsqrt(x.pow(2.0).mean(dim=1, keepdim=True) + eps)


def linear_lrelu(x, w, b, slope=SLOPE):
    return F.leaky_relu(x @ w.t() + b, slope)


def lrelu_bias_bwd(dy, y, slope=SLOPE):
    """from the saved output; the slope at 0 is `slope` (torch's rule)"""
    dz = dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    return dz, dz.sum(0)


def styles(s, L, s2=None, cutoff=None, avg=None, beta=None, psi=None, trunc_cutoff=None):
    """-> (styles [B, L, Z], the average after the call) in the reference's order: update, mixing, truncation"""
    out = s.unsqueeze(1).repeat(1, L, 1)
    layer = torch.arange(L).view(1, L, 1)
    if beta is not None:
        avg = torch.lerp(avg, out.detach().mean(dim=0), 1.0 - beta)
    if s2 is not None:
        out = torch.where(layer < cutoff, out, s2.unsqueeze(1).repeat(1, L, 1))
    if psi is not None:
        coef = torch.where(layer < trunc_cutoff, torch.full((1, L, 1), psi, dtype=s.dtype), torch.ones(1, L, 1, dtype=s.dtype))
        out = torch.lerp(avg, out, coef)
    return out, avg


def planted_rows(Z, dtype=torch.float64):
    """rows of tiny elements with ONE large one at the LAST position (and one with it at the first): a row sum that drops
    its tail misses the criterion by orders of magnitude"""
    x = torch.full((3, Z), 2.0 ** -12, dtype=dtype)
    x[0, Z - 1] = 64.0
    x[1, 0] = 64.0
    x[2, Z - 1] = -64.0
    return x


# ---- inputs and float64 results of a case ------------------------------------------------------------------------------------
def pn_case(B, Z, dtype=torch.float64):
    x = rand(B, Z, seed=11 * B + Z, dtype=dtype).requires_grad_(True)
    g = rand(B, Z, seed=13 * B + Z + 1, dtype=dtype)
    y = pixel_norm(x)
    (dx,) = torch.autograd.grad((y * g).sum(), x)
    # dx = r dy - x r^3 mean(dy x) is a difference of terms of the size lead = max r max |dy| that cancels altogether where a
    # row is one element (dx = dy r eps / (x^2 + eps)): the measure for nerr
    r = torch.rsqrt(x.detach().double().pow(2.0).mean(dim=1) + EPS)
    return dict(x=x.detach(), g=g, y=y.detach(), dx=dx, lead=float(r.max() * g.abs().max()))


def lin_case(B, K, N, dtype=torch.float64):
    x = rand(B, K, seed=B + 3 * K + 5 * N, dtype=dtype)
    w = (rand(N, K, seed=B + 3 * K + 5 * N + 1, dtype=dtype) / K ** 0.5).float().to(dtype)
    b = (0.3 * rand(N, seed=B + 3 * K + 5 * N + 2, dtype=dtype)).float().to(dtype)
    g = rand(B, N, seed=B + 3 * K + 5 * N + 3, dtype=dtype)
    y = linear_lrelu(x, w, b)
    dz, db = lrelu_bias_bwd(g, y)
    return dict(x=x, w=w, b=b, g=g, y=y, dz=dz, db=db)


def st_case(shape, var, dtype=torch.float64):
    (B, L, Z), (cut, tcut, beta) = shape, var
    seed = 7 * B + 3 * L + Z + 100 * len(str(var))
    s = rand(B, Z, seed=seed, dtype=dtype).requires_grad_(True)
    s2 = rand(B, Z, seed=seed + 1, dtype=dtype).requires_grad_(True) if cut is not None else None
    avg = rand(L, Z, seed=seed + 2, dtype=dtype) if (beta is not None or tcut is not None) else None
    g = rand(B, L, Z, seed=seed + 3, dtype=dtype)
    out, avg_out = styles(s, L, s2, cut, avg, beta, PSI if tcut is not None else None, tcut)
    grads = torch.autograd.grad((out * g).sum(), [s] + ([s2] if s2 is not None else []), allow_unused=True)
    return dict(s=s.detach(), s2=None if s2 is None else s2.detach(), avg=avg, g=g, out=out.detach(), avg_out=avg_out,
                ds=grads[0] if grads[0] is not None else torch.zeros_like(s),
                ds2=None if s2 is None else (grads[1] if grads[1] is not None else torch.zeros_like(s2)))


def fp32_loss():
    """the worst figures of a float32 restatement against float64 over CASES and EDGE_CASES: (forward viol, gradient nerr)"""
    fwd = grad = 0.0
    for B, Z in CASES["pixel_norm"] + EDGE_CASES["pixel_norm"]:
        a, r = pn_case(B, Z, torch.float32), pn_case(B, Z)
        fwd, grad = max(fwd, viol(a["y"], r["y"])), max(grad, nerr(a["dx"], r["dx"], lead=r["lead"]))
    for B, K, N in CASES["linear"] + EDGE_CASES["linear"]:
        a, r = lin_case(B, K, N, torch.float32), lin_case(B, K, N)
        fwd = max(fwd, viol(a["y"], r["y"]))
        # (dz follows the sign of y: where float32 rounds a pre-activation across 0 the two restatements differ by design)
        same = (a["y"] > 0) == (r["y"] > 0)
        grad = max(grad, nerr(a["dz"] * same, r["dz"] * same), nerr(a["db"], r["db"], lead=float(r["g"].abs().max())))
    for shape, var in CASES["styles"] + EDGE_CASES["styles"]:
        a, r = st_case(shape, var, torch.float32), st_case(shape, var)
        fwd = max(fwd, viol(a["out"], r["out"]))
        if r["avg_out"] is not None:
            fwd = max(fwd, viol(a["avg_out"], r["avg_out"]))
        grad = max(grad, nerr(a["ds"], r["ds"], lead=float(r["g"].abs().max())))
        if r["ds2"] is not None:
            grad = max(grad, nerr(a["ds2"], r["ds2"], lead=float(r["g"].abs().max())))
    return fwd, grad


if __name__ == "__main__":
    f, g = fp32_loss()
    print("float32 restatement against float64 over %d cases: forward viol %.3g, gradient nerr %.3g -> gradient gate %.3g"
          % (sum(len(v) for v in itertools.chain(CASES.values(), EDGE_CASES.values())), f, g, min(4 * g, 1e-4)))
