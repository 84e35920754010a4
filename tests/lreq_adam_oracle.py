"""float64 numpy restatement of the style variant's optimizer step and weight average (what sivae_hip.lreq_adam and
csrc/multi_tensor.hip compute), and the schedule of the recorded trajectory in tests/golden/lreq_adam.npz.

One step of one tensor with gradient g, in float64:

    v' = beta2 v + (1 - beta2) g g
    u  = lr sqrt(1 - beta2^step) coef  g / (sqrt(v') + eps)        (coef = 1 without an lr_equalization_coef)
    p' = p - u

A tensor without a gradient is skipped and keeps its step count; a tensor without state starts from step 0, v = 0.
The average: p' = p + w (q - p) for |w| < 0.5, else q - (q - p) (1 - w): the two forms agree in exact arithmetic, both
are kept so that the oracle takes the branch the float32 code takes.
"""
import numpy as np

# ---- the recorded trajectory (make_golden_lreq_adam.py runs the reference on it, the tests run the class on it) ----
SIZES = (1, 2, 3, 4, 5, 7, 33, 130, 1025, 8193)
GROUPS = ((0, 1, 2, 3, 4, 5), (6, 7, 8, 9))        # tensor indices per param group
COEFS = (None, 0.5, 1.0, None, 0.0721, 2.5, 0.0208, None, 1.0, 0.0147)  # lr_equalization_coef, None: the attribute is absent
STEPS = 12
RESET_BEFORE = 5                                    # the optimizer's state is thrown away before this step (1-based)
SNAPSHOTS = (1, 6, 12)
BETA2, EPS = 0.99, 1e-8
LR0 = 1.5e-3                                        # group 0: constant


def lr1(step):
    """group 1: rewritten before every step (1-based), as a scheduler does"""
    return 2e-3 * 0.85 ** (step - 1) * (0.1 if step <= 2 else 1.0)


def has_grad(step, t):
    """which tensors have a gradient at which step: every tensor misses some, none misses all"""
    return (step * 7 + t * 3) % 5 != 0 and not (t == 9 and step == 2)


def grad_exponent(step, t):
    """the step's gradient is a stored base gradient times 2^this (exact in both precisions)"""
    return ((step * 5 + t) % 3) - 1


def grad_of(base, step, t):
    """base: [2][tensor] arrays -> the gradient of tensor t at `step` (1-based) or None"""
    if not has_grad(step, t):
        return None
    return base[step % 2][t] * (2.0 ** grad_exponent(step, t))


def make_inputs(seed=20260):
    """-> (params [t], base gradients [2][t]) as float32 arrays; gradient magnitudes span 1e-3 .. 10 element by element"""
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    base = [[(rng.standard_normal(n) * 10.0 ** rng.uniform(-3.0, 0.7, n)).astype(np.float32) for n in SIZES]
            for _ in range(2)]
    return params, base


# ---- the arithmetic -----------------------------------------------------------------------------------------------
def step_size(lr, beta2, step, coef=None):
    s = lr * np.sqrt(1.0 - beta2 ** step)
    return s if coef is None else s * coef


def _f64(xp, *arrays):
    """numpy: float64 arrays; torch (xp = the torch module): the tensors must be float64 already"""
    if xp is np:
        return tuple(np.asarray(a, dtype=np.float64) for a in arrays)
    assert all(a.dtype == xp.float64 for a in arrays)
    return arrays


def step_tensor(p, v, g, s, beta2=BETA2, eps=EPS, xp=np):
    """-> (p', v', u) in float64 from float64 (or exactly widened float32) inputs; s: the step size.  xp: numpy, or torch
    to evaluate the same expressions on float64 tensors where they are (the large cases of the GPU tests)"""
    p, v, g = _f64(xp, p, v, g)
    with np.errstate(all="ignore"):
        v2 = beta2 * v + (1.0 - beta2) * (g * g)
        u = s * (g / (xp.sqrt(v2) + eps))
    return p - u, v2, u


def lerp(p, q, w, xp=np):
    p, q = _f64(xp, p, q)
    d = q - p
    return p + w * d if abs(w) < 0.5 else q - d * (1.0 - w)


class Optimizer:
    """the class's rules on lists of float64 arrays: groups with their own lr, lazy state, skipped tensors"""

    def __init__(self, params, groups=GROUPS, coefs=COEFS, beta2=BETA2, eps=EPS):
        self.p = [np.asarray(a, dtype=np.float64).copy() for a in params]
        self.groups, self.coefs, self.beta2, self.eps = groups, coefs, beta2, eps
        self.state = {}

    def reset(self):
        self.state = {}

    def step(self, grads, lrs):
        """grads: [tensor] arrays or None; lrs: one learning rate per group"""
        for group, lr in zip(self.groups, lrs):
            for t in group:
                if grads[t] is None:
                    continue
                st = self.state.setdefault(t, {"step": 0, "exp_avg_sq": np.zeros_like(self.p[t])})
                st["step"] += 1
                s = step_size(lr, self.beta2, st["step"], self.coefs[t])
                self.p[t], st["exp_avg_sq"], _ = step_tensor(self.p[t], st["exp_avg_sq"], grads[t], s, self.beta2, self.eps)

    def steps(self):
        return [self.state[t]["step"] if t in self.state else 0 for t in range(len(self.p))]

    def exp_avg_sq(self):
        return [self.state[t]["exp_avg_sq"] if t in self.state else np.zeros_like(self.p[t]) for t in range(len(self.p))]


def run_schedule(stepper, first=1, last=STEPS, reset=None):
    """drives `stepper(step, lrs)` over the recorded schedule; `reset()` is called before step RESET_BEFORE"""
    for k in range(first, last + 1):
        if k == RESET_BEFORE and reset is not None:
            reset()
        stepper(k, (LR0, lr1(k)))


def trajectory(params, base):
    """-> {snapshot step: (params, exp_avg_sq, step counts)} of the oracle over the recorded schedule"""
    opt, out = Optimizer(params), {}

    def stepper(k, lrs):
        opt.step([grad_of(base, k, t) for t in range(len(SIZES))], lrs)
        if k in SNAPSHOTS:
            out[k] = ([a.copy() for a in opt.p], [a.copy() for a in opt.exp_avg_sq()], opt.steps())

    run_schedule(stepper, reset=opt.reset)
    return out


def run_class(cls, params0, base, dtype, device="cpu", first=1, last=STEPS, resume=None, after_step=None):
    """An LREQAdam class (the reference's or sivae_hip's) over steps first .. last of the recorded schedule on torch tensors
    of `dtype` -> ({snapshot step: (params, exp_avg_sq, step counts)} as float64 arrays, the optimizer, the parameters).
    resume = (params, exp_avg_sq, step counts): start from that state, handed over through load_state_dict.
    after_step(k, optimizer) is called after every step."""
    import collections

    import torch
    start = params0 if resume is None else resume[0]
    ps = []
    for t, a in enumerate(start):
        p = torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dtype).to(device))
        if COEFS[t] is not None:
            p.lr_equalization_coef = COEFS[t]
        ps.append(p)
    opt = cls([{"params": [ps[t] for t in GROUPS[0]], "lr": LR0}, {"params": [ps[t] for t in GROUPS[1]]}],
              lr=lr1(1), betas=(0.0, BETA2), eps=EPS, weight_decay=0)
    if resume is not None:
        sd = opt.state_dict()
        order = [t for g in GROUPS for t in g]  # (state_dict numbers the parameters group by group)
        sd["state"] = {i: {"step": int(resume[2][t]), "exp_avg_sq": torch.from_numpy(np.array(resume[1][t])).to(dtype)}
                       for i, t in enumerate(order) if resume[2][t] > 0}
        opt.load_state_dict(sd)
    out = {}

    def snapshot():
        has = [len(opt.state[p]) > 0 for p in ps]
        return ([p.detach().double().cpu().numpy().copy() for p in ps],
                [opt.state[p]["exp_avg_sq"].double().cpu().numpy().copy() if h else np.zeros(p.shape) for p, h in zip(ps, has)],
                [int(opt.state[p]["step"]) if h else 0 for p, h in zip(ps, has)])

    def stepper(k, lrs):
        opt.param_groups[1]["lr"] = lrs[1]
        for t, p in enumerate(ps):
            g = grad_of(base, k, t)
            p.grad = None if g is None else torch.from_numpy(np.asarray(g)).to(dtype).to(device)
        opt.step()
        if after_step is not None:
            after_step(k, opt)
        if k in SNAPSHOTS:
            out[k] = snapshot()

    def reset():  # (what the reference's lod_driver does on every LOD change)
        opt.state = collections.defaultdict(dict)

    run_schedule(stepper, first, last, reset)
    return out, opt, ps


def rel_dev(a, b):
    """max-norm relative deviation of a from b"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))
