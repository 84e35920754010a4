"""The style variant's optimizer and weight average (reference: style_soft_intro_vae/custom_adam.py, LREQAdam, and
model.py:320-329, the lerp towards the averaged model) on the multi-tensor kernels of csrc/multi_tensor.hip.

LREQAdam is Adam without a first moment (beta_1 = 0) whose step is scaled, per tensor, by that tensor's
`lr_equalization_coef`.  Everything the reference's training loop, LOD driver, scheduler and checkpointer touch is the
reference's: the constructor, the `param_groups` keys (lr, beta_2, eps, weight_decay), `state[p] = {'step': int,
'exp_avg_sq': tensor}`, so state dicts interchange with the reference's class.  `step()` keeps nothing between calls: the
state is looked up in `self.state` every time (the LOD driver replaces that dict on every LOD change), `group['lr']` is
read every time (the scheduler rewrites it), and gradients are whatever `.grad` holds now (`zero_grad` drops them).

float32 contiguous ROCm tensors of all groups go through ONE `ops.mt_lreq_adam` call; anything else (CPU tensors, other
dtypes, a non-contiguous parameter, gradient or state) takes the same five element-wise operations in torch, tensor by
tensor, which is also what runs without a GPU.  `last_step` says what the last call did.
"""
import math

import torch

__all__ = ["LREQAdam", "lerp_parameters"]


def _fusable(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and not t.is_sparse for t in tensors)


def _bump(params):
    # the kernels write through raw pointers: torch's version counter does not move, the packed weight operands of
    # the convolutions and linears are keyed on this generation as well
    from . import functional
    functional.bump_generation(params)


class LREQAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.0, 0.99), eps=1e-8, weight_decay=0):
        beta_2 = betas[1]
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 == betas[0]:
            raise ValueError("Invalid beta parameter at index 0: {}".format(betas[0]))
        if not 0.0 <= beta_2 < 1.0:
            raise ValueError("Invalid beta parameter at index 1: {}".format(beta_2))
        if weight_decay != 0:
            # (the reference's branch for it reads a `p.coef` attribute nothing sets; its training script passes 0)
            raise NotImplementedError("LREQAdam: weight_decay != 0 is not supported, got {}".format(weight_decay))
        super().__init__(params, dict(lr=lr, beta_2=beta_2, eps=eps, weight_decay=weight_decay))
        self.last_step = {"fused": 0, "fallback": 0, "launches": 0}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        fused = {}  # (device, beta_2, eps) -> ([p], [g], [v], [step size], [state]): one multi-tensor call each
        fallback = 0
        for group in self.param_groups:
            if group["weight_decay"] != 0:
                raise NotImplementedError("LREQAdam: weight_decay != 0 is not supported")
            beta_2, eps, lr = group["beta_2"], group["eps"], group["lr"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad
                if grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg_sq"] = torch.zeros_like(p)
                exp_avg_sq = state["exp_avg_sq"]
                step_size = lr * math.sqrt(1 - beta_2 ** (state["step"] + 1))
                if hasattr(p, "lr_equalization_coef"):
                    step_size *= p.lr_equalization_coef
                if _fusable(p, grad, exp_avg_sq) and p.device == grad.device == exp_avg_sq.device \
                        and p.shape == grad.shape == exp_avg_sq.shape:
                    # (its step count moves once the launch has been made: a refused call leaves the state as it was)
                    lists = fused.setdefault((p.device, beta_2, eps), ([], [], [], [], []))
                    for l, x in zip(lists, (p, grad, exp_avg_sq, step_size, state)):
                        l.append(x)
                    continue
                state["step"] += 1
                exp_avg_sq.mul_(beta_2).addcmul_(grad, grad, value=1 - beta_2)
                denom = exp_avg_sq.sqrt().add_(eps)
                p.addcdiv_(grad, denom, value=-step_size)
                fallback += 1
        launches = n_fused = 0
        if fused:
            from . import ops
            for (_, beta_2, eps), (ps, gs, vs, ss, states) in fused.items():
                launches += ops.mt_lreq_adam(ps, gs, vs, ss, beta_2, eps)
                for state in states:
                    state["step"] += 1
                _bump(ps)
                n_fused += len(ps)
        self.last_step = {"fused": n_fused, "fallback": fallback, "launches": launches}
        return loss


@torch.no_grad()
def lerp_parameters(params, other_params, weight):
    """p.lerp_(q, weight) for every pair (the loop body of the reference's model.py:328-329): one multi-tensor call for the
    float32 contiguous ROCm pairs, torch's lerp_ for the rest.  -> {"fused", "fallback", "launches"}"""
    params, other_params = list(params), list(other_params)
    if len(params) != len(other_params):
        raise ValueError("lerp_parameters: %d tensors against %d" % (len(params), len(other_params)))
    fused, fallback = {}, 0
    for p, q in zip(params, other_params):
        p, q = p.data, q.data
        if _fusable(p, q) and p.device == q.device and p.shape == q.shape:
            dst, src = fused.setdefault(p.device, ([], []))
            dst.append(p)
            src.append(q)
        else:
            p.lerp_(q, weight)
            fallback += 1
    launches = n_fused = 0
    if fused:
        from . import ops
        for dst, src in fused.values():
            launches += ops.mt_lerp_(dst, src, weight)
            n_fused += len(dst)
    _bump(params)
    return {"fused": n_fused, "fallback": fallback, "launches": launches}
