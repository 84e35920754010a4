#!/usr/bin/env python3
"""Times the 3-D encoder's last stage, ReLU -> BatchNorm1d -> max over the points, as the composition
(relu_bn_stats, relu_bn_apply, max_points_fwd; max_points_bwd, relu_bn_bwd) and as the fused form (relu_bn_stats,
relu_bn_max_fwd; relu_bn_max_bwd), on the GPU with HIP events in one process:

  stage    the last stage alone, forward + backward on [B, 512, N] at the tensor level (no autograd)
  encoder  models/vae.py::Encoder forward + backward (autograd included) with pointcloud.RELU_BN_MAX off and on

Method: 5 warm-up calls, then 5 rounds of 20 calls; a round's figure is the time of its 20 calls / 20;
min / median / max over the rounds.  The two forms alternate round by round, so both see the same state of the box.
The stage loop keeps its 134 MB tensor in the last-level cache between the calls; the encoder figure is the one to judge by.
Prints one JSON line (times in microseconds).

    python tools/bench_pointcloud.py [--batch 32] [--points 2048] [--z 128] [--rounds 5] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "soft-intro-vae-pytorch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from sivae_hip import pointcloud as PC  # noqa: E402
import soft_intro_vae_3d.models.vae as V  # noqa: E402


def alternating(fns, rounds, calls, warmup):
    """fns: {name: callable} -> {name: dict(min_us, median_us, max_us, rounds_us)}; the callables take turns per round"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    return {k: dict(min_us=round(min(v), 1), median_us=round(sorted(v)[len(v) // 2], 1), max_us=round(max(v), 1),
                    rounds_us=[round(x, 1) for x in v]) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--z", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pointcloud: needs a ROCm device (timings on a CPU would say nothing)")
    dev = torch.device("cuda:0")
    B, C, N = a.batch, 512, a.points
    g = torch.Generator().manual_seed(0)
    act = torch.randn(B, C, N, generator=g).to(dev)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.rand(C, generator=g) - 0.5).to(dev)
    gy = torch.randn(B, C, generator=g).to(dev)
    last = {}

    def composition():
        mean, invstd = PC.relu_bn_stats(act)
        vals, arg = PC.max_points_fwd(PC.relu_bn_apply(act, mean, invstd, gamma, beta))
        last["composition"] = (vals, arg) + PC.relu_bn_bwd(PC.max_points_bwd(gy, arg, N), act, mean, invstd, gamma)

    def fused():
        mean, invstd = PC.relu_bn_stats(act)
        vals, arg = PC.relu_bn_max_fwd(act, mean, invstd, gamma, beta)
        last["fused"] = (vals, arg) + PC.relu_bn_max_bwd(gy, arg, act, mean, invstd, gamma)

    res = dict(batch=B, channels=C, points=N, z=a.z, rounds=a.rounds, calls=a.calls, warmup=a.warmup,
               device=torch.cuda.get_device_name(0))
    res["stage"] = alternating(dict(composition=composition, fused=fused), a.rounds, a.calls, a.warmup)
    c, f = last["composition"], last["fused"]
    res["stage"]["forward_equal"] = bool(torch.equal(c[0], f[0]) and torch.equal(c[1], f[1]))
    res["stage"]["da_max_abs_diff"] = float((c[2] - f[2]).abs().max())
    res["stage"]["da_max_abs"] = float(c[2].abs().max())
    del last, c, f

    torch.manual_seed(0)
    enc = V.Encoder({"z_size": a.z, "model": {"E": {"use_bias": True, "relu_slope": 0.2}}}).to(dev).train()
    x = (torch.rand(B, 3, N, generator=g) - 0.5).to(dev)
    r1, r2 = torch.randn(B, a.z, generator=g).to(dev), torch.randn(B, a.z, generator=g).to(dev)

    def encoder(flag):
        def run():
            PC.RELU_BN_MAX = flag
            for p in enc.parameters():
                p.grad = None
            mu, logvar = enc(x)
            torch.autograd.backward((mu, logvar), (r1, r2))
        return run

    default = PC.RELU_BN_MAX
    try:
        res["encoder"] = alternating(dict(composition=encoder(False), fused=encoder(True)), a.rounds, a.calls,
                                     a.warmup)
    finally:
        PC.RELU_BN_MAX = default
    comp, fus = res["encoder"]["composition"], res["encoder"]["fused"]
    res["encoder"]["composition_spread_us"] = round(comp["max_us"] - comp["min_us"], 1)
    res["encoder"]["gain_us"] = round(comp["median_us"] - fus["median_us"], 1)
    res["encoder"]["fused_wins"] = bool(res["encoder"]["gain_us"] > res["encoder"]["composition_spread_us"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
