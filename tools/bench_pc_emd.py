#!/usr/bin/env python3
"""Times the all-pairs earth mover's matrix behind MMD-EMD / COV-EMD (`sivae_hip.pointcloud.emd_matrix`, csrc/pc_emd.hip)
on the GPU with HIP events.  The only comparator there is (no earlier form of the op exists) is a plain torch restatement
of the ten levels on the same device in the same process, batched over the reference clouds:

    w = exp(level * d2);  ratioL = remL / (1e-9 + (w * remR).sum(2));  ...           # [pairs, N, M] tensors, ~15 passes a level

Steps (each one process of its own under `timeout`; the driver itself never touches the GPU and stops at the first step
that fails):

  ab     240 x 800 clouds of 2048 points: one warm-up call, then 5 rounds of one call of the op, each launch timed.  The
         torch restatement cannot take 192 000 cloud pairs in any reasonable time (it moves about 2.5 GB a pair), so it
         is timed on the first --baseline-pairs pairs of row 0, alternating with the op ON THE SAME PAIRS round by round;
         the two are compared on those pairs (values, too) and the whole-matrix figure of the restatement is an
         extrapolation, reported as one.
  slab   64 x 64 clouds of 2048 points, 5 rounds, each launch timed: launches of whole rows, exactly as many cloud pairs as
         EMD_POINT_PAIRS_PER_LAUNCH allows (at 800 reference clouds a row is longer than that and goes in two unequal
         blocks of columns).
  full   the whole 2400 x 800 matrix ONCE, each launch timed (the longest single launch is what
         pointcloud.EMD_POINT_PAIRS_PER_LAUNCH bounds).

  loss   NOT part of the driver: the reconstruction loss `pointcloud.emd_distance` (emd_loss_kernel), 32 pairs of 2048-point
         clouds.  (a) forward + backward with the gradient of the second argument only, as training asks, alternating
         round by round with the torch restatement ON THE SAME PAIRS, its plan detached and autograd on; (b) the cost of
         the gradients: emd_matrix over 32 cloud pairs of the same sizes (one sample cloud against the 32 left clouds, one
         launch), then emd_loss_fwd with no gradient, with dright, with both, every launch timed; (c) the longest launch
         EMD_LOSS_POINT_PAIRS_PER_LAUNCH allows at this size (256 pairs of 2048 points, both gradients).  It appends its
         line to its own file, profiles/pc_emd_loss_bench.txt (--loss-out).

Each step prints one JSON line; the driver appends the raw lines to profiles/pc_emd_bench.txt.

    python tools/bench_pc_emd.py [--out profiles/pc_emd_bench.txt]        # the driver: all three steps
    python tools/bench_pc_emd.py --step ab [--sample 240] [--ref 800] [--points 2048] [--rounds 5] [--baseline-pairs 32]
    python tools/bench_pc_emd.py --step slab [--points 2048] [--rounds 5]
    python tools/bench_pc_emd.py --step full [--sample 2400] [--ref 800] [--points 2048]
    python tools/bench_pc_emd.py --step loss [--pairs 32] [--points 2048] [--rounds 5] [--loss-out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "soft-intro-vae-pytorch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

STEP_TIMEOUT_S = {"ab": 300, "slab": 120, "full": 420}
SWEEPS = 30  # three sweeps over all point pairs in each of the ten levels


def _stats(ms):
    return dict(min_ms=round(min(ms), 3), median_ms=round(sorted(ms)[len(ms) // 2], 3), max_ms=round(max(ms), 3),
                rounds_ms=[round(v, 3) for v in ms])


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def _inputs(torch, a, sample):
    g = torch.Generator().manual_seed(0)
    dev = torch.device("cuda:0")
    return ((torch.rand(sample, a.points, 3, generator=g) - 0.5).to(dev),
            (torch.rand(a.ref, a.points, 3, generator=g) - 0.5).to(dev))


def _device(torch):
    p = torch.cuda.get_device_properties(0)
    return dict(device=p.name, compute_units=p.multi_processor_count)


def _rates(res, S, R, M, N, ms, cus):
    """point pairs (each visited in 30 sweeps) and weights (one exponential each) per second, and the fp32 VALU issue slots
    (one lane, one instruction; 64 lanes per CU and clock) the device has per weight at the clock given with --clock-mhz"""
    pairs = float(S) * R * M * N
    res["point_pairs"] = pairs
    res["cloud_pairs_per_s"] = float(S) * R / (ms * 1e-3)
    res["point_pairs_per_s"] = pairs / (ms * 1e-3)
    res["weights_per_s"] = SWEEPS * pairs / (ms * 1e-3)
    res["valu_lane_slots_per_weight_at_clock"] = round(cus * 64 * res["clock_mhz"] * 1e6 / res["weights_per_s"], 3)


def torch_emd(torch, sample, ref, normalize=True, detach_plan=False):
    """the ten levels in plain torch ops: sample [M, 3] or [P, M, 3] (right), ref [P, N, 3] (left) -> [P] float32.
    detach_plan: the levels run without autograd and the cost is sum(plan * dist) with the plan a constant, so that
    autograd yields matchcostgrad's gradient (what emd_distance returns)"""
    P, n, m = ref.shape[0], ref.shape[1], sample.shape[-2]
    right = sample if sample.dim() == 3 else sample[None]
    diff = ref[:, :, None, :] - right[:, None, :, :]                           # [P, n, m, 3]
    d2 = diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1] + diff[..., 2] * diff[..., 2]
    del diff
    dist = d2.sqrt()
    big = float(max(n, m))
    cost = torch.zeros(P, dtype=torch.float64, device=ref.device)
    with torch.set_grad_enabled(torch.is_grad_enabled() and not detach_plan):
        if detach_plan:
            d2, plan = d2.detach(), torch.zeros_like(d2)
        remL = torch.full((P, n), big / n, dtype=torch.float32, device=ref.device)
        remR = torch.full((P, m), big / m, dtype=torch.float32, device=ref.device)
        for j in range(7, -3, -1):
            w = torch.exp(d2 * (-(4.0 ** j) if j > -2 else 0.0))
            ratioL = remL / (1e-9 + (w * remR[:, None, :]).sum(2))
            sumr = remR * (w * ratioL[:, :, None]).sum(1)
            ratioR = remR * torch.clamp(remR / (sumr + 1e-9), max=1.0)
            remR = torch.clamp(remR - sumr, min=0.0)
            w = w * ratioL[:, :, None] * ratioR[:, None, :]                    # (the plan of this level)
            if detach_plan:
                plan += w
            else:
                cost += (w * dist).sum((1, 2), dtype=torch.float64)
            remL = torch.clamp(remL - w.sum(2), min=0.0)
    if detach_plan:
        cost = (plan * dist).sum((1, 2), dtype=torch.float64)
    return (cost / big if normalize else cost).float()


def _time_launches(torch, PC, fn, entry="sivae_emd_matrix"):
    """-> (result, total ms, [ms of each launch of `entry`])"""
    launches = []
    real = PC._lib.call

    def call(name, *args):
        if name != entry:
            return real(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = real(name, *args)
        e1.record()
        launches.append((e0, e1))
        return rc

    PC._lib.call = call
    try:
        out, ms = _timed(torch, fn)
    finally:
        PC._lib.call = real
    return out, ms, [e0.elapsed_time(e1) for e0, e1 in launches]


def step_ab(a):
    import torch
    from sivae_hip import pointcloud as PC
    S = a.sample if a.sample else 240
    sample, ref = _inputs(torch, a, S)
    R, M, P = a.ref, a.points, min(a.baseline_pairs, a.ref)

    def new():
        return PC.emd_matrix(sample, ref)

    def new_sub():
        return PC.emd_matrix(sample[:1], ref[:P])[0]

    def baseline_sub():
        return torch_emd(torch, sample[0], ref[:P])

    D1, d1, d0 = new(), new_sub(), baseline_sub()  # (warm-up of every timed form)
    torch.cuda.synchronize()
    rel = float(((d1.double() - d0.double()).abs() / d0.double()).max())
    same = bool(torch.equal(D1[0, :P], d1))
    ms, longest, sub = [], [], dict(new=[], baseline=[])
    for _ in range(a.rounds):
        _, t, per_launch = _time_launches(torch, PC, new)
        ms.append(t)
        longest.append(max(per_launch))
        for name, fn in (("new", new_sub), ("baseline", baseline_sub)):
            sub[name].append(_timed(torch, fn)[1])
    res = dict(step="ab", sample=S, ref=R, points=M, rounds=a.rounds, clock_mhz=a.clock_mhz, **_device(torch))
    res["new"] = _stats(ms)
    res["launches"] = len(per_launch)
    res["longest_launch"] = _stats(longest)
    res["point_pairs_per_launch"] = PC.EMD_POINT_PAIRS_PER_LAUNCH
    res["baseline_pairs"] = P
    res["new_on_baseline_pairs"], res["torch_on_baseline_pairs"] = _stats(sub["new"]), _stats(sub["baseline"])
    res["max_rel_diff_new_vs_torch"] = rel
    res["slab_of_row_0_bit_equal_to_whole"] = same
    spread = res["torch_on_baseline_pairs"]["max_ms"] - res["torch_on_baseline_pairs"]["min_ms"]
    res["torch_spread_ms"] = round(spread, 3)
    res["gain_ms_on_baseline_pairs"] = round(res["torch_on_baseline_pairs"]["median_ms"]
                                             - res["new_on_baseline_pairs"]["median_ms"], 3)
    res["new_wins"] = bool(res["gain_ms_on_baseline_pairs"] > spread)
    # the subset is smaller than one wave of blocks: the whole-matrix ratio is the one to quote
    res["torch_whole_matrix_ms_extrapolated"] = round(res["torch_on_baseline_pairs"]["median_ms"] * S * R / P, 1)
    res["speedup_whole_matrix_extrapolated"] = round(res["torch_whole_matrix_ms_extrapolated"] / res["new"]["median_ms"], 1)
    _rates(res, S, R, M, M, res["new"]["median_ms"], res["compute_units"])
    print(json.dumps(res))


def step_slab(a):
    import torch
    from sivae_hip import pointcloud as PC
    S = R = 64
    a.ref = R
    sample, ref = _inputs(torch, a, S)
    PC.emd_matrix(sample, ref)  # (warm-up)
    torch.cuda.synchronize()
    ms, per_launch = [], []
    for _ in range(a.rounds):
        _, t, launches = _time_launches(torch, PC, lambda: PC.emd_matrix(sample, ref))
        ms.append(t)
        per_launch += launches
    res = dict(step="slab", sample=S, ref=R, points=a.points, rounds=a.rounds, clock_mhz=a.clock_mhz, **_device(torch))
    res.update(matrix=_stats(ms), launches_per_call=len(per_launch) // a.rounds,
               cloud_pairs_per_launch=max(1, min(S, PC.EMD_POINT_PAIRS_PER_LAUNCH // (R * a.points * a.points))) * R,
               point_pairs_per_launch=PC.EMD_POINT_PAIRS_PER_LAUNCH, launch=_stats(per_launch))
    del res["launch"]["rounds_ms"]
    _rates(res, S, R, a.points, a.points, res["matrix"]["median_ms"], res["compute_units"])
    print(json.dumps(res))


def step_full(a):
    import torch
    from sivae_hip import pointcloud as PC
    S = a.sample if a.sample else 2400
    sample, ref = _inputs(torch, a, S)
    PC.emd_matrix(sample[:8], ref[:8])  # (loads the library and the kernel; 64 cloud pairs)
    torch.cuda.synchronize()
    D, ms, per_launch = _time_launches(torch, PC, lambda: PC.emd_matrix(sample, ref))
    (_, _, col_min, _), mm_ms = _timed(torch, lambda: PC.match_min(D))
    res = dict(step="full", sample=S, ref=a.ref, points=a.points, clock_mhz=a.clock_mhz, **_device(torch))
    res.update(matrix_ms=round(ms, 3), launches=len(per_launch), longest_launch_ms=round(max(per_launch), 3),
               median_launch_ms=round(sorted(per_launch)[len(per_launch) // 2], 3),
               shortest_launch_ms=round(min(per_launch), 3), match_min_ms=round(mm_ms, 3),
               point_pairs_per_launch=PC.EMD_POINT_PAIRS_PER_LAUNCH, finite=bool(torch.isfinite(D).all()),
               mmd=float(col_min.double().mean()))
    _rates(res, S, a.ref, a.points, a.points, ms, res["compute_units"])
    print(json.dumps(res))


def step_loss(a):
    import torch
    from sivae_hip import pointcloud as PC
    B, n = a.pairs, a.points
    g = torch.Generator().manual_seed(0)
    dev = torch.device("cuda:0")
    gts = (torch.rand(B, n, 3, generator=g) - 0.5).to(dev)        # the loss's first argument (left), no gradient
    rec = (torch.rand(B, n, 3, generator=g) - 0.5).to(dev)        # its second (right): the decoder's output

    def fwd_bwd(loss_of):
        x = rec.clone().requires_grad_(True)
        loss_of(gts, x).sum().backward()
        return x.grad

    def new():
        return fwd_bwd(lambda l, r: PC.emd_distance(l, r))

    def baseline():
        return fwd_bwd(lambda l, r: torch_emd(torch, r, l, normalize=False, detach_plan=True))

    g1, g0 = new(), baseline()  # (warm-up of both forms)
    torch.cuda.synchronize()
    rel = float((g1.double() - g0.double()).abs().max() / g0.double().abs().max())
    ab = dict(new=[], baseline=[])
    for _ in range(a.rounds):
        for name, fn in (("new", new), ("baseline", baseline)):
            ab[name].append(_timed(torch, fn)[1])
    res = dict(step="loss", pairs=B, points=n, rounds=a.rounds, **_device(torch))
    res["fwd_bwd_dright_only"], res["torch_plan_detached_fwd_bwd"] = _stats(ab["new"]), _stats(ab["baseline"])
    spread = res["torch_plan_detached_fwd_bwd"]["max_ms"] - res["torch_plan_detached_fwd_bwd"]["min_ms"]
    res["torch_spread_ms"] = round(spread, 3)
    res["gain_ms"] = round(res["torch_plan_detached_fwd_bwd"]["median_ms"] - res["fwd_bwd_dright_only"]["median_ms"], 3)
    res["new_wins"] = bool(res["gain_ms"] > spread)
    res["speedup"] = round(res["torch_plan_detached_fwd_bwd"]["median_ms"] / res["fwd_bwd_dright_only"]["median_ms"], 1)
    res["max_rel_diff_dright_new_vs_torch_autograd"] = rel
    # the cost of the gradients, every launch timed
    forms = (("emd_matrix_1x%d" % B, "sivae_emd_matrix", lambda: PC.emd_matrix(rec[:1], gts, normalize=False)),
             ("cost_only", "sivae_emd_loss", lambda: PC.emd_loss_fwd(gts, rec, False, False)),
             ("with_dright", "sivae_emd_loss", lambda: PC.emd_loss_fwd(gts, rec, False, True)),
             ("with_both", "sivae_emd_loss", lambda: PC.emd_loss_fwd(gts, rec, True, True)))
    times = {name: [] for name, _, _ in forms}
    for name, _, fn in forms:
        fn()  # (warm-up)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, entry, fn in forms:
            _, _, per_launch = _time_launches(torch, PC, fn, entry)
            times[name] += per_launch
    res["launch_ms"] = {name: _stats(v) for name, v in times.items()}
    # the longest launch the cap allows at this size: one cloud pair on every compute unit, both gradients
    full = max(1, PC.EMD_LOSS_POINT_PAIRS_PER_LAUNCH // (n * n))
    gts_full, rec_full = gts.repeat((full + B - 1) // B, 1, 1)[:full], rec.repeat((full + B - 1) // B, 1, 1)[:full]
    PC.emd_loss_fwd(gts_full, rec_full, True, True)
    torch.cuda.synchronize()
    full_ms = []
    for _ in range(a.rounds):
        full_ms += _time_launches(torch, PC, lambda: PC.emd_loss_fwd(gts_full, rec_full, True, True), "sivae_emd_loss")[2]
    res["full_round"] = dict(pairs=full, launches_per_call=len(full_ms) // a.rounds, with_both=_stats(full_ms))
    res["launches_per_call"] = {name: len(v) // a.rounds for name, v in times.items()}
    res["longest_launch_ms"] = round(max(full_ms), 3)
    res["point_pairs_per_launch"] = PC.EMD_LOSS_POINT_PAIRS_PER_LAUNCH
    print(json.dumps(res))
    out = a.loss_out if os.path.isabs(a.loss_out) else os.path.join(REPO, a.loss_out)
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")


def drive(a):
    out = a.out if os.path.isabs(a.out) else os.path.join(REPO, a.out)
    for step in ("ab", "slab", "full"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--ref", str(a.ref), "--points", str(a.points), "--rounds", str(a.rounds), "--clock-mhz", str(a.clock_mhz),
               "--baseline-pairs", str(a.baseline_pairs)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            raise SystemExit("bench_pc_emd: step %s ended with status %d; nothing further is started" % (step, p.returncode))
        with open(out, "a") as f:
            f.write(p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("ab", "slab", "full", "loss"))
    ap.add_argument("--sample", type=int, default=0, help="sample clouds (default: 240 for ab, 2400 for full)")
    ap.add_argument("--ref", type=int, default=800)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--baseline-pairs", type=int, default=32, help="cloud pairs the torch restatement is timed on")
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock the VALU issue rate is quoted at")
    ap.add_argument("--out", default=os.path.join("profiles", "pc_emd_bench.txt"))
    ap.add_argument("--pairs", type=int, default=32, help="cloud pairs of the loss step (a training batch)")
    ap.add_argument("--loss-out", default=os.path.join("profiles", "pc_emd_loss_bench.txt"))
    a = ap.parse_args()
    if a.step is None:
        return drive(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pc_emd: needs a ROCm device (timings on a CPU would say nothing)")
    dict(ab=step_ab, slab=step_slab, full=step_full, loss=step_loss)[a.step](a)


if __name__ == "__main__":
    main()
