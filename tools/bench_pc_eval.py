#!/usr/bin/env python3
"""Times the all-pairs Chamfer matrix behind MMD-CD / COV-CD (`sivae_hip.pointcloud.chamfer_matrix`, csrc/pc_eval.hip) on
the GPU with HIP events, against what the engine offered before it: one `chamfer_fwd` call per sample row,

    pointcloud.chamfer_fwd(sample[s:s+1].expand(R, M, 3).contiguous(), ref)[0]      # = row s of D, normalize=False

Steps (each one process of its own under `timeout`; the driver itself never touches the GPU and stops at the first step
that fails):

  ab     240 x 800 clouds of 2048 points (10 % of the 2400 + 800 clouds tools/bench_jsd.py uses): one warm-up call of each
         form, then 5 rounds of one call each, the two forms alternating round by round, so both see the same state of
         the box.  Also: the largest relative difference between the two on the rows both computed, match_min's time.
  full   the whole 2400 x 800 matrix ONCE with the new op only, each launch timed (the longest single launch is what
         pointcloud.MATRIX_POINT_PAIRS_PER_LAUNCH bounds), then match_min.

  self   1-NN accuracy's matrices, run on its own (the driver does not start it): 240 clouds of 2048 points,
         `chamfer_matrix(x, x)` against `chamfer_matrix_self(x)` (the pairs i <= j by folded rows, mirrored), one warm-up
         call of each, then 5 rounds alternating; the two results must be equal bit for bit.  Also: the longest single
         launch of the self form, and `nn1_loo` on random matrices at S = 2400, R = 800.  Its raw line goes to
         profiles/pc_eval_self_bench.txt.

Each step prints one JSON line; the driver appends the raw lines to profiles/pc_eval_bench.txt.

    python tools/bench_pc_eval.py [--out profiles/pc_eval_bench.txt]        # the driver: ab and full
    python tools/bench_pc_eval.py --step ab [--sample 240] [--ref 800] [--points 2048] [--rounds 5]
    python tools/bench_pc_eval.py --step full [--sample 2400] [--ref 800] [--points 2048]
    python tools/bench_pc_eval.py --step self [--sample 240] [--points 2048] [--rounds 5] [--out profiles/pc_eval_self_bench.txt]
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

STEP_TIMEOUT_S = {"ab": 240, "full": 180}  # (the driver's steps)


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
    """distances per second, and the fp32 VALU issue slots (one lane, one instruction; 64 lanes per CU and clock) the
    device has per distance at the clock given with --clock-mhz"""
    dist = float(S) * R * M * N
    res["distances"] = dist
    res["distances_per_s"] = dist / (ms * 1e-3)
    res["valu_lane_slots_per_distance_at_clock"] = round(cus * 64 * res["clock_mhz"] * 1e6 / res["distances_per_s"], 3)


def step_ab(a):
    import torch
    from sivae_hip import pointcloud as PC
    S = a.sample if a.sample else 240
    sample, ref = _inputs(torch, a, S)
    R, M = a.ref, a.points

    def new():
        return PC.chamfer_matrix(sample, ref, normalize=False)

    def baseline():
        return torch.stack([PC.chamfer_fwd(sample[s:s + 1].expand(R, M, 3).contiguous(), ref)[0] for s in range(S)])

    D1, D0 = new(), baseline()  # (warm-up)
    torch.cuda.synchronize()
    rel = float(((D1.double() - D0.double()).abs() / D0.double()).max())
    ms = dict(new=[], baseline=[])
    for _ in range(a.rounds):
        for name, fn in (("new", new), ("baseline", baseline)):
            ms[name].append(_timed(torch, fn)[1])
    mm = [_timed(torch, lambda: PC.match_min(D1))[1] for _ in range(a.rounds + 1)][1:]
    res = dict(step="ab", sample=S, ref=R, points=M, rounds=a.rounds, clock_mhz=a.clock_mhz, **_device(torch))
    res["new"], res["baseline"], res["match_min"] = _stats(ms["new"]), _stats(ms["baseline"]), _stats(mm)
    res["max_rel_diff_new_vs_baseline"] = rel
    spread = res["baseline"]["max_ms"] - res["baseline"]["min_ms"]
    res["baseline_spread_ms"] = round(spread, 3)
    res["gain_ms"] = round(res["baseline"]["median_ms"] - res["new"]["median_ms"], 3)
    res["new_wins"] = bool(res["gain_ms"] > spread)
    res["speedup_of_medians"] = round(res["baseline"]["median_ms"] / res["new"]["median_ms"], 2)
    _rates(res, S, R, M, M, res["new"]["median_ms"], res["compute_units"])
    print(json.dumps(res))


def step_full(a):
    import torch
    from sivae_hip import pointcloud as PC
    S = a.sample if a.sample else 2400
    sample, ref = _inputs(torch, a, S)
    PC.chamfer_matrix(sample[:8], ref[:8])  # (loads the library and the kernel; 64 cloud pairs)
    torch.cuda.synchronize()
    launches = []
    real = PC._lib.call

    def call(name, *args):
        if name != "sivae_chamfer_matrix":
            return real(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = real(name, *args)
        e1.record()
        launches.append((e0, e1))
        return rc

    PC._lib.call = call
    try:
        D, ms = _timed(torch, lambda: PC.chamfer_matrix(sample, ref))
    finally:
        PC._lib.call = real
    per_launch = [e0.elapsed_time(e1) for e0, e1 in launches]
    (_, _, col_min, _), mm_ms = _timed(torch, lambda: PC.match_min(D))
    res = dict(step="full", sample=S, ref=a.ref, points=a.points, clock_mhz=a.clock_mhz, **_device(torch))
    res.update(matrix_ms=round(ms, 3), launches=len(per_launch), longest_launch_ms=round(max(per_launch), 3),
               launch_ms=[round(v, 3) for v in per_launch], match_min_ms=round(mm_ms, 3),
               point_pairs_per_launch=PC.MATRIX_POINT_PAIRS_PER_LAUNCH, finite=bool(torch.isfinite(D).all()),
               mmd=float(col_min.double().mean()))
    _rates(res, S, a.ref, a.points, a.points, ms, res["compute_units"])
    print(json.dumps(res))


def step_self(a):
    import torch
    from sivae_hip import pointcloud as PC
    S = a.sample if a.sample else 240
    x = _inputs(torch, a, S)[0]
    M = a.points
    launches = []
    real = PC._lib.call

    def call(name, *args):
        if name != "sivae_chamfer_matrix_self":
            return real(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = real(name, *args)
        e1.record()
        launches.append((e0, e1))
        return rc

    def full():
        return PC.chamfer_matrix(x, x, normalize=False)

    def self_():
        return PC.chamfer_matrix_self(x, normalize=False)

    D0, D1 = full(), self_()  # (warm-up)
    torch.cuda.synchronize()
    ms = dict(full=[], self=[])
    PC._lib.call = call
    try:
        for _ in range(a.rounds):
            for name, fn in (("full", full), ("self", self_)):
                ms[name].append(_timed(torch, fn)[1])
    finally:
        PC._lib.call = real
    per_launch = [e0.elapsed_time(e1) for e0, e1 in launches]
    # nn1_loo at the protocol's sizes, on random matrices (it reads (S + R)^2 words once)
    g = torch.Generator().manual_seed(1)
    Sn, Rn = 2400, a.ref
    Dss, Dsr, Drr = (torch.rand(r, c, generator=g).to(x.device) for r, c in ((Sn, Sn), (Sn, Rn), (Rn, Rn)))
    nn = [_timed(torch, lambda: PC.nn1_loo(Dss, Dsr, Drr))[1] for _ in range(a.rounds + 1)][1:]
    res = dict(step="self", clouds=S, points=M, rounds=a.rounds, clock_mhz=a.clock_mhz, **_device(torch))
    res["full"], res["self"], res["nn1_loo"] = _stats(ms["full"]), _stats(ms["self"]), _stats(nn)
    res["nn1_loo_sizes"] = [Sn, Rn]
    res["equal_bit_for_bit"] = bool(torch.equal(D0, D1))
    res["ratio_of_medians"] = round(res["self"]["median_ms"] / res["full"]["median_ms"], 4)
    res["ratio_by_pair_count"] = round((S + 1) / (2.0 * S), 4)
    res["launches_per_call"] = len(per_launch) // a.rounds
    res["longest_launch_ms"] = round(max(per_launch), 3)
    res["point_pairs_per_launch"] = PC.MATRIX_POINT_PAIRS_PER_LAUNCH
    _rates(res, S, (S + 1) / 2.0, M, M, res["self"]["median_ms"], res["compute_units"])
    print(json.dumps(res))
    out = a.out if os.path.isabs(a.out) else os.path.join(REPO, a.out)
    with open(out, "a") as f:
        f.write(json.dumps(res) + "\n")


def drive(a):
    out = a.out if os.path.isabs(a.out) else os.path.join(REPO, a.out)
    for step in ("ab", "full"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--ref", str(a.ref), "--points", str(a.points), "--rounds", str(a.rounds), "--clock-mhz", str(a.clock_mhz)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            raise SystemExit("bench_pc_eval: step %s ended with status %d; nothing further is started" % (step, p.returncode))
        with open(out, "a") as f:
            f.write(p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("ab", "full", "self"))
    ap.add_argument("--sample", type=int, default=0, help="sample clouds (default: 240 for ab, 2400 for full)")
    ap.add_argument("--ref", type=int, default=800)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock the VALU issue rate is quoted at")
    ap.add_argument("--out", default=None, help="raw lines: profiles/pc_eval_bench.txt, pc_eval_self_bench.txt for --step self")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join("profiles", "pc_eval_self_bench.txt" if a.step == "self" else "pc_eval_bench.txt")
    if a.step is None:
        return drive(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pc_eval: needs a ROCm device (timings on a CPU would say nothing)")
    dict(ab=step_ab, full=step_full, self=step_self)[a.step](a)


if __name__ == "__main__":
    main()
