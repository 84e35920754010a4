#!/usr/bin/env python3
"""Times the 3-D variant's validation metric, `metrics.jsd.jsd_between_point_cloud_sets`, on the GPU with HIP events:
S = 2400 sample clouds against 800 reference clouds of 2048 points, voxels = 28 (the shape of one trial of the
reference's calc_jsd_valid on a class with 800 validation clouds), on two inputs

  cube     uniform in the unit cube: about half of the points lie outside the clipped grid's cells and take the
           exhaustive route
  sphere   the same draws scaled into the sphere per cloud (0.45 x / max |x|): the lookup route dominates

and, in the same process, a stock-torch composition of the same result on the same device: chunked torch.cdist against
the cell table, argmin, bincount, then the divergence in float64 torch ops.  Prints one JSON line.

    python tools/bench_jsd.py [--sample 2400] [--ref 800] [--points 2048] [--voxels 28] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "soft-intro-vae-pytorch_amd")
for p in (PKG, os.path.join(PKG, "soft_intro_vae_3d")):
    if p not in sys.path:
        sys.path.insert(0, p)

from metrics.jsd import jsd_between_point_cloud_sets  # noqa: E402  (the drop-in, as the training script imports it)
from sivae_hip import pointcloud as PC  # noqa: E402


def timed(fn, reps):
    """-> (last result, median ms over reps, all ms); one warm-up call first.  Both columns (the engine and the torch
    composition) are timed by this function with the same number of repetitions"""
    fn()
    torch.cuda.synchronize()
    ms = []
    out = None
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, sorted(ms)[len(ms) // 2], ms


def torch_counters(pcs, cells, chunk=32768):
    flat = pcs.reshape(-1, 3)
    counters = torch.zeros(cells.shape[0], dtype=torch.int64, device=pcs.device)
    for i in range(0, flat.shape[0], chunk):
        idx = torch.cdist(flat[i:i + chunk], cells).argmin(dim=1)
        counters += torch.bincount(idx, minlength=cells.shape[0])
    return counters


def torch_jsd(sample, ref, cells):
    def h(p):
        nz = p[p > 0]
        return -(nz * torch.log2(nz)).sum()

    P, Q = torch_counters(sample, cells).double(), torch_counters(ref, cells).double()
    P, Q = P / P.sum(), Q / Q.sum()
    return float(h((P + Q) / 2.0) - (h(P) + h(Q)) / 2.0), P, Q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=2400)
    ap.add_argument("--ref", type=int, default=800)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--voxels", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jsd: needs a ROCm device (timings on a CPU would say nothing)")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    cube_s = (torch.rand(a.sample, a.points, 3, generator=g) - 0.5).to(dev)
    cube_r = (torch.rand(a.ref, a.points, 3, generator=g) - 0.5).to(dev)

    def into_sphere(x):
        return x * (0.45 / x.norm(dim=2).amax(dim=1))[:, None, None]

    cells = PC.device_grid(dev, a.voxels, True)[0]
    res = dict(sample=a.sample, ref=a.ref, points=a.points, voxels=a.voxels, cells=int(cells.shape[0]), reps=a.reps)
    for name, s, r in (("cube", cube_s, cube_r), ("sphere", into_sphere(cube_s), into_sphere(cube_r))):
        ours, ms, all_ms = timed(lambda: jsd_between_point_cloud_sets(s, r, voxels=a.voxels), a.reps)
        # the decoder's layout: [S, 3, N] storage read through its transposed view
        st = s.permute(0, 2, 1).contiguous().transpose(1, 2)
        ours_t, ms_t, _ = timed(lambda: jsd_between_point_cloud_sets(st, r, voxels=a.voxels), a.reps)
        (theirs, P, _), ms_torch, all_torch = timed(lambda: torch_jsd(s, r, cells), a.reps)
        cs, _, status = PC.occupancy_grid(s, a.voxels, True, want_bernoulli=False, return_status=True)
        cr, _, status_r = PC.occupancy_grid(r, a.voxels, True, want_bernoulli=False, return_status=True)
        n_pts = (a.sample + a.ref) * a.points
        res[name] = dict(
            hip_ms=round(ms, 3), hip_ms_all=[round(v, 3) for v in all_ms], hip_transposed_view_ms=round(ms_t, 3),
            torch_ms=round(ms_torch, 3), torch_ms_all=[round(v, 3) for v in all_torch], jsd_hip=float(ours),
            jsd_hip_transposed_view=float(ours_t), jsd_torch=theirs,
            exhaustive_fraction=round((int(status[1]) + int(status_r[1])) / n_pts, 5),
            # (float32 cdist uses the expanded form: a few points near a cell boundary may land in the neighbour cell)
            counters_l1_vs_torch=int((cs.double() / cs.sum() - P).abs().mul(cs.sum()).round().sum()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
