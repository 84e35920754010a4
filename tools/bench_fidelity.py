#!/usr/bin/env python3
"""Times the pairwise figures on the FID features (`sivae_hip.fidelity`, csrc/feat_pairs.hip) and, in the same call, a
chunked torch fp64 restatement of the same figures on the same device (matmul + topk / compare).  The Inception forward
is outside all of this.

Steps (each one process of its own under `timeout`; the driver itself never touches the GPU and stops at the first step
that fails):

  prdc   precision / recall / density / coverage of two sets of --rows x 2048 fp32 rows (k = 3), every step timed with
         HIP events: the row norms, the two same-set neighbour passes, the two ball counts, the cross nearest-neighbour
         pass; every launch of the strip kernels is timed on its own (ops.TIMER) and the longest one reported with its
         multiply-adds.  Then the restatement: row chunks of the fp64 distance matrix from torch.matmul, topk and
         compares.  The figures of the two must agree (reported, with the number of memberships that differ).
  kid    KID with 100 subsets of 1000 rows out of --rows: the gather and the three kernel sums, against the restatement
         (bmm of the gathered subsets in fp64).

Each step prints one JSON line; the driver runs prdc at 10 000 and 50 000 rows and kid at 50 000 and appends the raw lines
to profiles/fidelity_bench.txt.  No ratio is fixed in advance: what is measured is written down, also where torch's BLAS
wins the raw product.

    python tools/bench_fidelity.py [--out profiles/fidelity_bench.txt]
    python tools/bench_fidelity.py --step prdc|kid [--rows 50000] [--dims 2048] [--macs N]
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

STEP_TIMEOUT_S = {"prdc": 420, "kid": 240}
CHUNK_BYTES = 1 << 30  # of the restatement's fp64 distance rows


def _timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return out, e0.elapsed_time(e1)


def _device(torch):
    p = torch.cuda.get_device_properties(0)
    return dict(device=p.name, compute_units=p.multi_processor_count)


def _features(torch, rows, dims):
    """real rows relu(z W + b) (non-negative and correlated like pooled post-ReLU features); the first half of the fake
    rows are real rows plus noise, the second half come from a wider, shifted distribution"""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    w = torch.eye(dims, device=dev) + 0.5 * torch.randn(dims, dims, generator=g, device=dev) / dims ** 0.5
    b = 0.25 + 0.5 * torch.rand(dims, generator=g, device=dev)
    real, fake = torch.empty(rows, dims, device=dev), torch.empty(rows, dims, device=dev)
    for i in range(0, rows, 4096):
        n = min(4096, rows - i)
        real[i:i + n] = torch.relu(torch.randn(n, dims, generator=g, device=dev) @ w + b)
        near = real[i:i + n] + 0.05 * torch.randn(n, dims, generator=g, device=dev)
        far = torch.relu(1.5 * torch.randn(n, dims, generator=g, device=dev) @ w + b + 0.5)
        fake[i:i + n] = torch.where((torch.arange(i, i + n, device=dev) < rows // 2)[:, None], near, far)
    return real, fake


def _torch_prdc(torch, real, fake, k):
    """the same figures from chunks of the fp64 distance matrix: matmul + topk / compare"""
    xr, xf = real.double(), fake.double()
    nr, nf = (xr * xr).sum(1), (xf * xf).sum(1)
    chunk = max(1, CHUNK_BYTES // (8 * max(real.shape[0], fake.shape[0])))

    def rows_of(a, na, b, nb, fn):
        for i in range(0, a.shape[0], chunk):
            d2 = (na[i:i + chunk, None] + nb[None, :] - 2.0 * (a[i:i + chunk] @ b.t())).clamp_min_(0.0)
            fn(i, d2)

    def kth_self(a, na):
        out = torch.empty(a.shape[0], dtype=torch.float64, device=a.device)

        def take(i, d2):
            idx = torch.arange(i, i + d2.shape[0], device=a.device)
            d2[idx - i, idx] = float("inf")
            out[i:i + d2.shape[0]] = torch.topk(d2, k, dim=1, largest=False).values[:, k - 1]
        rows_of(a, na, a, na, take)
        return out

    rad_r, rad_f = kth_self(xr, nr), kth_self(xf, nf)
    in_real = torch.zeros(fake.shape[0], dtype=torch.int64, device=real.device)
    in_fake = torch.zeros(real.shape[0], dtype=torch.int64, device=real.device)
    nearest = torch.empty(real.shape[0], dtype=torch.float64, device=real.device)

    def count_fake(i, d2):
        in_real[i:i + d2.shape[0]] = (d2 <= rad_r[None, :]).sum(1)

    def count_real(i, d2):
        in_fake[i:i + d2.shape[0]] = (d2 <= rad_f[None, :]).sum(1)
        nearest[i:i + d2.shape[0]] = d2.min(1).values

    rows_of(xf, nf, xr, nr, count_fake)
    rows_of(xr, nr, xf, nf, count_real)
    n_real, n_fake = real.shape[0], fake.shape[0]
    return dict(precision=int((in_real > 0).sum()) / n_fake, recall=int((in_fake > 0).sum()) / n_real,
                density=int(in_real.sum()) / (k * n_fake), coverage=int((nearest <= rad_r).sum()) / n_real), in_real


def step_prdc(a):
    import torch
    from sivae_hip import fidelity as FD
    from sivae_hip import ops
    if a.macs:
        FD.FEAT_MACS_PER_LAUNCH = a.macs
    real, fake = _features(torch, a.rows, a.dims)
    k = 3
    FD.knn_sqdist(real[:256], k=k)   # (warm-up: loads the library and the kernels)
    torch.cuda.synchronize()
    res = dict(step="prdc", rows=a.rows, dims=a.dims, k=k, macs_per_launch=FD.FEAT_MACS_PER_LAUNCH,
               launches_per_pass=len(FD.plan_slabs(a.rows, a.rows, a.dims)), **_device(torch))
    ops.TIMER = ops.KernelTimer()
    (nr, nf), res["norms_ms"] = _timed(torch, lambda: (FD._norms("bench", real), FD._norms("bench", fake)))
    rad_r, res["knn_real_ms"] = _timed(torch, lambda: FD._knn(real, nr, real, nr, k, True)[:, k - 1].contiguous())
    rad_f, res["knn_fake_ms"] = _timed(torch, lambda: FD._knn(fake, nf, fake, nf, k, True)[:, k - 1].contiguous())
    in_real, res["within_real_balls_ms"] = _timed(torch, lambda: FD._within(fake, nf, real, nr, rad_r))
    _, res["within_fake_balls_ms"] = _timed(torch, lambda: FD._within(real, nr, fake, nf, rad_f))
    _, res["nearest_fake_ms"] = _timed(torch, lambda: FD._knn(real, nr, fake, nf, 1, False))
    torch.cuda.synchronize()
    launches = [(s.elapsed_time(e), key, flops) for key, flops, s, e, _ in ops.TIMER.records]
    ops.TIMER = None
    ms, key, flops = max(launches)
    res["longest_launch"] = dict(ms=round(ms, 3), kernel=key, macs=int(flops / 2), fp64_tflops=round(flops / ms / 1e9, 2))
    for name in ("feat_knn_update", "feat_within_update"):
        mine = [(m, f) for m, kk, f in launches if kk == name]
        res[name] = dict(launches=len(mine), total_ms=round(sum(m for m, _ in mine), 3),
                         fp64_tflops=round(sum(f for _, f in mine) / sum(m for m, _ in mine) / 1e9, 2))
    figures, res["prdc_ms"] = _timed(torch, lambda: FD.prdc(real, fake, k=k))
    res["figures"] = {n: figures[n] for n in ("precision", "recall", "density", "coverage")}
    (ref, ref_in_real), res["torch_fp64_prdc_ms"] = _timed(torch, lambda: _torch_prdc(torch, real, fake, k))
    (_, _), res["torch_fp64_prdc_second_ms"] = _timed(torch, lambda: _torch_prdc(torch, real, fake, k))
    res["torch_fp64_figures"] = ref
    res["memberships_that_differ"] = int((in_real.long() != ref_in_real).sum())
    for key_ in list(res):
        if key_.endswith("_ms"):
            res[key_] = round(res[key_], 3)
    res["torch_over_device"] = round(res["torch_fp64_prdc_second_ms"] / res["prdc_ms"], 2)
    print(json.dumps(res))


def step_kid(a):
    import torch
    from sivae_hip import fidelity as FD
    real, fake = _features(torch, a.rows, a.dims)
    subsets, m = 100, 1000
    idx = FD.kid_indices(a.rows, a.rows, subsets, m, seed=0)
    FD.kid(real, fake, indices=(idx[0][:2], idx[1][:2]))   # (warm-up)
    torch.cuda.synchronize()
    res = dict(step="kid", rows=a.rows, dims=a.dims, subsets=subsets, subset_size=m, **_device(torch))
    (mean, std), res["kid_ms"] = _timed(torch, lambda: FD.kid(real, fake, indices=idx))
    (mean2, std2), res["kid_second_ms"] = _timed(torch, lambda: FD.kid(real, fake, indices=idx))
    res["kid"], res["bit_identical_runs"] = [mean, std], bool((mean, std) == (mean2, std2))

    def restated():
        gamma, vals = 1.0 / a.dims, []
        for s in range(subsets):
            x, y = real[idx[0][s].to(real.device)].double(), fake[idx[1][s].to(real.device)].double()
            kxx, kyy, kxy = ((gamma * (p @ q.t()) + 1.0) ** 3 for p, q in ((x, x), (y, y), (x, y)))
            vals.append((kxx.sum() - kxx.diagonal().sum()) / (m * (m - 1)) + (kyy.sum() - kyy.diagonal().sum()) / (m * (m - 1))
                        - 2.0 * kxy.sum() / (m * m))
        vals = torch.stack(vals)
        return float(vals.mean()), float(vals.std(unbiased=False))

    restated()
    (rm, rs), res["torch_fp64_kid_ms"] = _timed(torch, restated)
    res["torch_fp64_kid"] = [rm, rs]
    for key_ in list(res):
        if key_.endswith("_ms"):
            res[key_] = round(res[key_], 3)
    res["torch_over_device"] = round(res["torch_fp64_kid_ms"] / res["kid_second_ms"], 2)
    print(json.dumps(res))


def drive(a):
    out = a.out if os.path.isabs(a.out) else os.path.join(REPO, a.out)
    for step, rows in (("prdc", 10000), ("prdc", 50000), ("kid", 50000)):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--rows", str(rows), "--dims", str(a.dims)] + (["--macs", str(a.macs)] if a.macs else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if p.returncode != 0:
            raise SystemExit("bench_fidelity: step %s at %d rows ended with status %d; nothing further is started"
                             % (step, rows, p.returncode))
        with open(out, "a") as f:
            f.write(p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("prdc", "kid"))
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--macs", type=int, default=0, help="FEAT_MACS_PER_LAUNCH for this run (default: the module's)")
    ap.add_argument("--out", default=os.path.join("profiles", "fidelity_bench.txt"))
    a = ap.parse_args()
    if a.step is None:
        return drive(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fidelity: needs a ROCm device (timings on a CPU would say nothing)")
    dict(prdc=step_prdc, kid=step_kid)[a.step](a)


if __name__ == "__main__":
    main()
