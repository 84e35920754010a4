#!/usr/bin/env python3
"""Times FID on the device (`sivae_hip.fid`, csrc/fid.hip) against the reference's host path on the same data.  The
Inception forward is outside all of this: its cost is the same on both paths.

Steps (each one process of its own under `timeout`; the driver itself never touches the GPU and stops at the first step
that fails):

  stream    50 000 x 2048 fp32 activations, already on the device, in batches of 50 through ActivationStatistics up to
            (mu, sigma); HIP events around the whole pass, one warm-up pass, then --rounds passes.  Baseline, once: what
            soft_intro_vae/metrics/fid_score.py:197, :202-203, :349-350 does with the same batches: a device-to-host
            copy of every batch, np.concatenate, np.mean and np.cov (which converts to float64), 16 threads.
  distance  frechet_distance at d = 2048 on the statistics of two 8192-row sets, with the eigen-decompositions on host
            copies and, where this torch build has a device solver, on the device.  Baseline, once: the reference's formula
            (fid_score.py:304-325: scipy.linalg.sqrtm of sigma1 sigma2) on host copies.
  flush     the moment kernel alone on one 1024 x 2048 block: fp64 FLOP/s, algorithmic (n d (d + 1): the upper triangle
            with the diagonal) and executed (whole 64 x 64 tiles on and above the diagonal).

Each step prints one JSON line; the driver appends the raw lines to profiles/fid_bench.txt.

    python tools/bench_fid.py [--out profiles/fid_bench.txt]        # the driver: all three steps
    python tools/bench_fid.py --step stream|distance|flush [--rows 50000] [--dims 2048] [--rounds 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "soft-intro-vae-pytorch_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

STEP_TIMEOUT_S = {"stream": 240, "distance": 300, "flush": 60}
THREADS = 16


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


def _device(torch):
    p = torch.cuda.get_device_properties(0)
    return dict(device=p.name, compute_units=p.multi_processor_count)


def _activations(torch, rows, dims, seed):
    """fp32 [rows, dims] on the device: relu(z W + b), non-negative and correlated like pooled post-ReLU features"""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(seed)
    w = torch.eye(dims, device=dev) + 0.5 * torch.randn(dims, dims, generator=g, device=dev) / dims ** 0.5
    b = 0.25 + 0.5 * torch.rand(dims, generator=g, device=dev)
    out = torch.empty(rows, dims, device=dev)
    for i in range(0, rows, 4096):
        z = torch.randn(min(4096, rows - i), dims, generator=g, device=dev)
        out[i:i + z.shape[0]] = torch.relu(z @ w + b)
    return out


def step_stream(a):
    import numpy as np
    import torch
    from sivae_hip import fid as F
    torch.set_num_threads(THREADS)
    dev = torch.device("cuda:0")
    act = _activations(torch, a.rows, a.dims, 0)
    batches = [act[i:i + a.batch] for i in range(0, a.rows, a.batch)]

    def device_pass():
        st = F.ActivationStatistics(a.dims, dev)
        for x in batches:
            st.update(x)
        return st.finalize()

    device_pass()  # (warm-up: loads the library and the kernels)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.rounds):
        (mu, sigma), t = _timed(torch, device_pass)
        ms.append(t)

    def host_pass():
        acts = [x.cpu().data.numpy().reshape(x.size(0), -1) for x in batches]
        arr = np.concatenate(acts)[:a.rows]
        return np.mean(arr, axis=0), np.cov(arr, rowvar=False)

    t0 = time.perf_counter()
    mu_h, sigma_h = host_pass()
    host_ms = (time.perf_counter() - t0) * 1e3
    res = dict(step="stream", rows=a.rows, dims=a.dims, batch=a.batch, rounds=a.rounds, host_threads=THREADS,
               **_device(torch))
    res["device"] = _stats(ms)
    res["reference_host_ms"] = round(host_ms, 1)
    res["speedup"] = round(host_ms / res["device"]["median_ms"], 1)
    res["device_wins"] = bool(res["device"]["max_ms"] < host_ms)
    res["sigma_max_diff_rel_to_max"] = float(np.abs(sigma.cpu().numpy() - sigma_h).max() / np.abs(sigma_h).max())
    res["mu_max_diff_rel_to_max_vs_float32_mean"] = float(np.abs(mu.cpu().numpy() - mu_h).max() / np.abs(mu_h).max())
    print(json.dumps(res))


def step_distance(a):
    import numpy as np
    import torch
    from scipy import linalg
    from sivae_hip import fid as F
    torch.set_num_threads(THREADS)
    dev = torch.device("cuda:0")
    stats = []
    for seed in (1, 2):
        st = F.ActivationStatistics(a.dims, dev)
        st.update(_activations(torch, 4 * a.dims, a.dims, seed))
        stats.append(st.finalize())
    (m1, s1), (m2, s2) = stats
    res = dict(step="distance", dims=a.dims, rows_per_side=4 * a.dims, rounds=a.rounds, host_threads=THREADS,
               **_device(torch))
    values = {}
    for where in ("cpu", "device"):
        F.EIGH = where
        try:
            values[where] = F.frechet_distance(m1, s1, m2, s2)  # (warm-up)
        except RuntimeError as e:
            res["eigh_" + where] = "unavailable: %s" % str(e).splitlines()[0][:200]
            continue
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            F.frechet_distance(m1, s1, m2, s2)
            ms.append((time.perf_counter() - t0) * 1e3)
        res["eigh_" + where] = _stats(ms)
    # where the time goes: the three products alone
    from sivae_hip import ops
    x = s1.contiguous()
    ops.fid_xty(x, x, symmetric=True)
    _, t_sym = _timed(torch, lambda: ops.fid_xty(x, x, symmetric=True))
    _, t_plain = _timed(torch, lambda: ops.fid_xty(x, s2))
    res["xty_symmetric_ms"], res["xty_plain_ms"] = round(t_sym, 3), round(t_plain, 3)
    res["xty_plain_fp64_tflops"] = round(2.0 * a.dims ** 3 / (t_plain * 1e-3) / 1e12, 2)

    mu1, mu2, sg1, sg2 = (t.cpu().numpy() for t in (m1, m2, s1, s2))
    t0 = time.perf_counter()
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sg1.dot(sg2), disp=False)
    ref = float(diff.dot(diff) + np.trace(sg1) + np.trace(sg2) - 2 * np.trace(covmean.real))
    host_ms = (time.perf_counter() - t0) * 1e3
    res["reference_host_ms"] = round(host_ms, 1)
    res["reference_value"], res["values"] = ref, values
    res["sqrtm_max_imag"] = float(np.abs(covmean.imag).max()) if np.iscomplexobj(covmean) else 0.0
    res["max_rel_diff_vs_reference"] = max(abs(v - ref) / abs(ref) for v in values.values())
    timed = {k: res["eigh_" + k]["max_ms"] for k in values}
    res["device_wins"] = {k: bool(v < host_ms) for k, v in timed.items()}
    print(json.dumps(res))


def step_flush(a):
    import torch
    from sivae_hip import ops
    dev = torch.device("cuda:0")
    n, d = 1024, a.dims
    block = _activations(torch, n, d, 3)
    G, s = ops.fid_state(d, dev)
    ops.fid_moments(block, n, G, s)  # (warm-up)
    torch.cuda.synchronize()
    ms = [_timed(torch, lambda: ops.fid_moments(block, n, G, s))[1] for _ in range(max(a.rounds, 10))]
    tiles = (d + 63) // 64
    algorithmic, executed = float(n) * d * (d + 1), 2.0 * n * 64 * 64 * tiles * (tiles + 1) / 2
    med = sorted(ms)[len(ms) // 2] * 1e-3
    res = dict(step="flush", rows=n, dims=d, **_device(torch))
    res["launch"] = _stats(ms)
    res["fp64_tflops_algorithmic"] = round(algorithmic / med / 1e12, 2)
    res["fp64_tflops_executed"] = round(executed / med / 1e12, 2)
    print(json.dumps(res))


def drive(a):
    out = a.out if os.path.isabs(a.out) else os.path.join(REPO, a.out)
    for step in ("stream", "distance", "flush"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--rows", str(a.rows), "--dims", str(a.dims), "--batch", str(a.batch), "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            raise SystemExit("bench_fid: step %s ended with status %d; nothing further is started" % (step, p.returncode))
        with open(out, "a") as f:
            f.write(p.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("stream", "distance", "flush"))
    ap.add_argument("--rows", type=int, default=50000)
    ap.add_argument("--dims", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "fid_bench.txt"))
    a = ap.parse_args()
    if a.step is None:
        return drive(a)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_fid: needs a ROCm device (timings on a CPU would say nothing)")
    dict(stream=step_stream, distance=step_distance, flush=step_flush)[a.step](a)


if __name__ == "__main__":
    main()
