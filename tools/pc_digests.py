#!/usr/bin/env python3
"""sha256 of every output of the ReLU -> BatchNorm1d / max-over-points entry points of csrc/pointcloud.hip (relu_bn_stats,
relu_bn_apply, relu_bn_bwd, max_points_fwd / _bwd, relu_bn_max_fwd / _bwd) on seeded inputs, one line per tensor: two
builds of the library that print the same lines compute the same bits.  Shapes are the smallest that reach each path
(tests/test_relu_bn_max_gpu.py, tests/test_pointcloud_paths_gpu.py) plus the real channel count; inputs are
test_relu_bn_max_gpu._case's: a dead channel, a negative and a zero gamma, exact zeros, planted ties.

    python tools/pc_digests.py                    the digests of the library SIVAE_LIB names (default: the in-tree build)
    python tools/pc_digests.py --against OLD.so   one fresh child process per library; prints the lines that differ
"""
import hashlib
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "soft-intro-vae-pytorch_amd"))
# (B, C, N, a one element behind an aligned start)
SHAPES = [(3, 5, 100, False), (2, 3, 33, False), (1, 7, 1, False), (2, 6, 260, False), (2, 5, 2048, False),
          (3, 5, 132, True), (3, 5, 1368, False), (3, 7, 2731, False), (2, 512, 2048, False)]


def digests():
    import torch
    from sivae_hip import pointcloud as PC
    for B, C, N, misaligned in SHAPES:
        g = torch.Generator().manual_seed(B * 1000 + C * 10 + N)
        a = torch.randn(B, C, N, generator=g)
        a[torch.rand(B, C, N, generator=g) < 0.1] = 0.0
        a[:, 0] = -a[:, 0].abs()
        gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
        gamma[1], gamma[2] = -gamma[1], 0.0
        vec = N % 4 == 0 and not misaligned
        if C > 3 and N > (40 if vec else 67):  # the maximum twice in one lane and once in another
            a[B - 1, C - 1, [4, 5, 40] if vec else [3, 67, 10]] = 9.0
        gy, dy = torch.randn(B, C, generator=g), torch.randn(B, C, N, generator=g)
        gy[0, C - 1] = gy[B - 1, 0] = 0.0
        buf = torch.empty(a.numel() + 8, device="cuda:0")
        ad = buf[1:1 + a.numel()].view(a.shape) if misaligned else buf[:a.numel()].view(a.shape)
        ad.copy_(a)
        gamma, beta, gy, dy = (t.to("cuda:0") for t in (gamma, beta, gy, dy))
        rm, rv = torch.zeros(C, device="cuda:0"), torch.ones(C, device="cuda:0")
        out = {}
        out["stats.mean"], out["stats.invstd"] = mean, invstd = PC.relu_bn_stats(ad, rm, rv)
        out["stats.running_mean"], out["stats.running_var"] = rm, rv
        out["apply.y"] = y = PC.relu_bn_apply(ad, mean, invstd, gamma, beta)
        out["bwd.da"], out["bwd.dgamma"], out["bwd.dbeta"] = PC.relu_bn_bwd(dy, ad, mean, invstd, gamma)
        out["max_fwd.vals"], out["max_fwd.arg"] = vals, arg = PC.max_points_fwd(y)
        out["max_bwd.dx"] = PC.max_points_bwd(gy, arg, N)
        out["bn_max_fwd.vals"], out["bn_max_fwd.arg"] = PC.relu_bn_max_fwd(ad, mean, invstd, gamma, beta)
        out["bn_max_bwd.da"], out["bn_max_bwd.dgamma"], out["bn_max_bwd.dbeta"] = PC.relu_bn_max_bwd(gy, arg, ad, mean, invstd,
                                                                                                   gamma)
        for name, t in out.items():
            print("(%d, %d, %d)%s %-20s %s" % (B, C, N, "*" if misaligned else "", name,
                                             hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()))


def against(old):
    runs = []
    for lib in (os.path.abspath(old), os.environ.get("SIVAE_LIB", "")):
        env = dict(os.environ, SIVAE_LIB=lib)
        runs.append(subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, check=True, capture_output=True,
                                   text=True, timeout=300).stdout.splitlines())
    differ = [(o, n) for o, n in zip(*runs) if o != n]
    for o, n in differ:
        print("old %s\nnew %s" % (o, n))
    print("%d digests, %d differ" % (len(runs[0]), len(differ) + abs(len(runs[0]) - len(runs[1]))))
    return 1 if differ or len(runs[0]) != len(runs[1]) or not runs[0] else 0


if __name__ == "__main__":
    sys.exit(against(sys.argv[2]) if sys.argv[1:2] == ["--against"] else digests())
