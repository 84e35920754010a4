"""Generate the style variant's optimizer fixture from the REAL reference (runs only where the reference checkout is at hand).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lreq_adam.py /path/to/reference

The reference's style_soft_intro_vae/custom_adam.py is imported from its own directory and runs on the CPU, twice on the
same inputs: in float64 (the recorded trajectory) and in float32 (the yardstick: what the reference itself loses in the
precision the kernels work in).  The inputs and the schedule (sizes, groups, coefficients, which gradient is None at
which step, the second group's learning rate, the state reset) are those of tests/lreq_adam_oracle.py.  lreq_adam.npz holds

  p0/<t>, g<i>/<t>          the float32 inputs: parameters and the two base gradients (a step's gradient is a base times a
                            power of two, oracle.grad_of)
  p<k>/<t>, v<k>/<t>        the float64 parameters and exp_avg_sq after step k in oracle.SNAPSHOTS (zeros where a tensor has
                            no state), steps<k> the per-tensor step counts
  f32_dev_p, f32_dev_v      the worst per-tensor max-norm relative deviation of the float32 run from the float64 run over
                            the snapshots
  lerp_p, lerp_q, lerp_w    the inputs of the weight average and its two weights, one on each side of 0.5: the training
                            script's 1 - 0.5^(32 / 10000) and 0.75;  lerp_out<i> torch's float64 lerp_ for weight i
  meta                      JSON: the torch version the reference ran on

Nothing of the reference is copied: the fixture holds inputs and recorded results only.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import lreq_adam_oracle as O  # noqa: E402


def main(reference):
    sys.path.insert(0, os.path.join(reference, "style_soft_intro_vae"))
    from custom_adam import LREQAdam
    params0, base = O.make_inputs()
    r64, r32 = (O.run_class(LREQAdam, params0, base, dt)[0] for dt in (torch.float64, torch.float32))
    d = {"meta": np.frombuffer(json.dumps({"torch": torch.__version__}).encode(), dtype=np.uint8)}
    dev = [0.0, 0.0]
    for t, a in enumerate(params0):
        d["p0/%d" % t] = a
        for i in range(2):
            d["g%d/%d" % (i, t)] = base[i][t]
    for k in O.SNAPSHOTS:
        assert r64[k][2] == r32[k][2]
        d["steps%d" % k] = np.array(r64[k][2], dtype=np.int64)
        for t in range(len(params0)):
            d["p%d/%d" % (k, t)], d["v%d/%d" % (k, t)] = r64[k][0][t], r64[k][1][t]
            for j in range(2):
                dev[j] = max(dev[j], O.rel_dev(r32[k][j][t], r64[k][j][t]))
    d["f32_dev_p"], d["f32_dev_v"] = np.float64(dev[0]), np.float64(dev[1])
    rng = np.random.default_rng(7)
    lp, lq = rng.standard_normal(1025).astype(np.float32), rng.standard_normal(1025).astype(np.float32)
    ws = np.array([1.0 - 0.5 ** (32 / (10 * 1000.0)), 0.75])
    d["lerp_p"], d["lerp_q"], d["lerp_w"] = lp, lq, ws
    for i, w in enumerate(ws):
        d["lerp_out%d" % i] = torch.from_numpy(lp).double().lerp_(torch.from_numpy(lq).double(), float(w)).numpy()
    path = os.path.join(HERE, "lreq_adam.npz")
    np.savez_compressed(path, **d)
    print("wrote %s (%d bytes): float32 against float64, worst per tensor: p %.3e, v %.3e; step counts after %d: %s"
          % (path, os.path.getsize(path), dev[0], dev[1], O.STEPS, r64[O.STEPS][2]))


if __name__ == "__main__":
    main(sys.argv[1])
