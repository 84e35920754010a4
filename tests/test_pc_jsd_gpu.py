"""GPU checks of the JSD validation metric (csrc/pc_jsd.hip, sivae_hip/pointcloud.py, soft_intro_vae_3d/metrics/jsd.py)
against the fixture recorded from the reference (tests/golden/pc3d_jsd.npz) and the float64 restatement of
tests/pc3d_jsd_oracle.py.

Counters are integers and are compared for EQUALITY.  That is a fair demand only where float32 can tell a point's nearest
centre from its second nearest: the fixture's inputs (and the seeded draws below, asserted here) keep a relative gap of
at least 2^-16 between the two squared distances, 64 x the 4 * 2^-24 error of a direct-form float32 distance.

Divergences: |value - fixture| <= 1e-10, the worst-case bound 3.5e-11 of float64 sums of <= 21 952 terms of size
<= log2 G, rounded up.  Each test prints the error it finds.
"""
import functools
import os

import numpy as np
import pytest
import torch

import pc3d_jsd_oracle as JO
import pc3d_oracle as O
from support.pc import DEV, _PC, _np

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [("A_sample", 28, True), ("A_ref", 28, True), ("B", 28, True), ("C", 8, False), ("E", 28, True)]


@functools.lru_cache(maxsize=None)
def _fx():
    return dict(np.load(os.path.join(GOLD, "pc3d_jsd.npz")))


def _pcs(key):
    fx = _fx()
    return fx[key] if key.startswith("A_") else fx[key + "_pcs"]


def _J():
    import soft_intro_vae_3d.metrics.jsd as J
    return J


@pytest.mark.parametrize("key,res,clip", CASES)
def test_occupancy_grid_equals_the_reference(key, res, clip):
    PC, fx = _PC(), _fx()
    x = torch.from_numpy(_pcs(key)).to(DEV)
    counters, bernoulli, status = PC.occupancy_grid(x, res, clip, return_status=True)
    assert counters.dtype == torch.int32 and bernoulli.dtype == torch.int32
    print("%s: %d of %d points on the exhaustive route" % (key, int(status[1]), x.shape[0] * x.shape[1]))
    assert np.array_equal(_np(counters), fx[key + "_counters"])
    assert np.array_equal(_np(bernoulli), fx[key + "_bernoulli"])
    # two calls are bit-identical; the counters do not depend on whether the per-cloud counts are wanted
    c2, b2 = PC.occupancy_grid(x, res, clip)
    assert torch.equal(c2, counters) and torch.equal(b2, bernoulli)
    c3, b3 = PC.occupancy_grid(x, res, clip, want_bernoulli=False)
    assert b3 is None and torch.equal(c3, counters)
    # the drop-in's function: the reference's return types and its entropy
    ent, cnt = _J()._entropy_of_occupancy_grid(x, res, clip)
    assert isinstance(cnt, np.ndarray) and cnt.dtype == np.float64 and np.array_equal(cnt, fx[key + "_counters"])
    if key != "E":
        assert isinstance(ent, float) and abs(ent - float(fx[key + "_entropy"])) <= 1e-10 * float(fx[key + "_entropy"])


def test_occupancy_grid_reads_a_transposed_view_in_place():
    PC, fx = _PC(), _fx()
    base = torch.from_numpy(fx["A_sample"]).to(DEV).permute(0, 2, 1).contiguous()  # [3, 3, 2048], a decoder's layout
    view = base.transpose(1, 2)
    ptr, strides = view.data_ptr(), view.stride()
    assert not view.is_contiguous() and view.shape == (3, 2048, 3)
    counters, bernoulli = PC.occupancy_grid(view, 28, True)
    assert view.data_ptr() == ptr == base.data_ptr() and view.stride() == strides == (3 * 2048, 1, 2048)
    assert np.array_equal(_np(counters), fx["A_sample_counters"]) and np.array_equal(_np(bernoulli), fx["A_sample_bernoulli"])
    assert np.array_equal(_np(PC.voxel_histogram(view, 28)), JO.voxel_distribution(fx["A_sample"], 28))


@pytest.mark.parametrize("voxels", [64, 28])
def test_voxel_histogram_equals_the_reference(voxels):
    PC, J, fx = _PC(), _J(), _fx()
    for k in ("1", "2"):
        x = torch.from_numpy(fx["D_pc" + k]).to(DEV)
        counts = PC.voxel_histogram(x, voxels)
        assert counts.dtype == torch.int32 and np.array_equal(_np(counts), fx["D_counts%s_%d" % (k, voxels)])
        assert torch.equal(PC.voxel_histogram(x, voxels), counts)
        d = J._pc_to_voxel_distribution(x, voxels)
        assert d.dtype == np.int32 and np.array_equal(d, fx["D_counts%s_%d" % (k, voxels)])


def test_divergences_equal_the_reference():
    PC, J, fx = _PC(), _J(), _fx()
    a_s, a_r = torch.from_numpy(fx["A_sample"]).to(DEV), torch.from_numpy(fx["A_ref"]).to(DEV)
    cs, cr = torch.from_numpy(fx["A_sample_counters"]).to(DEV), torch.from_numpy(fx["A_ref_counters"]).to(DEV)
    v = PC.js_divergence(cs, cr)
    assert v.dtype == torch.float64 and v.dim() == 0
    vals = {"js_divergence int32 (A)": (float(v), fx["A_jsd"]),
            "js_divergence float64 (A)": (float(PC.js_divergence(cs.double(), cr.double())), fx["A_jsd"]),
            "js_divergence mixed (A)": (float(PC.js_divergence(cs, cr.double())), fx["A_jsd"])}
    for name, got in (("jsd_between_point_cloud_sets (A)", J.jsd_between_point_cloud_sets(a_s, a_r, voxels=28)),
                      ("_js_divergence tensors (A)", J._js_divergence(cs, cr)),
                      ("_js_divergence tensor and numpy array (A)", J._js_divergence(cs, fx["A_ref_counters"])),
                      ("_js_divergence numpy array and tensor (A)",
                       J._js_divergence(fx["A_sample_counters"].astype(np.float64), cr))):
        assert isinstance(got, np.float64), name
        vals[name] = (float(got), fx["A_jsd"])
    d1, d2 = torch.from_numpy(fx["D_pc1"]).to(DEV), torch.from_numpy(fx["D_pc2"]).to(DEV)
    for voxels in (64, 28):
        got = J.js_divercence_between_pc(d1, d2, voxels)
        assert isinstance(got, np.float64)
        vals["js_divercence_between_pc (D, %d)" % voxels] = (float(got), fx["D_jsd_%d" % voxels])
    assert J.js_divercence_between_pc(d1, d2) == vals["js_divercence_between_pc (D, 64)"][0]  # (the default is 64)
    for name, (got, want) in vals.items():
        print("%s: %.15g, |error| %.3e" % (name, got, abs(got - float(want))))
    for name, (got, want) in vals.items():
        assert abs(got - float(want)) <= 1e-10, name
    # identical sets
    for got in (J.jsd_between_point_cloud_sets(a_s, a_s.clone()), J.js_divercence_between_pc(d1, d1.clone(), 28),
                float(PC.js_divergence(cs, cs.clone()))):
        print("identical sets: %.3e" % abs(got))
        assert abs(got) <= 1e-10
    # two runs are bit-identical; an all-zero vector gives NaN as the reference's 0 / 0 does
    assert float(PC.js_divergence(cs, cr)) == float(v)
    assert np.isnan(float(PC.js_divergence(torch.zeros_like(cs), cr)))


@functools.lru_cache(maxsize=None)
def _large_case(clip):
    """resolution 40: 64 000 cells unclipped (beyond any LDS histogram: global atomics per point), and the clipped grid,
    whose outside points take the exhaustive route on that same kernel.  Seed 3, scaled 1.1 so that points fall outside
    the cube too; the draw keeps the 2^-16 gap (asserted)."""
    g = np.random.Generator(np.random.PCG64(3))
    x = ((g.random(size=(2, 300, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.1)).astype(np.float32)
    cells = JO.grid(40, clip)[0]
    counters, bernoulli, gap = JO.occupancy(x, cells)
    return x, len(cells), counters, bernoulli, float(gap.min())


@pytest.mark.parametrize("clip", [False, True])
def test_occupancy_grid_large_grid_route(clip):
    PC = _PC()
    x, G, counters, bernoulli, gap = _large_case(clip)
    print("resolution 40, clipped %s: %d cells, smallest gap %.3e" % (clip, G, gap))
    assert gap >= JO.GAP and (G == 64000 or clip)
    c, b, status = PC.occupancy_grid(torch.from_numpy(x).to(DEV), 40, clip, return_status=True)
    assert c.shape == (G,) and np.array_equal(_np(c), counters) and np.array_equal(_np(b), bernoulli)
    assert (int(status[1]) > 0) == clip
    c2, b2 = PC.occupancy_grid(torch.from_numpy(x).to(DEV), 40, clip)
    assert torch.equal(c2, c) and torch.equal(b2, b)
    # counters alone, which is what jsd_between_point_cloud_sets asks for, on the same global-atomics route
    c3, b3 = PC.occupancy_grid(torch.from_numpy(x).to(DEV), 40, clip, want_bernoulli=False)
    assert b3 is None and np.array_equal(_np(c3), counters)
    J = _J()
    got = J.jsd_between_point_cloud_sets(torch.from_numpy(x).to(DEV), torch.from_numpy(x[:1]).to(DEV), voxels=40,
                                         in_unit_sphere=clip)
    want = JO.js_divergence(counters, JO.occupancy(x[:1], JO.grid(40, clip)[0])[0])
    print("JSD on the resolution-40 grid: %.15g, |error| %.3e" % (got, abs(got - want)))
    assert abs(got - want) <= 1e-10


def test_many_tiles_and_list_flushes():
    """a cloud of 5000 points (five tiles of 1024, the last one partial) scaled 1.6, so that the list of points waiting
    for the exhaustive route fills and is flushed inside a cloud; resolution 8 clipped keeps the restatement small"""
    PC = _PC()
    g = np.random.Generator(np.random.PCG64(5))
    x = ((g.random(size=(3, 5000, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.6)).astype(np.float32)
    counters, bernoulli, gap = JO.occupancy(x, JO.grid(8, True)[0])
    ok = gap >= JO.GAP
    x[~ok] = 0.01  # (a point under the gap is replaced by one that is far above it)
    counters, bernoulli, gap = JO.occupancy(x, JO.grid(8, True)[0])
    assert gap.min() >= JO.GAP
    c, b, status = PC.occupancy_grid(torch.from_numpy(x).to(DEV), 8, True, return_status=True)
    print("%d of %d points on the exhaustive route" % (int(status[1]), 15000))
    assert int(status[1]) > 3 * 2048
    assert np.array_equal(_np(c), counters) and np.array_equal(_np(b), bernoulli)


def test_non_finite_and_cpu_inputs_raise():
    PC, J = _PC(), _J()
    x = torch.from_numpy(_pcs("C").copy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.occupancy_grid(x, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        J.jsd_between_point_cloud_sets(x, x)
    for bad in (float("nan"), float("inf")):
        y = x.clone()
        y[1, 7, 2] = bad
        with pytest.raises(ValueError):
            PC.occupancy_grid(y.to(DEV), 8)
        with pytest.raises(ValueError):
            J.jsd_between_point_cloud_sets(x.to(DEV), y.to(DEV), voxels=8, in_unit_sphere=False)
    y = x.clone()
    y[0, 0, 0] = float("nan")
    with pytest.raises(ValueError):
        PC.voxel_histogram(y.to(DEV), 8)


def test_validation_loop_body():
    """the body of the training script's calc_jsd_valid at small size: decode 6 latent vectors with the drop-in model in
    eval(), transpose_ the [6, 3, 2048] output in place, and take the JSD against case A's sample set.  Decoder outputs
    cannot be filtered for the gap: with k points under it, the counters may differ from the restatement by at most 2 k
    in L1, and the test fails as ill-conditioned if k exceeds 0.1 % of the points."""
    import soft_intro_vae_3d.models.vae as V
    PC, J, fx = _PC(), _J(), _fx()
    z = 128
    sd = O.recipe_state_dict(O.model_specs(z), 17, torch.float32)
    model = V.SoftIntroVAE(O.config(z))
    model.load_state_dict(sd, strict=True)
    model = model.to(DEV).eval()
    noise = torch.randn(6, z, generator=torch.Generator().manual_seed(23)).to(DEV)
    x = torch.from_numpy(fx["A_sample"]).to(DEV)
    with torch.no_grad():
        x_g = model.decode(noise)
    assert x_g.shape[-2:] == (3, 2048)
    x_g.transpose_(1, 2)
    assert not x_g.is_contiguous()
    jsd = J.jsd_between_point_cloud_sets(x, x_g, voxels=28)
    print("JSD of 6 decoded clouds against case A: %.12g" % jsd)
    assert isinstance(jsd, np.float64) and np.isfinite(jsd) and 0.0 <= jsd <= 1.0
    host = x_g.cpu().numpy()
    counters, _, gap = JO.occupancy(host, JO.grid(28, True)[0])
    k = int((gap < JO.GAP).sum())
    print("decoded points under the 2^-16 gap: %d of %d; |x_g| max %.3f" % (k, gap.size, float(np.abs(host).max())))
    assert k <= 0.001 * gap.size, "ill-conditioned: %d of %d decoded points lie on a cell boundary" % (k, gap.size)
    got = _np(PC.occupancy_grid(x_g, 28, True)[0])
    assert int(np.abs(got.astype(np.int64) - counters).sum()) <= 2 * k
    want = JO.js_divergence(fx["A_sample_counters"], got)
    assert abs(float(jsd) - want) <= 1e-10


def test_kernel_timer_reports_the_work_of_the_route_taken():
    """an installed KernelTimer gets one record per occupancy launch whose work figure follows the points that took
    the exhaustive route (8 operations per distance) plus a per-point term, not S N G whatever the route"""
    from sivae_hip import ops
    PC, fx = _PC(), _fx()
    x = torch.from_numpy(fx["A_ref"]).to(DEV)
    inside = x * 0.5  # (|coordinate| <= 0.2: every point's own cell is in the clipped table)
    assert ops.TIMER is None
    ops.TIMER = ops.KernelTimer()
    try:
        _, _, st_a = PC.occupancy_grid(x, 28, True, return_status=True)
        _, _, st_b = PC.occupancy_grid(inside, 28, True, return_status=True)
        torch.cuda.synchronize()
        recs = [r for r in ops.TIMER.records if r[0] == "occupancy_grid_kernel"]
        summary = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    n = x.shape[0] * x.shape[1]
    assert int(st_a[1]) > 0 and int(st_b[1]) == 0 and len(recs) == 2
    assert recs[0][1] == 8.0 * int(st_a[1]) * 10144 + 30.0 * n and recs[1][1] == 30.0 * n
    assert summary["occupancy_grid_kernel"]["launches"] == 2 and summary["occupancy_grid_kernel"]["total_ms"] > 0.0
