"""CPU-side checks of the JSD validation metric of the 3-D slice: the numpy float64 restatement (tests/pc3d_jsd_oracle.py)
against the fixture recorded from the reference (counters exactly, entropies and divergences to 1e-10 relative), the
package's host-built cell table against the recorded mask and spacing, the drop-in module's surface, and the argument
validation of the new entry points (every call returns before any launch)."""
import ctypes
import functools
import inspect
import os

import numpy as np
import pytest
import torch

import pc3d_jsd_oracle as JO
from sivae_hip import lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _fx():
    return dict(np.load(os.path.join(GOLD, "pc3d_jsd.npz")))


def _close(a, b):
    return abs(float(a) - float(b)) <= 1e-10 * abs(float(b))


@pytest.mark.parametrize("key,res,clip", [("A_sample", 28, True), ("A_ref", 28, True), ("B", 28, True), ("C", 8, False),
                                          ("E", 28, True)])
def test_restatement_occupancy_equals_reference(key, res, clip):
    fx = _fx()
    pcs = fx[key] if key.startswith("A_") else fx[key + "_pcs"]
    counters, bernoulli, gap = JO.occupancy(pcs, JO.grid(res, clip)[0])
    assert gap.min() >= JO.GAP, "the fixture's input condition: every point's gap is at least 2^-16"
    assert np.array_equal(counters, fx[key + "_counters"]) and np.array_equal(bernoulli, fx[key + "_bernoulli"])
    assert counters.sum() == pcs.shape[0] * pcs.shape[1]
    if key != "E":
        assert _close(JO.bernoulli_entropy(bernoulli, len(pcs)), fx[key + "_entropy"])


def test_restatement_divergences_equal_reference():
    fx = _fx()
    assert _close(JO.js_divergence(fx["A_sample_counters"], fx["A_ref_counters"]), fx["A_jsd"])
    for v in (64, 28):
        c1, c2 = JO.voxel_distribution(fx["D_pc1"], v), JO.voxel_distribution(fx["D_pc2"], v)
        assert np.array_equal(c1, fx["D_counts1_%d" % v]) and np.array_equal(c2, fx["D_counts2_%d" % v])
        assert _close(JO.js_divergence(c1, c2), fx["D_jsd_%d" % v])
    assert not np.array_equal(fx["B_counters"], fx["B_bernoulli"])  # (the copy and the repeated points show)


@pytest.mark.parametrize("res", [28, 8])
def test_host_cell_table_equals_the_recorded_grid(res):
    from sivae_hip import pointcloud as PC
    import soft_intro_vae_3d.metrics.jsd as J
    fx = _fx()
    want = np.unpackbits(fx["mask%d" % res])[:res ** 3].astype(bool)
    axis, mask, spacing = PC.unit_cube_grid(res, True)
    assert np.array_equal(mask, want) and spacing == float(fx["spacing%d" % res])
    cells, omask, _ = JO.grid(res, True)
    assert np.array_equal(omask, want) and np.array_equal(PC.grid_cells(axis, mask), cells)
    grid, sp = J._unit_cube_grid_point_cloud(res, True)
    assert grid.dtype == np.float32 and np.array_equal(grid, cells) and sp == spacing
    full, _ = J._unit_cube_grid_point_cloud(res)
    assert full.shape == (res, res, res, 3) and np.array_equal(full.reshape(-1, 3), JO.grid(res, False)[0])
    if res == 28:
        assert len(cells) == 10144


def test_dropin_surface_matches_the_reference():
    """names, parameter lists and defaults of soft_intro_vae_3d/metrics/jsd.py"""
    import soft_intro_vae_3d.metrics.jsd as J
    assert J.__all__ == ['js_divercence_between_pc', 'jsd_between_point_cloud_sets']

    def sig(f):
        return [(k, p.default) for k, p in inspect.signature(f).parameters.items()]

    E = inspect.Parameter.empty
    assert sig(J.js_divercence_between_pc) == [("pc1", E), ("pc2", E), ("voxels", 64)]
    assert sig(J.jsd_between_point_cloud_sets) == [("sample_pcs", E), ("ref_pcs", E), ("voxels", 28), ("in_unit_sphere", True)]
    assert sig(J._js_divergence) == [("P", E), ("Q", E)]
    assert sig(J._pc_to_voxel_distribution) == [("pc", E), ("n_voxels", 64)]
    assert sig(J._entropy_of_occupancy_grid) == [("pclouds", E), ("grid_resolution", E), ("in_sphere", False)]
    assert sig(J._unit_cube_grid_point_cloud) == [("resolution", E), ("clip_sphere", False)]
    for banned in ("scipy", "sklearn"):
        assert ("import " + banned) not in inspect.getsource(J) and ("from " + banned) not in inspect.getsource(J)


def test_host_js_divergence_on_numpy_counts():
    """the numpy path of the drop-in's _js_divergence (the reference's accepts arrays)"""
    import soft_intro_vae_3d.metrics.jsd as J
    fx = _fx()
    v = J._js_divergence(fx["A_sample_counters"].astype(np.float64), fx["A_ref_counters"].astype(np.float64))
    assert isinstance(v, np.float64) and abs(v - float(fx["A_jsd"])) <= 1e-10
    assert abs(J._js_divergence(fx["C_counters"], fx["C_counters"])) <= 1e-10
    assert np.isnan(J._js_divergence(np.zeros(4), np.ones(4)))


def test_cpu_tensors_are_rejected():
    from sivae_hip import pointcloud as PC
    import soft_intro_vae_3d.metrics.jsd as J
    x = torch.zeros(2, 5, 3)
    for f in (lambda: PC.occupancy_grid(x, 8), lambda: PC.voxel_histogram(x, 8),
              lambda: PC.js_divergence(torch.ones(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32)),
              lambda: J.jsd_between_point_cloud_sets(x, x), lambda: J.js_divercence_between_pc(x, x),
              lambda: J._entropy_of_occupancy_grid(x, 8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f()


def test_jsd_entry_points_validate_arguments():
    """null pointers, zero sizes, S N >= 2^31, resolutions and modes outside the kernels' range: the documented codes.
    (None of the three entry points takes a workspace: there is no workspace query and no short-workspace code.)"""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    o = L.sivae_occupancy_grid
    ok = dict(pcs=one, ss=30, sn=3, sc=1, S=2, N=5, cells=one, lut=one, axis=one, res=8, G=512, counters=one, bern=one,
              status=one, stream=null)

    def occ(**kw):
        a = dict(ok, **kw)
        return o(*[a[k] for k in ok])

    for k in ("pcs", "cells", "lut", "axis", "counters", "status"):
        assert occ(**{k: null}) == -1, k
    assert occ(S=0) == -2 and occ(N=0) == -2 and occ(G=0) == -2 and occ(S=-1) == -2
    assert occ(res=1) == -2 and occ(res=65) == -2 and occ(G=513) == -2
    assert occ(S=1 << 16, N=1 << 15) == -5 and occ(S=1 << 20, N=1 << 20) == -5
    v = L.sivae_voxel_histogram
    assert v(null, 30, 3, 1, 2, 5, 8, one, one, null) == -1 and v(one, 30, 3, 1, 2, 5, 8, null, one, null) == -1
    assert v(one, 30, 3, 1, 2, 5, 8, one, null, null) == -1
    assert v(one, 30, 3, 1, 0, 5, 8, one, one, null) == -2 and v(one, 30, 3, 1, 2, 0, 8, one, one, null) == -2
    assert v(one, 30, 3, 1, 2, 5, 0, one, one, null) == -2
    assert v(one, 30, 3, 1, 1 << 16, 1 << 15, 8, one, one, null) == -5 and v(one, 30, 3, 1, 2, 5, 1291, one, one, null) == -5
    j = L.sivae_js_divergence
    assert j(null, one, 0, 0, 8, one, null) == -1 and j(one, null, 0, 0, 8, one, null) == -1
    assert j(one, one, 0, 0, 8, null, null) == -1
    assert j(one, one, 0, 0, 0, one, null) == -2 and j(one, one, 2, 0, 8, one, null) == -6


def test_build_imports_the_metric_module():
    import __graft_entry__ as G
    assert "soft_intro_vae_3d.metrics.jsd" in inspect.getsource(G.build)
    from sivae_hip import pointcloud as PC
    for name in ("occupancy_grid", "voxel_histogram", "js_divergence"):
        assert callable(getattr(PC, name))
