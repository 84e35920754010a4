"""Generate the JSD-metric fixture from the REAL reference (runs only where the reference checkout is mounted; needs the
scipy and scikit-learn the reference imports).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_jsd.py /path/to/reference

The reference's soft_intro_vae_3d/metrics/jsd.py is imported BY FILE PATH under a private module name.  pc3d_jsd.npz holds
inputs and outputs only (float32 PCG64 draws, the reference's counters, entropies and divergences):

  A  voxels 28 clipped; sample [3, 2048, 3] uniform in the cube, reference set [2, 2048, 3] scaled 0.8: counters and entropy
     of both sets, their JSD
  B  voxels 28 clipped, [5, 333, 3] scaled 1.3 (points outside the cube); cloud 1 is a copy of cloud 0 and 16 points of
     cloud 2 are repeated inside it: counters, entropy
  C  resolution 8 unclipped, [4, 100, 3] scaled 1.1: counters, entropy
  D  js_divercence_between_pc on two [4, 100, 3] sets scaled 1.2, voxels 64 and 28: the count vectors and the values
  E  [1, 1, 3], voxels 28 clipped: counters.  The reference's own loop cannot run a one-point cloud (np.squeeze leaves
     it a 0-d index array to iterate over), so this case is recorded from the calls that loop makes: the reference's
     grid and the same sklearn NearestNeighbors(n_neighbors=1) query
  the in-sphere masks of the resolution-28 and resolution-8 grids (bit-packed) and their spacing

The per-cell "clouds that touched it" counts are not returned by the reference; they are recorded as the sum over the
clouds of (counters > 0) of the reference run on each cloud alone.

Before recording, the script checks in a child interpreter that with this project's soft_intro_vae_3d/ directory FIRST on
PYTHONPATH and the reference's own directory behind it, the reference's train_soft_intro_vae_3d.py and
evaluation/find_best_epoch_on_validation_soft.py (plotting, dataset and utility imports stubbed) resolve `metrics.jsd`,
`models.vae` and the function they call to this project's modules, without importing scipy or scikit-learn.

Input condition of A, B, C, E: in float64 every point's nearest and second-nearest centre differ by at least 2^-16 of the
second distance; a point that fails is redrawn, and the script fails if more than 1 % of a case's points needed that.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import pc3d_jsd_oracle as JO  # noqa: E402

if len(sys.argv) != 2:
    raise SystemExit("usage: make_golden_jsd.py /path/to/reference")
REF = sys.argv[1]


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


RESOLVE_CHECK = r"""
import importlib.machinery, importlib.util, os, sys
from unittest import mock
drop, ref3d = sys.argv[1], sys.argv[2]
assert sys.path.index(drop) < sys.path.index(ref3d)
for name in ("matplotlib", "matplotlib.pyplot", "mpl_toolkits", "mpl_toolkits.mplot3d", "tqdm", "pandas", "utils",
             "utils.pcutil", "utils.util", "datasets", "datasets.transforms3d", "datasets.shapenet"):
    m = mock.MagicMock(name=name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__path__ = []
    sys.modules[name] = m
for name, path in (("_ref3d_train", "train_soft_intro_vae_3d.py"),
                   ("_ref3d_best_epoch", os.path.join("evaluation", "find_best_epoch_on_validation_soft.py"))):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref3d, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for pkg in ("metrics.jsd", "models.vae"):
        assert os.path.abspath(sys.modules[pkg].__file__).startswith(drop + os.sep), (path, pkg, sys.modules[pkg].__file__)
    assert mod.jsd_between_point_cloud_sets is sys.modules["metrics.jsd"].jsd_between_point_cloud_sets
    assert mod.SoftIntroVAE is sys.modules["models.vae"].SoftIntroVAE
assert "scipy" not in sys.modules and "sklearn" not in sys.modules
print("resolved: metrics.jsd ->", sys.modules["metrics.jsd"].__file__)
"""


def check_imports_resolve():
    """the reference's two scripts import this project's metrics.jsd when the drop-in directory comes first"""
    drop = os.path.join(os.path.dirname(os.path.dirname(HERE)), "soft-intro-vae-pytorch_amd", "soft_intro_vae_3d")
    ref3d = os.path.join(os.path.abspath(REF), "soft_intro_vae_3d")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([drop, ref3d]), PYTHONDONTWRITEBYTECODE="1")
    subprocess.check_call([sys.executable, "-c", RESOLVE_CHECK, drop, ref3d], env=env)


def draw(g, shape, scale, cells):
    """float32 uniform in the cube times scale, points under the gap redrawn -> (clouds, number of redraws)"""
    x = ((g.random(size=shape, dtype=np.float32) - np.float32(0.5)) * np.float32(scale)).astype(np.float32)
    flat = x.reshape(-1, 3)
    redrawn = 0
    while True:
        bad = np.nonzero(JO.nearest(flat, cells)[1] < JO.GAP)[0]
        if len(bad) == 0:
            break
        redrawn += len(bad)
        flat[bad] = (g.random(size=(len(bad), 3), dtype=np.float32) - np.float32(0.5)) * np.float32(scale)
    assert redrawn <= 0.01 * len(flat), "too many points near a cell boundary: %d of %d" % (redrawn, len(flat))
    assert (JO.nearest(flat, cells)[1] >= JO.GAP).all()
    return flat.reshape(shape), redrawn


def occupancy(ref, pcs, res, clip):
    """the reference on the set, and on each cloud alone for the per-cloud counts"""
    ent, counters = ref._entropy_of_occupancy_grid(torch.from_numpy(pcs), res, clip)
    bern = np.zeros(len(counters), dtype=np.int32)
    for s in range(len(pcs)):
        bern += ref._entropy_of_occupancy_grid(torch.from_numpy(pcs[s:s + 1]), res, clip)[1] > 0
    assert (counters == np.round(counters)).all()
    return np.float64(ent), counters.astype(np.int32), bern


def mask_of(ref, res):
    full = ref._unit_cube_grid_point_cloud(res, False)[0].reshape(-1, 3)
    clipped, spacing = ref._unit_cube_grid_point_cloud(res, True)
    key = lambda a: np.ascontiguousarray(a).view([("", a.dtype)] * 3).reshape(-1)  # noqa: E731
    mask = np.isin(key(full), key(clipped))
    assert np.array_equal(full[mask], clipped)
    return mask, spacing, clipped


if __name__ == "__main__":
    check_imports_resolve()
    ref = _by_path("_ref3d_jsd", os.path.join(REF, "soft_intro_vae_3d", "metrics", "jsd.py"))
    g = np.random.Generator(np.random.PCG64(2028))
    out = {}
    m28, sp28, cells28 = mask_of(ref, 28)
    m8, sp8, _ = mask_of(ref, 8)
    cells8 = ref._unit_cube_grid_point_cloud(8, False)[0].reshape(-1, 3)
    out.update(mask28=np.packbits(m28), mask8=np.packbits(m8), spacing28=np.float64(sp28), spacing8=np.float64(sp8))
    assert len(cells28) == 10144

    a_s, r1 = draw(g, (3, 2048, 3), 1.0, cells28)
    a_r, r2 = draw(g, (2, 2048, 3), 0.8, cells28)
    out["A_sample"], out["A_ref"] = a_s, a_r
    out["A_sample_entropy"], out["A_sample_counters"], out["A_sample_bernoulli"] = occupancy(ref, a_s, 28, True)
    out["A_ref_entropy"], out["A_ref_counters"], out["A_ref_bernoulli"] = occupancy(ref, a_r, 28, True)
    out["A_jsd"] = np.float64(ref.jsd_between_point_cloud_sets(torch.from_numpy(a_s), torch.from_numpy(a_r), voxels=28))

    b, r3 = draw(g, (5, 333, 3), 1.3, cells28)
    b[1] = b[0]
    b[2, 16:32] = b[2, 0:16]
    assert (JO.nearest(b.reshape(-1, 3), cells28)[1] >= JO.GAP).all()
    out["B_pcs"] = b
    out["B_entropy"], out["B_counters"], out["B_bernoulli"] = occupancy(ref, b, 28, True)
    assert not np.array_equal(out["B_counters"], out["B_bernoulli"])

    c, r4 = draw(g, (4, 100, 3), 1.1, cells8)
    out["C_pcs"] = c
    out["C_entropy"], out["C_counters"], out["C_bernoulli"] = occupancy(ref, c, 8, False)

    d1 = ((g.random(size=(4, 100, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
    d2 = ((g.random(size=(4, 100, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(1.2)).astype(np.float32)
    out["D_pc1"], out["D_pc2"] = d1, d2
    for v in (64, 28):
        out["D_counts1_%d" % v] = ref._pc_to_voxel_distribution(torch.from_numpy(d1), v)
        out["D_counts2_%d" % v] = ref._pc_to_voxel_distribution(torch.from_numpy(d2), v)
        out["D_jsd_%d" % v] = np.float64(ref.js_divercence_between_pc(torch.from_numpy(d1), torch.from_numpy(d2), v))

    e, r5 = draw(g, (1, 1, 3), 1.0, cells28)
    out["E_pcs"] = e
    nn = ref.NearestNeighbors(n_neighbors=1).fit(cells28)
    e_counters = np.zeros(len(cells28), dtype=np.int32)
    e_counters[int(nn.kneighbors(e[0])[1][0, 0])] = 1
    out["E_counters"], out["E_bernoulli"] = e_counters, e_counters.copy()

    path = os.path.join(HERE, "pc3d_jsd.npz")
    np.savez_compressed(path, **out)
    print("pc3d_jsd: redraws A %d + %d, B %d, C %d, E %d; JSD(A) %.12g; %d bytes"
          % (r1, r2, r3, r4, r5, float(out["A_jsd"]), os.path.getsize(path)))
