"""CPU-side checks of the 3-D variant's earth mover's reconstruction loss (csrc/pc_emd.hip::emd_loss_kernel,
sivae_hip.pointcloud.emd_loss_fwd / emd_distance, soft_intro_vae_3d/losses/earth_mover_distance.py::EMD): the gradient
oracle tests/pc3d_emd_grad_oracle.py against an exact matching and its two identities, the new prototypes and the
argument validation of sivae_emd_loss (every call returns before any launch), and the Python surface."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pc3d_emd_grad_oracle as GO
from sivae_hip import lib


# ------------------------------------------------------------------------------------------------ the oracle
def test_gradient_oracle_against_an_exact_matching():
    """64 points on a 4 x 4 x 4 grid of spacing 0.25 against the same points displaced by 0.02 in random directions and
    permuted: at the first level (exp(-16384 d2)) a point's own copy weighs 1.4e-3 and every other point at most
    exp(-16384 0.23^2) = 0, so the plan is the permutation to the 1e-9 of step 1; both gradients are the unit vectors of
    the matched pairs and the cost is the sum of the matched distances (measured: 6e-10)."""
    rng = np.random.default_rng(64)
    g = (np.arange(4) - 1.5) * 0.25
    A = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(64, 3)
    step = rng.standard_normal((64, 3))
    step *= 0.02 / np.sqrt((step * step).sum(axis=1, keepdims=True))
    perm = rng.permutation(64)
    B = (A + step)[perm]                       # B[i] is the displaced copy of A[perm[i]]
    cost, dleft, dright = GO.emd_grad(A, B)
    unit = -step / 0.02                        # (A_k - B_match(k)) / |.|
    err_l, err_r = np.abs(dleft - unit).max(), np.abs(dright + unit[perm]).max()
    print("exact matching: cost off by %.3e, dleft by %.3e, dright by %.3e" % (abs(cost - 64 * 0.02), err_l, err_r))
    assert abs(cost - 64 * 0.02) <= 1e-8 and err_l <= 1e-8 and err_r <= 1e-8
    cn, ln, rn = GO.emd_grad(A, B, normalize=True)
    assert abs(cn - cost / 64) <= 1e-15 and np.array_equal(ln, dleft / 64) and np.array_equal(rn, dright / 64)


@pytest.mark.parametrize("n,m", [(1, 1), (5, 7), (64, 64), (48, 80), (257, 257), (300, 513)])
def test_oracle_identities(n, m):
    """with the plan fixed the cost is 1-homogeneous in the points and does not move under a common translation"""
    rng = np.random.default_rng(1000 * n + m)
    A, B = rng.random((n, 3)) - 0.5, rng.random((m, 3)) - 0.5
    cost, dleft, dright = GO.emd_grad(A, B)
    h, p = GO.homogeneity_defect(A, B, cost, dleft, dright), GO.momentum_defect(dleft, dright)
    print("oracle (%d, %d): homogeneity %.3e, momentum %.3e" % (n, m, h, p))
    assert h <= 1e-12 and p <= 1e-12
    assert dleft.shape == (n, 3) and dright.shape == (m, 3) and dleft.dtype == np.float64
    c32, l32, r32 = GO.emd_grad(A.astype(np.float32), B.astype(np.float32), dtype=np.float32)
    assert l32.dtype == np.float32 and r32.dtype == np.float32


def test_oracle_coincident_points_contribute_nothing():
    A = np.array([[0.25, -0.5, 1.0], [0.0, 0.0, 0.0]])
    cost, dleft, dright = GO.emd_grad(A, A)
    assert np.isfinite(dleft).all() and np.isfinite(dright).all()
    assert np.abs(dleft).max() <= 1e-8 and np.abs(dright).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ the entry point
def test_prototypes_parse_from_the_header():
    protos = lib.parse_header()
    ret, args = protos["sivae_emd_loss"]
    assert ret is ctypes.c_int
    p, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    assert args == [p, ll, ll, ll, p, ll, ll, ll, p, p, p, i, i, i, i, p, ctypes.c_size_t, p]
    ret, args = protos["sivae_emd_loss_workspace_bytes"]
    assert ret is ctypes.c_size_t and args == [i, i, i]
    text = open(lib.HEADER_PATH).read()
    doc = text[text.index("The same quantity as a reconstruction loss"):text.index("size_t sivae_emd_loss_workspace_bytes")]
    for said in ("HELD CONSTANT", "gradcheck does not apply", "left = preds, right = gts", "NaN", "No atomics"):
        assert said in doc, said


def test_emd_loss_entry_point_validates_arguments():
    """null pointers, non-positive sizes, clouds beyond 4096 points, an index at 2^31 - 1, a flag outside {0, 1}, a null
    workspace: the documented codes, in the manner of test_pc_emd_host.py.  Either gradient pointer may be null."""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    f = L.sivae_emd_loss
    ok = dict(left=one, ls=30, ln=3, lc=1, right=one, rs=30, rn=3, rc=1, cost=one, dl=one, dr=one, B=4, N=10, M=10, norm=0,
              ws=one, ws_bytes=0, stream=null)

    def em(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("left", "right", "cost"):
        assert em(**{k: null}) == -1, k
        assert em(**{k: null, "dl": null, "dr": null}) == -1, k
    for k in ("B", "N", "M"):
        assert em(**{k: 0}) == -2 and em(**{k: -3}) == -2, k
    assert em(N=4097) == -5 and em(M=4097) == -5 and em(N=4097, M=4097) == -5
    assert em(B=174763, N=4096, M=1) == -5              # 3 B max(N, M) = 2^31 + 2048
    assert em(B=0x7fffffff, N=1, M=1) == -5
    assert em(B=715827882, N=1, M=1, ws=null) == -4      # 3 B = 2^31 - 2: admitted, refused for its workspace only
    assert em(norm=2) == -6 and em(norm=-1) == -6
    assert em(ws=null) == -4 and em(N=4096, M=4096, ws=null) == -4
    assert em(dl=null, dr=null, ws=null) == -4           # (the gradients are optional: the refusal is the workspace's)
    wb = L.sivae_emd_loss_workspace_bytes
    for args in ((4, 10, 10), (32, 2048, 2048), (1, 4096, 4096), (1, 1, 1), (0, 5, 10), (4, 4097, 10)):
        assert wb(*args) == 0, args
    assert L.sivae_abi_version() == 1


# ------------------------------------------------------------------------------------------------ the Python surface
def test_pointcloud_surface():
    from sivae_hip import pointcloud as PC
    x = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.emd_loss_fwd(x, x, True, True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.emd_distance(x, x)
    for bad in (torch.zeros(5, 3), torch.zeros(2, 3, 5), torch.zeros(2, 5, 3, 1)):
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            PC.emd_loss_fwd(bad, x, True, True)
        with pytest.raises(ValueError, match=r"\[B, N, 3\]"):
            PC.emd_loss_fwd(x, bad, False, True)
    assert list(inspect.signature(PC.emd_loss_fwd).parameters) == ["left", "right", "want_dleft", "want_dright", "normalize"]
    assert inspect.signature(PC.emd_loss_fwd).parameters["normalize"].default is False
    assert list(inspect.signature(PC.emd_distance).parameters) == ["preds", "gts", "normalize"]
    assert inspect.signature(PC.emd_distance).parameters["normalize"].default is False
    src = inspect.getsource(PC.emd_loss_fwd)
    assert src.index("EMD_MAX_POINTS") < src.index("_lib.call(")
    # the module's idiom: checks, allocation through the module's torch / workspace (what tests/support/guard.py patches)
    assert "_require_clouds(" in src and "workspace(" in src and "torch.empty(" in src and "timer_end(" in src
    assert "EMD_LOSS_POINT_PAIRS_PER_LAUNCH" in src and PC.EMD_LOSS_POINT_PAIRS_PER_LAUNCH > 0
    assert "gradcheck" in PC.emd_distance.__doc__ and "emd_distance(preds [B, N, 3], gts [B, M, 3])" in PC.__doc__
    assert issubclass(PC.EmdFn, torch.autograd.Function)


@pytest.mark.parametrize("how", ["left too long", "right too long", "batches differ"])
def test_bad_sizes_raise_before_any_launch(monkeypatch, how):
    """the device check is stood in for (there is no device here); the library must not be reached"""
    from sivae_hip import pointcloud as PC
    small, large, three = torch.zeros(2, 5, 3), torch.zeros(2, 4097, 3), torch.zeros(3, 5, 3)
    monkeypatch.setattr(PC, "_require_clouds", lambda pcs, who: (pcs.shape[0], pcs.shape[1], pcs.stride()))
    monkeypatch.setattr(PC._lib, "call", lambda *a: pytest.fail("the library was called"))
    monkeypatch.setattr(PC._lib, "load", lambda: pytest.fail("the library was asked for a workspace size"))
    left, right, match = {"left too long": (large, small, "4096"), "right too long": (small, large, "4096"),
                          "batches differ": (three, small, "3 left clouds against 2")}[how]
    with pytest.raises(ValueError, match=match):
        PC.emd_loss_fwd(left, right, True, True)


def test_drop_in_module_surface():
    import soft_intro_vae_3d.losses.earth_mover_distance as M
    loss = M.EMD()
    assert isinstance(loss, torch.nn.Module) and not list(loss.parameters())
    assert list(inspect.signature(M.EMD.forward).parameters) == ["self", "preds", "gts"]
    assert list(inspect.signature(M.EMD.__init__).parameters) == ["self"]
    assert "gradcheck" in M.EMD.__doc__ and "unnormalised" in M.EMD.__doc__
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            loss(torch.zeros(2, 5, 3), torch.zeros(2, 5, 3))
