"""CPU-side checks of the 3-D variant's set-to-set evaluation (csrc/pc_eval.hip, sivae_hip.pointcloud.chamfer_matrix /
match_min, soft_intro_vae_3d/metrics/evaluation_metrics.py): the argument validation of sivae_chamfer_matrix and
sivae_match_min (every call returns before any launch), the Python surface, and the float64 oracle
tests/pc3d_eval_oracle.py against hand-computed clouds."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pc3d_eval_oracle as EO
from sivae_hip import lib


def test_pc_eval_entry_points_validate_arguments():
    """null pointers, non-positive sizes, empty / out-of-range row ranges, S R >= 2^31 - 1, flags outside {0, 1}, a short
    or null workspace: the documented codes, in the manner of test_relu_bn_max_host.py"""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    f = L.sivae_chamfer_matrix
    ok = dict(sample=one, ss=30, sn=3, sc=1, ref=one, rs=30, rn=3, rc=1, D=one, S=4, R=5, M=10, N=10, s0=0, s1=4, norm=1,
              sqrt=0, ws=one, ws_bytes=0, stream=null)

    def cm(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("sample", "ref", "D"):
        assert cm(**{k: null}) == -1, k
    for k in ("S", "R", "M", "N"):
        assert cm(**{k: 0}) == -2 and cm(**{k: -3}) == -2, k
    assert cm(s0=2, s1=2) == -2 and cm(s0=3, s1=2) == -2 and cm(s0=-1) == -2 and cm(s1=5) == -2  # row range
    assert cm(S=1 << 16, R=1 << 15, s1=1) == -5
    assert cm(S=0x7fffffff, R=1, s1=1) == -5            # (the bound itself is refused)
    assert cm(norm=2) == -6 and cm(sqrt=-1) == -6
    assert cm(ws=null) == -4                             # (a null workspace is refused even where none is used)
    wb = L.sivae_chamfer_matrix_workspace_bytes
    assert wb(4, 5, 10, 10) == 0 and wb(4, 5, 2049, 1024) == 0 and wb(4, 5, 2048, 5000) == 0
    need = wb(4, 5, 2049, 1025)                          # both clouds in several chunks: one stretch of N words per block
    assert need == 4 * 5 * 1025 * 4
    assert wb(3000, 800, 2049, 1025) == 2048 * 1025 * 4  # (the grid is capped at 2048 blocks)
    assert wb(0, 5, 10, 10) == 0 and wb(1 << 16, 1 << 15, 10, 10) == 0
    assert cm(M=2049, N=1025, ws_bytes=need - 1) == -4
    m = L.sivae_match_min
    ok = [one] * 7                                       # D, S, R, row_min, row_arg, col_min, col_arg
    for i in (0, 3, 4, 5, 6):
        args = [one, 4, 5, one, one, one, one]
        args[i] = null
        assert m(*args, null) == -1, i
    for S, R in ((0, 5), (4, 0), (-1, 5), (4, -2)):
        assert m(one, S, R, one, one, one, one, null) == -2, (S, R)
    assert m(one, 1 << 16, 1 << 15, one, one, one, one, null) == -5
    assert m(one, 1, 0x7fffffff, one, one, one, one, null) == -5
    assert L.sivae_abi_version() == 1


def test_pointcloud_surface_rejects_cpu_tensors_and_wrong_ranks():
    from sivae_hip import pointcloud as PC
    x = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.chamfer_matrix(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.match_min(torch.zeros(2, 3))
    for bad in (torch.zeros(5, 3), torch.zeros(2, 3, 5), torch.zeros(2, 5, 3, 1)):
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            PC.chamfer_matrix(bad, x)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            PC.chamfer_matrix(x, bad)
    for bad in (torch.zeros(4), torch.zeros(2, 3, 4), torch.zeros(0, 3)):
        with pytest.raises(ValueError, match=r"\[S, R\]"):
            PC.match_min(bad)
    # the module's idiom: checks, allocation through the module's torch / workspace (what tests/support/guard.py patches)
    src = inspect.getsource(PC.chamfer_matrix)
    assert "_require_clouds(" in src and "workspace(" in src and "torch.empty(" in src and "timer_end(" in src
    assert "MATRIX_POINT_PAIRS_PER_LAUNCH" in src and PC.MATRIX_POINT_PAIRS_PER_LAUNCH > 0
    src = inspect.getsource(PC.match_min)
    assert "_require_f32(" in src and "torch.empty(" in src and "timer_end(" in src
    assert "chamfer_matrix(sample [S, M, 3], ref [R, N, 3]" in PC.__doc__ and "match_min(D [S, R])" in PC.__doc__


def test_drop_in_module_surface():
    import soft_intro_vae_3d.metrics.evaluation_metrics as E
    assert E.minimum_matching_distance is E.minimum_mathing_distance
    sig = inspect.signature(E.minimum_mathing_distance)
    assert list(sig.parameters)[:8] == ["sample_pcs", "ref_pcs", "batch_size", "normalize", "sess", "verbose", "use_sqrt",
                                        "use_EMD"]
    assert sig.parameters["normalize"].default is True and sig.parameters["use_sqrt"].default is False
    sig = inspect.signature(E.coverage)
    assert list(sig.parameters)[:9] == ["sample_pcs", "ref_pcs", "batch_size", "normalize", "sess", "verbose", "use_sqrt",
                                        "use_EMD", "ret_dist"]
    assert "dist" in sig.parameters and "dist" in inspect.signature(E.minimum_mathing_distance).parameters
    x = np.zeros((2, 5, 3), dtype=np.float32)
    for f in (E.minimum_mathing_distance, E.coverage):
        with pytest.raises(NotImplementedError):
            f(x, x, use_EMD=True)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            f(np.zeros((5, 3), dtype=np.float32), x)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            f(torch.zeros(2, 5, 3), torch.zeros(2, 3, 5))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E.chamfer_matrix(x, x)
    src = inspect.getsource(E)
    for banned in ("tensorflow", "scipy", "sklearn"):
        assert "import " + banned not in src and "from " + banned not in src
    import __graft_entry__ as G
    assert "soft_intro_vae_3d.metrics.evaluation_metrics" in inspect.getsource(G.build)


def test_oracle_against_hand_computed_clouds():
    # P = {(0,0,0), (1,0,0)}, Q = {(0,0,0), (0,2,0)}:  |P_j - Q_i|^2 = [[0, 4], [1, 5]]  (rows j, columns i)
    P = np.array([[[0, 0, 0], [1, 0, 0]]], dtype=np.float32)
    Q = np.array([[[0, 0, 0], [0, 2, 0]]], dtype=np.float32)
    # a = (0, 1), b = (0, 4)
    assert EO.chamfer_matrix(P, Q, normalize=False)[0, 0] == 0 + 1 + 0 + 4
    assert EO.chamfer_matrix(P, Q, normalize=True)[0, 0] == 0.5 + 2.0
    assert EO.chamfer_matrix(P, Q, normalize=False, use_sqrt=True)[0, 0] == 1 + 2
    assert EO.chamfer_matrix(P, Q, normalize=True, use_sqrt=True)[0, 0] == 0.5 + 1.0
    # different sizes: one point against two
    P1 = P[:, 1:]                                                             # {(1,0,0)}: distances (1, 5)
    assert EO.chamfer_matrix(P1, Q, normalize=True)[0, 0] == 1.0 / 1 + (1 + 5) / 2
    # a set against itself and another cloud: D = [[0, x], [x, 0]]
    both = np.concatenate([P, Q])
    D = EO.chamfer_matrix(both, both, normalize=False)
    assert D.shape == (2, 2) and D[0, 0] == 0 and D[1, 1] == 0 and D[0, 1] == 5 and D[1, 0] == 5
    mmd, matched, arg = EO.minimum_matching_distance(D)
    assert mmd == 0.0 and matched.tolist() == [0, 0] and arg.tolist() == [0, 1]
    cov, ref, dist = EO.coverage(D)
    assert cov == 1.0 and ref.tolist() == [0, 1] and dist.tolist() == [0, 0]
    # ties: the lowest index; coverage counts distinct references
    D = np.array([[3.0, 1.0, 1.0], [2.0, 5.0, 2.0], [9.0, 1.0, 4.0]])
    rm, ra, cm, ca = EO.match_min(D)
    assert ra.tolist() == [1, 0, 1] and rm.tolist() == [1, 2, 1] and ca.tolist() == [1, 0, 0] and cm.tolist() == [2, 1, 1]
    assert EO.coverage(D)[0] == 2 / 3 and EO.minimum_matching_distance(D)[0] == 4 / 3
    assert EO.smallest_gap(np.array([[1.0, 2.0], [4.0, 3.0]])) == 0.25      # rows 1/2, 1/4; columns 3/4, 1/3
    # a non-finite coordinate: its row / column, nothing else
    bad = both.copy()
    bad[0, 1, 2] = np.nan
    D = EO.chamfer_matrix(bad, both)
    assert np.isnan(D[0]).all() and np.isfinite(D[1]).all()
    bad = both.copy()
    bad[1, 0, 0] = np.inf
    D = EO.chamfer_matrix(both, bad)
    assert np.isnan(D[:, 1]).all() and np.isfinite(D[:, 0]).all()
