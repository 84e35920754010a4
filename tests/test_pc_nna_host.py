"""CPU-side checks of the 3-D variant's 1-nearest-neighbour accuracy (csrc/pc_eval.hip: sivae_chamfer_matrix_self,
sivae_nn1_loo; sivae_hip.pointcloud.chamfer_matrix_self / nn1_loo; one_nn_accuracy of
soft_intro_vae_3d/metrics/evaluation_metrics.py): the argument validation of the entry points (every call returns before
any launch), the float64 oracle tests/pc3d_nna_oracle.py against hand-computed matrices, the folded-row walk of the
triangle, and the Python surface."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import pc3d_nna_oracle as NO
from sivae_hip import lib

INF, NAN = float("inf"), float("nan")


def test_pc_nna_entry_points_validate_arguments():
    """null pointers, non-positive sizes, folded-row ranges outside 0 <= f0 < f1 <= ceil(S / 2) for odd and even S,
    S S and (S + R)^2 >= 2^31 - 1, flags outside {0, 1}, a short or null workspace: the documented codes, in the manner of
    test_pc_eval_host.py"""
    L = lib.load()
    null, one = None, ctypes.c_void_p(16)
    f = L.sivae_chamfer_matrix_self
    ok = dict(clouds=one, ss=30, sn=3, sc=1, D=one, S=4, M=10, f0=0, f1=2, norm=1, sqrt=0, ws=one, ws_bytes=0, stream=null)

    def cs(**kw):
        a = dict(ok, **kw)
        return f(*[a[k] for k in ok])

    for k in ("clouds", "D"):
        assert cs(**{k: null}) == -1, k
    for k in ("S", "M"):
        assert cs(**{k: 0}) == -2 and cs(**{k: -3}) == -2, k
    assert cs(f0=1, f1=1) == -2 and cs(f0=2, f1=1) == -2 and cs(f0=-1) == -2     # empty, reversed, negative
    assert cs(S=4, f1=3) == -2 and cs(S=5, f1=4) == -2 and cs(S=1, f1=2) == -2   # f1 > ceil(S / 2), even and odd S
    assert cs(S=46341, f1=1) == -5                       # 46341^2 = 2^31 + 88 633
    assert cs(S=46340, f1=1, sqrt=5) == -6               # (46340^2 < 2^31 - 1 passes the range check)
    assert cs(norm=2) == -6 and cs(sqrt=-1) == -6
    assert cs(ws=null) == -4                             # (a null workspace is refused even where none is used)
    wb = L.sivae_chamfer_matrix_self_workspace_bytes
    assert wb(2, 4, 10) == 0 and wb(2, 4, 1024) == 0 and wb(2, 4, 1025) == 0 and wb(2, 4, 2048) == 0
    need = wb(2, 4, 2053)                                # several chunks on both sides: M words per launched block
    assert need == 2 * 5 * 2053 * 4
    assert wb(1200, 2400, 2053) == 2048 * 2053 * 4       # (the grid is capped at 2048 blocks)
    assert wb(0, 4, 2053) == 0 and wb(3, 4, 2053) == 0 and wb(1, 46341, 2053) == 0
    assert cs(M=2053, ws_bytes=need - 1) == -4
    n = L.sivae_nn1_loo
    for i in (0, 1, 2, 5, 6):                            # Dss, Dsr, Drr, S, R, nn_val, nn_arg
        args = [one, one, one, 4, 5, one, one]
        args[i] = null
        assert n(*args, null) == -1, i
    for S, R in ((0, 5), (4, 0), (-1, 5), (4, -2)):
        assert n(one, one, one, S, R, one, one, null) == -2, (S, R)
    assert n(one, one, one, 46340, 1, one, one, null) == -5 and n(one, one, one, 1, 0x7ffffffe, one, one, null) == -5
    assert L.sivae_abi_version() == 1
    new = sorted(name for name in lib.prototypes() if "matrix_self" in name or "nn1" in name)    # (no test hook among them)
    assert new == ["sivae_chamfer_matrix_self", "sivae_chamfer_matrix_self_workspace_bytes", "sivae_nn1_loo"]


def test_folded_rows_walk_every_pair_once():
    """the walk stated in include/sivae_hip.h, restated: for S = 1 .. 39 every (s <= r) exactly once and nothing else"""
    for S in range(1, 40):
        seen = []
        for f in range((S + 1) // 2):
            for c in range(S + 1):
                if c < S - f:
                    seen.append((f, f + c))
                elif S - 1 - f != f:
                    seen.append((S - 1 - f, S - 1 - f + c - (S - f)))
        assert sorted(seen) == [(s, r) for s in range(S) for r in range(s, S)], S


def test_oracle_against_hand_computed_matrices():
    # two samples, two references; item 0's candidates 5 (1), 2 (2), 7 (3) -> 2; item 1: 5 (0), 9 (2), 1 (3) -> 3;
    # item 2 (reference 0): column 0 of Dsr = 2 (0), 9 (1), then 4 (3) -> 0; item 3: 7 (0), 1 (1), 4 (2) -> 1
    Dss = [[0.0, 5.0], [5.0, 0.0]]
    Dsr = [[2.0, 7.0], [9.0, 1.0]]
    Drr = [[0.0, 4.0], [4.0, 0.0]]
    val, arg = NO.nn1_loo(Dss, Dsr, Drr)
    assert arg.tolist() == [2, 3, 0, 1] and val.tolist() == [2.0, 1.0, 2.0, 1.0]
    r = NO.one_nn_accuracy(Dss, Dsr, Drr)
    assert (r["acc"], r["acc_sample"], r["acc_ref"]) == (0.0, 0.0, 0.0)
    assert NO.smallest_gap(Dss, Dsr, Drr) == min(3 / 5, 4 / 5, 2 / 4, 3 / 4)
    # the diagonal is never a candidate, whatever it holds
    for d in (0.0, -1.0, NAN, INF):
        A, B = np.array(Dss), np.array(Drr)
        np.fill_diagonal(A, d)
        np.fill_diagonal(B, d)
        assert NO.nn1_loo(A, Dsr, B)[1].tolist() == [2, 3, 0, 1]
    # a tie between a candidate of each set: the lowest joint index wins (item 0: 3 at items 1 and 2; item 3: 6 at
    # items 1 and 2)
    Dss = [[0.0, 3.0], [3.0, 0.0]]
    Dsr = [[3.0, 8.0], [9.0, 6.0]]
    Drr = [[0.0, 6.0], [6.0, 0.0]]
    val, arg = NO.nn1_loo(Dss, Dsr, Drr)
    assert arg.tolist() == [1, 0, 0, 1] and val.tolist() == [3.0, 3.0, 3.0, 6.0]
    r = NO.one_nn_accuracy(Dss, Dsr, Drr)
    assert (r["acc"], r["acc_sample"], r["acc_ref"]) == (0.5, 1.0, 0.0)
    assert NO.smallest_gap(Dss, Dsr, Drr) == 0.0
    # an item whose only finite candidate is in the other set (item 0), one with none at all (item 1: (+inf, -1)),
    # and a NaN that must not win (item 2: NaN at item 1, 4 at item 0, 5 at item 3)
    Dss = [[0.0, INF], [INF, 0.0]]
    Dsr = [[4.0, NAN], [NAN, INF]]
    Drr = [[0.0, 5.0], [5.0, 0.0]]
    val, arg = NO.nn1_loo(Dss, Dsr, Drr)
    assert arg.tolist() == [2, -1, 0, 2] and val.tolist() == [4.0, INF, 4.0, 5.0]
    # S = 1: the sample's candidates are all references; R = 1 likewise; S = R = 1: each has the other only
    val, arg = NO.nn1_loo([[0.0]], [[3.0, 2.0, 2.0]], [[0, 1, 9], [1, 0, 9], [9, 9, 0]])
    assert arg.tolist() == [2, 2, 1, 0] and val.tolist() == [2.0, 1.0, 1.0, 2.0]
    r = NO.one_nn_accuracy([[0.0]], [[3.0, 2.0, 2.0]], [[0, 1, 9], [1, 0, 9], [9, 9, 0]])
    assert (r["acc"], r["acc_sample"], r["acc_ref"]) == (0.5, 0.0, 2 / 3)
    val, arg = NO.nn1_loo([[0, 1, 9], [1, 0, 9], [9, 9, 0]], [[3.0], [2.0], [2.0]], [[0.0]])
    assert arg.tolist() == [1, 0, 3, 1] and val.tolist() == [1.0, 1.0, 2.0, 2.0]
    val, arg = NO.nn1_loo([[0.0]], [[7.0]], [[0.0]])
    assert arg.tolist() == [1, 0] and val.tolist() == [7.0, 7.0]
    assert NO.smallest_gap([[0.0]], [[7.0]], [[0.0]]) == 1.0
    # a non-symmetric Dss: item t reads ROW t (item 0: Dss[0][1] = 1 -> 1; item 1: Dss[1][0] = 8, Dsr[1][0] = 2 -> 2)
    val, arg = NO.nn1_loo([[0.0, 1.0], [8.0, 0.0]], [[5.0], [2.0]], [[0.0]])
    assert arg.tolist() == [1, 2, 1] and val.tolist() == [1.0, 2.0, 2.0]


def test_pointcloud_surface_rejects_cpu_tensors_and_wrong_ranks():
    from sivae_hip import pointcloud as PC
    assert list(inspect.signature(PC.chamfer_matrix_self).parameters) == ["clouds", "normalize", "use_sqrt"]
    assert inspect.signature(PC.chamfer_matrix_self).parameters["normalize"].default is True
    assert inspect.signature(PC.chamfer_matrix_self).parameters["use_sqrt"].default is False
    assert list(inspect.signature(PC.nn1_loo).parameters) == ["Dss", "Dsr", "Drr"]
    x = torch.zeros(2, 5, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.chamfer_matrix_self(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PC.nn1_loo(torch.zeros(2, 2), torch.zeros(2, 3), torch.zeros(3, 3))
    for bad in (torch.zeros(5, 3), torch.zeros(2, 3, 5), torch.zeros(2, 5, 3, 1)):
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            PC.chamfer_matrix_self(bad)
    for bad in ((torch.zeros(4), torch.zeros(2, 3), torch.zeros(3, 3)),            # rank
                (torch.zeros(2, 2), torch.zeros(2, 3, 1), torch.zeros(3, 3)),
                (torch.zeros(2, 2), torch.zeros(2, 0), torch.zeros(0, 0)),         # empty
                (torch.zeros(3, 3), torch.zeros(2, 3), torch.zeros(3, 3)),         # Dss is not [S, S]
                (torch.zeros(2, 2), torch.zeros(2, 3), torch.zeros(3, 2))):        # Drr is not [R, R]
        with pytest.raises(ValueError, match=r"nn1_loo"):
            PC.nn1_loo(*bad)
    # the module's idiom: checks, allocation through the module's torch / workspace (what tests/support/guard.py patches)
    src = inspect.getsource(PC.chamfer_matrix_self)
    assert "_require_clouds(" in src and "workspace(" in src and "torch.empty(" in src and "timer_end(" in src
    assert "MATRIX_POINT_PAIRS_PER_LAUNCH // ((S + 1) * M * M)" in src
    src = inspect.getsource(PC.nn1_loo)
    assert "_require_f32(" in src and "torch.empty(" in src and "timer_end(" in src
    assert "chamfer_matrix_self(clouds [S, M, 3]" in PC.__doc__ and "nn1_loo(Dss [S, S], Dsr [S, R], Drr [R, R])" in PC.__doc__


def test_drop_in_module_surface():
    import soft_intro_vae_3d.metrics.evaluation_metrics as E
    assert "chamfer_matrix_self" in E.__all__ and "one_nn_accuracy" in E.__all__
    assert list(inspect.signature(E.chamfer_matrix_self).parameters) == ["pcs", "normalize", "use_sqrt"]
    sig = inspect.signature(E.one_nn_accuracy)
    assert list(sig.parameters) == ["sample_pcs", "ref_pcs", "normalize", "use_sqrt", "metric", "dist", "dist_ss", "dist_rr"]
    assert sig.parameters["normalize"].default is True and sig.parameters["use_sqrt"].default is False
    assert sig.parameters["metric"].default == "cd"
    assert all(sig.parameters[k].default is None for k in ("dist", "dist_ss", "dist_rr"))
    x = np.zeros((2, 5, 3), dtype=np.float32)
    for metric in ("l2", "CD", None):
        with pytest.raises(ValueError, match="metric"):      # (before a device is asked for)
            E.one_nn_accuracy(x, x, metric=metric)
    for metric in ("cd", "emd"):
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            E.one_nn_accuracy(np.zeros((5, 3), dtype=np.float32), x, metric=metric)
        with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
            E.one_nn_accuracy(torch.zeros(2, 5, 3), torch.zeros(2, 3, 5), metric=metric)
    with pytest.raises(ValueError, match=r"\[S, N, 3\]"):
        E.chamfer_matrix_self(np.zeros((5, 3), dtype=np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E.chamfer_matrix_self(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            E.one_nn_accuracy(x, x)
    for f in (E.minimum_mathing_distance, E.coverage):       # (use_EMD stays as it is)
        with pytest.raises(NotImplementedError):
            f(x, x, use_EMD=True)
