"""Keeps the check cases of the style kernels in step with their launch logic, without a GPU: the thresholds of
csrc/style.hip's dispatch and the tile constants of csrc/rgb.hip are read out of the sources, and every configuration and
edge they define must have a case in CASES + EDGE_CASES of tests/style_oracle.py / tests/style_rgb_oracle.py (which
tests/test_style_gpu.py, test_style_net_gpu.py and test_style_edges_gpu.py run).  A moved threshold, a new branch or another
tile size fails here and says which kind of case is missing; a reformatted macro fails the count of branches found."""
import math
import os
import re

import pytest
import torch

import style_oracle as O
import style_rgb_oracle as R

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soft-intro-vae-pytorch_amd", "csrc")
INF = float("inf")


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def defines(text):
    return {k: int(v) for k, v in re.findall(r"^#define\s+(\w+)\s+(\d+)\b", text, re.M)}


def dispatch(text, macro):
    """the branches of ST_DISPATCH_FWD / _BWD -> [(low, high, NT, EPT)]: low < H W <= high, EPT = 0 the streamed form"""
    body = re.search(r"#define %s\(.*?while \(0\)" % macro, text, re.S).group(0)
    consts = defines(text)
    held = re.findall(r"if \(\(HW\) <= (\w+)\) ST_LAUNCH\(KERN, (\d+), (\d+),", body)
    last = re.findall(r"^\s*else ST_LAUNCH\(KERN, (\d+), (\d+),", body, re.M)
    assert len(last) == 1 and len(held) + 1 == body.count("ST_LAUNCH("), "the dispatch macro is not in the shape this test reads"
    out, low = [], 0
    for bound, nt, ept in held:
        high = int(bound) if bound.isdigit() else consts[bound]
        assert high > low, (macro, bound)
        out.append((low, high, int(nt), int(ept)))
        low = high
    return out + [(low, INF, int(last[0][0]), int(last[0][1]))]


@pytest.fixture(scope="module")
def style_src():
    return source("style.hip")


@pytest.fixture(scope="module")
def rgb_consts():
    text = source("rgb.hip")
    d = defines(text)
    stride = re.findall(r"for \(size_t q = threadIdx\.x; q < NB; q \+= (\d+)\)", text)
    assert len(stride) == 1, "rgb_merge_kernel's loop over the blocks is not in the shape this test reads"
    assert {"RGB_TILE", "RGB_NW"} <= set(d)
    return dict(tile=d["RGB_TILE"], nw=d["RGB_NW"], merge=int(stride[0]))


STYLE_HW = sorted({c[2] * c[3] for c in O.CASES + O.EDGE_CASES})


# ------------------------------------------------------------------------------------------------ style.hip
def test_the_dispatch_is_read_whole(style_src):
    fwd, bwd = dispatch(style_src, "ST_DISPATCH_FWD"), dispatch(style_src, "ST_DISPATCH_BWD")
    assert len(fwd) == 6 and len(bwd) == 5
    c = defines(style_src)
    assert fwd[-2][1] == c["ST_MAX_HELD_FWD"] and bwd[-2][1] == c["ST_MAX_HELD_BWD"]
    for table in (fwd, bwd):
        assert table[-1][3] == 0 and all(ept > 0 and ept % 4 == 0 for _, _, _, ept in table[:-1])
        for low, high, nt, ept in table[:-1]:
            assert high <= nt * ept, "a held configuration too small for its planes"


@pytest.mark.parametrize("macro", ["ST_DISPATCH_FWD", "ST_DISPATCH_BWD"])
def test_every_style_configuration_and_edge_has_a_case(style_src, macro):
    table = dispatch(style_src, macro)
    for idx, (low, high, nt, ept) in enumerate(table):
        what = "%s <%d, %d> (%s < H W <= %s)" % (macro, nt, ept, low, high)
        inside = [hw for hw in STYLE_HW if low < hw <= high]
        assert inside, "no case in " + what
        assert any(hw % 4 for hw in inside), "no case with a scalar tail in " + what
        assert any(hw % 4 == 0 for hw in inside), "no case on the 16-byte path in " + what
        if ept and idx > 0:
            assert any(hw < nt * ept for hw in inside), "no case that leaves a slot unfilled in " + what
        if ept > 4:  # (a slot no thread fills, and one that only some threads fill)
            assert any(hw <= nt * (ept - 4) for hw in inside), "no case that skips a whole slot in " + what
            assert any(hw % (4 * nt) for hw in inside), "no case with a partly filled slot in " + what
        if not ept:  # (the streamed loop: a last stride that is not full)
            assert any(hw % (4 * nt) for hw in inside), "no case with a partial last stride in " + what


def test_planted_indices(style_src):
    """inside the plane, and where the docstring of O.planted says: s is the first element of the second chunk of thread 0
    of a block of s / 4 threads, for every block size the dispatch uses"""
    nts = {nt for m in ("ST_DISPATCH_FWD", "ST_DISPATCH_BWD") for _, _, nt, _ in dispatch(style_src, m)}
    assert {4 * nt for nt in nts} == set(O.PLANT_STRIDES)
    assert set(O.EDGE_CASES) < set(O.PLANT_CASES) and (1, 1, 256, 256) in O.PLANT_CASES
    for case in O.PLANT_CASES:
        n = case[2] * case[3]
        at = O.planted(n)
        assert all(0 <= e < n for e in at), case
        lone_last = any(2 * s < n and (n - 1) % s == 0 for s in O.PLANT_STRIDES)  # (n - 1 starts the last round itself)
        assert at[0] == -32.0 and at[n - 1] == (-24.0 if lone_last else 64.0)
        want = {0, n - 1} | {e for s in O.PLANT_STRIDES if 2 * s < n for e in (s, (n - 1) // s * s)}
        assert set(at) == want and all(float(torch.tensor(v, dtype=torch.float32)) == v for v in at.values())
        d = O.plant(O.enc_inputs(case))
        flat = d["x"].flatten(2)
        assert all(bool((flat[:, :, e] == v).all()) for e, v in at.items()) and d["g"].flatten(2)[0, 0, n - 1] == at[n - 1]
    assert sorted(O.planted(66045)) == [0, 256, 1024, 4096, 65536, 65792, 66044] and sorted(O.planted(256)) == [0, 255]


# ------------------------------------------------------------------------------------------------ rgb.hip
def rgb_runs():
    """(K, C, B, H W of the kernels' planes, pooled) of every run the GPU tests make of an RGB case"""
    for case in R.CASES + R.EDGE_CASES:
        B, C, H, W, K = case
        for blend in R.variants(case):
            yield K, C, B, H * W, False                              # to_rgb (plain or blended), from_rgb plain
            if blend is not None:
                yield K, C, B, (H // 2) * (W // 2), True             # from_rgb on the pooled image


def test_every_rgb_configuration_and_edge_has_a_case(rgb_consts):
    tile, nw, merge = rgb_consts["tile"], rgb_consts["nw"], rgb_consts["merge"]
    runs = list(rgb_runs())
    assert {k for k, *_ in runs} == {1, 2, 3, 4}
    nb = lambda b, hw: b * math.ceil(hw / tile)  # noqa: E731
    assert any(k < 4 and nb(b, hw) > merge for k, _, b, hw, _ in runs), "no K < 4 case with more blocks than merge threads"
    assert any(k == 4 and nb(b, hw) > merge for k, _, b, hw, _ in runs), "no K = 4 case with more blocks than merge threads"
    for pooled in (False, True):
        assert any(hw > tile and hw % tile and p == pooled for _, _, _, hw, p in runs), \
            "no case of several tiles with a partial last one, pooled %s" % pooled
        assert any(hw > tile and hw % 4 == 0 and p == pooled for _, _, _, hw, p in runs)
    assert any(hw > tile and hw % 4 for _, _, _, hw, _ in runs), "no case of several tiles with scalar accesses"
    assert any(c > nw and c % nw for _, c, *_ in runs), "no case whose channels do not divide among the waves"
    # waves that start past C (cpw (nw - 1) >= C), and a wave with fewer channels than the others
    assert any(math.ceil(c / nw) * (nw - 1) >= c and c > nw for _, c, *_ in runs)
    assert any(k == 4 and c > nw and c % 2 for k, c, *_ in runs), "no K = 4 case with an odd C beyond one channel a wave"


# ------------------------------------------------------------------------------------------------ the gates' provenance
def quoted(module, oracle):
    """(forward, gradients) of the line a GPU test's docstring quotes from `python <oracle>.py`"""
    m = re.search(r"cd tests && python %s\.py\n\s+float32 restatement vs float64 over CASES and EDGE_CASES: "
                  r"forward (\S+), gradients (\S+)\n" % oracle, module.__doc__)
    assert m, "the docstring does not quote the oracle's line"
    return float(m.group(1)), float(m.group(2))


@pytest.mark.parametrize("which", ["style", "rgb"])
def test_the_float32_loss_is_what_the_gpu_tests_quote(which):
    """the gates are 4 x the float32 restatement's own loss over BOTH lists: measured here, it is not above the quoted
    figures (to the digits quoted), and FP32_GRAD_LOSS is the quoted figure"""
    if which == "style":
        import test_style_gpu as T
        fwd, grad = O.fp32_loss()
        q = quoted(T, "style_oracle")
    else:
        import test_style_net_gpu as T
        fwd, grad = R.fp32_loss()
        q = quoted(T, "style_rgb_oracle")
    print("%s: forward %.3e (quoted %.3e), gradients %.3e (quoted %.3e)" % (which, fwd, q[0], grad, q[1]))
    assert T.FP32_GRAD_LOSS == q[1] and T.GRAD_GATE == min(4 * q[1], 1e-4)
    assert float("%.3e" % fwd) <= q[0] and float("%.3e" % grad) <= q[1]


def test_from_inputs_finds_a_seed_for_every_edge_case():
    import test_style_edges_gpu as E
    variants = [(c, b) for c in R.EDGE_CASES for b in R.variants(c)] + E.RGB_BIT_VARIANTS
    for case, blend in variants:
        d = R.from_inputs(case, blend)
        assert 0 <= d["seed"] < R.MAX_SEEDS and R.kink_margin(d) >= R.KINK_MARGIN, (case, blend)
    assert R.MAX_SEEDS == 64
