"""GPU checks of the style kernels (csrc/style.hip, csrc/rgb.hip) at every launch configuration and tile edge: the cases of
style_oracle.EDGE_CASES and style_rgb_oracle.EDGE_CASES, which tests/test_style_edges_host.py holds against the thresholds
in the sources.  The checks are those of tests/test_style_gpu.py and tests/test_style_net_gpu.py, called at the new shapes
with their gates unchanged (the forward criterion O.viol <= 1, S.GRAD_GATE = 1e-4 and N.GRAD_GATE = 5.144e-06, both from
the float32 restatement's loss on the CPU over CASES and EDGE_CASES), plus planted planes, which make a plane sum that
drops one element visible to the forward criterion.

What the forward criterion sees of a dropped element.  On the CPU, a float64 restatement of the layer (mode 1, layer 0)
that leaves the LAST element of the plane out of the sums of the mean and of the variance (still divided by H W), against
the full float64 oracle at [1, 1, 255, 259]:

    random inputs (O.dec_inputs)          y at 0.308 of the criterion: it passes
    planted inputs (O.plant of the same)  y at 412.7 times the criterion

One unit-variance element among 66045 moves the mean by 1e-5 of a standard deviation; the planted 64 at the last index moves
it by a thousand times that.  O.planted() puts such values at the first element of a thread's second chunk for each block
size, at the start of the last round of chunks and at both ends of the plane: the elements a wrong slot or stride bound
loses.  The float32 restatement on the planted inputs loses at most 1.8e-07 forward (0.002 of the criterion) and 3.8e-06
in the gradients against float64, so the unchanged gates hold for a correct kernel."""
import functools

import pytest
import torch

import style_oracle as O
import style_rgb_oracle as R
import test_style_gpu as S
import test_style_net_gpu as N

pytestmark = pytest.mark.gpu

DEV = S.DEV
CID = lambda c: "x".join(map(str, c))  # noqa: E731
RGB_VARIANTS = [(c, b) for c in R.EDGE_CASES for b in R.variants(c)]


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize("variant", O.DEC_VARIANTS, ids=lambda v: "mode%d-layer%d%s" % (v[0], v[1], "-nw0" if v[2] else ""))
@pytest.mark.parametrize("case", O.EDGE_CASES, ids=CID)
def test_style_layer_against_the_oracle(case, variant):
    S.test_style_layer_against_the_oracle(case, variant)


@pytest.mark.parametrize("case", O.EDGE_CASES, ids=CID)
def test_stat_norm_against_the_oracle(case):
    S.test_stat_norm_against_the_oracle(case)


@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", RGB_VARIANTS, ids=N.VID)
def test_ops_against_the_oracle(variant, op):
    N.test_ops_against_the_oracle(variant, op)


# ------------------------------------------------------------------------------------------------ planted planes
@functools.lru_cache(maxsize=None)
def planted_dec(case):
    d = O.plant(O.dec_inputs(case, 1))
    return d, O.dec_reference(d, 1, 0)


@functools.lru_cache(maxsize=None)
def planted_enc(case):
    d = O.plant(O.enc_inputs(case))
    return d, O.enc_reference(d)


@pytest.mark.parametrize("case", O.PLANT_CASES, ids=CID)
def test_style_layer_on_planted_planes(case):
    """x and the upstream gradient carry O.planted() in every plane (module docstring): y, the saved statistics and every
    gradient against the float64 oracle"""
    d, ref = planted_dec(case)
    got = S.run_dec(d, 1, 0)
    vs = {k: O.viol(got[k], ref[k]) for k in ("y", "m", "r")}
    errs = {k: O.nerr(got[k], ref[k], ref["lead"] if k in O.LEAD_KEYS else 0.0) for k in ("dx", "dnw", "dbias", "dstyle")}
    print("planted style_layer %s: %s of the criterion; %s (gate %.1e)"
          % (case, ", ".join("%s %.3f" % kv for kv in vs.items()), ", ".join("%s %.2e" % kv for kv in errs.items()),
             S.GRAD_GATE))
    for k, v in vs.items():
        assert got[k].shape == ref[k].shape and v <= 1.0, (k, v)
    for k, e in errs.items():
        assert e <= S.GRAD_GATE, (k, e)


@pytest.mark.parametrize("case", O.PLANT_CASES, ids=CID)
def test_stat_norm_on_planted_planes(case):
    d, ref = planted_enc(case)
    got = S.run_enc(d)
    vs = {k: O.viol(got[k], ref[k]) for k in ("xn", "m", "std")}
    errs = {k: O.nerr(got[k], ref[k]) for k in ("dx", "dbias")}
    print("planted stat_norm %s: %s of the criterion; %s (gate %.1e)"
          % (case, ", ".join("%s %.3f" % kv for kv in vs.items()), ", ".join("%s %.2e" % kv for kv in errs.items()),
             S.GRAD_GATE))
    for k, v in vs.items():
        assert got[k].shape == ref[k].shape and v <= 1.0, (k, v)
    for k, e in errs.items():
        assert e <= S.GRAD_GATE, (k, e)


# ------------------------------------------------------------------------------------------------ bit-identity
# planes in <256, 4>, in <1024, 16> with a partial and an empty slot, in the streamed backward and in the streamed forward;
# H W % 4 = 0 throughout, so the aligned run is the 16-byte instantiation and the shifted one the scalar instantiation
STYLE_BIT_CASES = [(3, 2, 32, 32), (3, 2, 96, 100), (3, 2, 160, 200), (3, 2, 257, 256)]
RGB_BIT_VARIANTS = [((3, 3, 20, 20, 3), 0.25), ((3, 9, 8, 8, 2), 0.25), ((3, 3, 36, 44, 3), 0.25)]


def shifted(t):
    """t on the device one element behind a 512-byte aligned base"""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def sample(d, b, shared):
    """the inputs of sample b alone (the keys in `shared` and what is no tensor stay whole)"""
    return {k: (v if k in shared or not torch.is_tensor(v) else v[b:b + 1]) for k, v in d.items()}


@pytest.mark.parametrize("case", STYLE_BIT_CASES, ids=CID)
def test_style_bits_do_not_depend_on_alignment_batch_or_run(case):
    d, e = O.dec_inputs(case, 1), O.enc_inputs(case)
    for run, inp, planes, shared, per_sample in (
            (lambda t: S.run_dec(t, 1, 0), d, ("x", "noise", "g"), ("noise_weight", "bias"), ("y", "m", "r", "dx", "dstyle")),
            (S.run_enc, e, ("x", "g"), ("bias",), ("xn", "m", "std", "dx"))):
        base = run(inp)
        again = run(inp)
        moved = run({k: (shifted(S.put(v)) if k in planes else v) for k, v in inp.items()})
        alone = run(sample(inp, 1, shared))
        for k in base:
            assert torch.equal(again[k], base[k]), ("two runs", k)
            assert torch.equal(moved[k], base[k]), ("alignment", k)
        for k in per_sample:
            assert torch.equal(alone[k], base[k][1:2]), ("sample 1 alone", k)


@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", RGB_BIT_VARIANTS, ids=N.VID)
def test_rgb_alignment_changes_no_bit(variant, op):
    N.test_alignment_changes_no_bit(variant, op)


@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", RGB_BIT_VARIANTS, ids=N.VID)
def test_rgb_bits_do_not_depend_on_batch_or_run(variant, op):
    """two runs; sample 1 of the three against that sample alone, the forward output and the per-sample gradients (dw and
    dbias are sums over the batch)"""
    case_fn, run, keys, _ = N.RUN[op]
    d, _ = case_fn(*variant)
    base = run(d)
    N.same(run(d), base, keys, "two runs")
    alone = run(sample(d, 1, ("w", "bias")))
    for k in ("y", "dx", "dprev") if op == "to" else ("y", "dimg", "dother"):
        assert torch.equal(alone[k], base[k][1:2]), ("sample 1 alone", k)


# ------------------------------------------------------------------------------------------------ guarded
@pytest.mark.parametrize("case", [(1, 2, 1, 257), (1, 2, 25, 41), (1, 2, 96, 100), (1, 1, 1, 16385), (1, 1, 257, 256),
                                  (1, 1, 255, 259)], ids=CID)
def test_style_guarded(case):
    S.guarded_case(case)


@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", [((2, 3, 17, 19, 3), None), ((1, 3, 36, 44, 3), 0.25), ((300, 5, 4, 4, 3), None),
                                     ((300, 5, 4, 4, 3), 0.25), ((259, 2, 4, 4, 4), None), ((259, 2, 4, 4, 4), 0.75)],
                         ids=N.VID)
def test_rgb_guarded(variant, op):
    """with more than 256 blocks the workspace of exactly the reported size holds more partials than the merge kernel has
    threads"""
    N.guarded_variant(variant, op)


# ------------------------------------------------------------------------------------------------ flags
@pytest.mark.parametrize("op", ["to", "from"])
@pytest.mark.parametrize("variant", [((300, 5, 4, 4, 3), None), ((300, 5, 4, 4, 3), 0.25)], ids=N.VID)
def test_each_wanted_gradient_alone_beyond_256_blocks(variant, op):
    """with dbias alone to_rgb's merge starts at row C of the partials, with dw alone it launches C rows: each must give
    what the run that wants everything gives when a thread adds more than one block's partial"""
    N.wanted_alone(variant, op)
