"""Host-only checks of the dispatch of both modes (library predicates only: no GPU needed).

tests/conv_routes.py drives the public launch functions of sivae_hip.ops on meta tensors with the C-ABI call replaced by
a recorder.  tests/golden/conv_routes_fp32.json.gz is what it recorded (`python tests/conv_routes.py`) on the commit that
folded the per-variant fp32 BatchNorm entry points into the general ones; that recording is the one made BEFORE the
dispatch was split into route functions and launch bodies with its BatchNorm call records renamed to the general entries
and nothing else ("One BatchNorm entry point per pass", has the translation table and the comparison).  A
kernel pull request that changes a route regenerates it from the commit that introduces the route.

(a) the replay on this tree equals the fixture, record for record;
(b) for every case, the route function names what the launch then does: entry point, timer key, executed FLOPs,
    statistics rows, the materialised input, the refusal;
(c) pinned statements about the headline network (celeb256, channels 64-128-256-512-512-512).

The bf16 mode (sivae_hip.ops16) has the same two checks on tests/golden/conv_routes_bf16.json.gz
(`python tests/conv_routes.py --bf16`), recorded on the last commit whose ops16 launch functions still chose the entry
point inline ("pointcloud.hip: one definition per shared ReLU-BatchNorm/max expression"); its switch variants include
synchronised BatchNorm and two ranks on one device.  In (b) the workspace size is compared too, and the pooled data
gradient's route — which conv2d_pool never consults to refuse — must be refused exactly where the switch is off, the
map is odd or conv2d launches the split-K entry for the same layer.
"""
import pytest

import conv_routes as cr

_PRELUDE = ("sivae_pack_", "sivae_upsample2_fwd", "sivae_avgpool2_bwd")


def _route(ops, kind, p):
    """the *_route call that belongs to a generator case (None: the case has no route function)"""
    if kind == "fwd":
        return ops.conv2d_fwd_route(**p)
    if kind == "wgrad":
        return ops.conv2d_wgrad_route(**{k: v for k, v in p.items() if k != "has_out"})
    if kind == "up_dgrad":
        return ops.conv2d_up_dgrad_route(**{k: v for k, v in p.items() if k not in ("has_out", "accumulate")})
    if kind in ("bn_bwd", "bn_signmask", "bn_dzsum"):
        return ops.bn_bwd_route(p["B"], p["C"], p["H"], p["W"], op=kind[3:] if kind != "bn_bwd" else kind,
                                four_d=not p.get("flat", False), dy_pooled=p.get("dy_pooled", False),
                                nseg=p.get("nseg", 1))
    if kind.endswith("16"):
        from sivae_hip import ops16
        fn = dict(conv16=ops16.conv2d_route, pool16=ops16.conv2d_pool_route, wgrad16=ops16.conv2d_wgrad_route)
        if kind == "bn_bwd16":
            return ops16.bn_bwd_route(p["B"], p["C"], p["H"], p["W"], nseg=p["nseg"])
        # (an upsampled input of an odd map: the output map is twice the input's, one less than the case names)
        H, W = (p["H"] // 2 * 2, p["W"] // 2 * 2) if p.get("upsample") else (p["H"], p["W"])
        return fn[kind](p["B"], p["Ci"], p["Co"], H, W, *([p["ks"]] if "ks" in p else []), **{
            k: v for k, v in p.items() if k in ("bias", "out_f32", "want_stats") and kind == "conv16"})
    return None


def _route_vs_record(r, p, rec):
    """-> None, or what the route says differently from what the launch recorded"""
    if rec[-1][0] == "raise":
        got = None if r.error is None else (r.error[0].__name__, r.error[1])
        return None if got == tuple(rec[-1][1:]) else "refusal %r, route says %r" % (rec[-1][1:], got)
    if r.error is not None:
        return "route refuses (%s) what the launch ran" % (r.error,)
    calls = [ev[1] for ev in rec if ev[0] == "call"]
    main = [c for c in calls if not c.startswith(_PRELUDE)]
    if not main or main[0] != r.entry:
        return "launched %s, route says %s" % (main, r.entry)
    expanded = any(c in ("sivae_upsample2_fwd", "sivae_avgpool2_bwd") for c in calls)
    if expanded != bool(r.materialise):
        return "materialised input: launch %s, route %s" % (expanded, r.materialise)
    timer = [ev for ev in rec if ev[0] == "timer"]
    if r.key is not None or timer:
        flops = timer[0][2] if timer else None
        want = ["timer", r.key, flops, flops if r.ratio is None else flops * r.ratio[0] / r.ratio[1]]
        if timer != [want]:
            return "timer %s, route says %s" % (timer, want)
    if p.get("want_stats") and rec[-1][1][1][0] != r.stats_rows:
        return "statistics rows %s, route says %d" % (rec[-1][1][1], r.stats_rows)
    return None


def _route16_vs_record(ops, events, r, kind, p, rec):
    """_route_vs_record for a bf16 case, plus the workspace size and the planner's refusal of the pooled data gradient"""
    if kind == "pool16":
        twin = cr.record_case(ops, events, "conv16", dict(B=p["B"], Ci=p["Ci"], Co=p["Co"], H=p["H"], W=p["W"], ks=3))
        from sivae_hip import ops16
        refused = not ops16.POOL_DGRAD or p["H"] % 2 or p["W"] % 2 or twin[0][1] == "sivae_bf16_conv2d_fwd_splitk"
        if (r.error is not None) != bool(refused):
            return "pooled data gradient refused: route %s, expected %s" % (r.error, bool(refused))
        r = r._replace(error=None)
    msg = _route_vs_record(r, p, rec)
    launch = [ev for ev in rec if ev[0] == "call"][0]
    if msg is None and r.ws_bytes and launch[-2] != r.ws_bytes:  # (entries with a workspace end: ..., its size, stream)
        msg = "workspace of %d bytes, route says %d" % (launch[-2], r.ws_bytes)
    return msg


@pytest.fixture(scope="module")
def replay16():
    """one run of the bf16 generator on this tree: ({variant: [(case name, record)]}, route disagreements)"""
    wrong = []

    def on_case(ops, variant, name, kind, p, rec):
        events = ops.TIMER.events
        msg = _route16_vs_record(ops, events, _route(ops, kind, p), kind, p, rec)
        if msg is not None:
            wrong.append("[%s] %s: %s" % (variant, name, msg))

    return cr.generate(on_case, bf16=True), wrong


@pytest.fixture(scope="module")
def replay():
    """one run of the generator on this tree: ({variant: [(case name, record)]}, route disagreements, the cases of the
    celeb256 walks as (name, kind, params, record))"""
    wrong, headline = [], []

    def on_case(ops, variant, name, kind, p, rec):
        r = _route(ops, kind, p)
        if r is not None:
            msg = _route_vs_record(r, p, rec)
            if msg is not None:
                wrong.append("[%s] %s: %s" % (variant, name, msg))
        if variant == "default" and name.startswith("celeb256_bs"):
            headline.append((name, kind, p, rec))

    return cr.generate(on_case), wrong, headline


def _same_as_fixture(got, want, floor):
    assert list(got) == list(want), "switch variants differ: %s vs %s" % (list(got), list(want))
    n = 0
    for variant, rows in want.items():
        new = got[variant]
        assert [name for name, _ in new] == [name for name, _ in rows], "case table of variant %s differs" % variant
        for (name, a), (_, b) in zip(rows, new):
            assert a == b, "[%s] %s\n  recorded: %s\n  now:      %s" % (variant, name, a, b)
            n += 1
    assert n >= floor, n  # (sanity: the table and the network walks were there)


def test_replay_equals_the_recording_of_the_previous_dispatch(replay):
    _same_as_fixture(replay[0], cr.expand(cr.load_fixture()), 100000)


def test_bf16_replay_equals_the_recording_of_the_previous_dispatch(replay16):
    _same_as_fixture(replay16[0], cr.expand(cr.load_fixture(cr.FIXTURE16)), 30398)  # (the recorded count)


def test_the_bf16_route_is_what_is_launched(replay16):
    wrong = replay16[1]
    assert not wrong, "%d cases; first: %s" % (len(wrong), wrong[0])


def test_the_route_is_what_is_launched(replay):
    wrong = replay[1]
    assert not wrong, "%d cases; first: %s" % (len(wrong), wrong[0])


def _keys(headline, net, kind):
    """[(output map, upsampled input, fused prologue, timer key)] of the 3x3 layers of one unpaired celeb256 walk"""
    out = []
    for name, k, p, rec in headline:
        if name.startswith(net + " nseg=1 ") and k == kind and p["ks"] == 3:
            key = [ev[1] for ev in rec if ev[0] == "timer"]
            assert len(key) == 1, (name, rec)
            out.append((p["H"], bool(p.get("upsample")), bool(p.get("pro")), key[0]))
    return out


@pytest.mark.parametrize("net", ["celeb256_bs128", "celeb256_bs16"])
def test_headline_network_routes(replay, net):
    """celeb256 at 128 images and as a 16-image shard (what tests/test_e2e_gpu.py states through timer keys on a GPU):
    every 3x3 conv that reads a stored input, from 256x256 down to 16x16, runs conv_wino4_kernel<false|true> (plain |
    fused prologue) and its weight gradient wino4_wgrad_kernel<.,false>; at 128 images the 512-channel 8x8 / 4x4 layers
    run conv_wino4_grid_kernel<.> and wino4_wgrad_kernel<.,true>; at 16 images the 8x8 / 4x4 forward stays on
    conv_wino_kernel<2,2,.> / conv_wino_kernel<1,1,.> while their weight gradient is wino4_wgrad_kernel<.,true>.
    A conv of an upsampled input takes the same kernels on the 16x16 / 8x8 maps (the input is materialised) and the
    phase-form kernels conv_wino_up_kernel / wino_up_wgrad_kernel from 32x32 up."""
    headline = replay[2]
    tf = {True: "true", False: "false"}
    fwd, wg = _keys(headline, net, "fwd"), _keys(headline, net, "wgrad")
    assert {m for m, _, _, _ in fwd} == {4, 8, 16, 32, 64, 128, 256} == {m for m, _, _, _ in wg}
    for m, up, pro, key in fwd:
        if up and m >= 32:
            want = "conv_wino_up_kernel<%s,%s>" % ("1,4" if m >= 64 else "2,3", tf[pro])
        elif m >= 16:
            want = "conv_wino4_kernel<%s>" % tf[pro]
        elif net == "celeb256_bs128":
            want = "conv_wino4_grid_kernel<%s>" % tf[pro]
        else:
            want = "conv_wino_kernel<%s,%s>" % ("2,2" if m == 8 else "1,1", tf[pro])
        assert key == want, (net, "fwd", m, up, pro, key, want)
    for m, up, pro, key in wg:
        want = "wino_up_wgrad_kernel" if (up and m >= 32) else "wino4_wgrad_kernel<%s,%s>" % (tf[pro], tf[m <= 8])
        assert key == want, (net, "wgrad", m, up, pro, key, want)
