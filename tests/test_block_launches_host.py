"""Host-only characterisation of the block glue (functional.py / functional16.py): no GPU needed.

tests/block_launches.py drives the real autograd Functions on meta tensors under the recorder of tests/conv_routes.py.
tests/golden/block_launches.json.gz is what it recorded (`python tests/block_launches.py`) on the commit that folded the
per-variant fp32 BatchNorm entry points into the general ones; that recording is the one made BEFORE the blocks were split
into a plan and its execution with its BatchNorm call records renamed to the general entries and nothing else (DESIGN.md,
"One BatchNorm entry point per pass").  A pull request that adds a block form regenerates it from the commit that
introduces the form.

(a) the replay on this tree equals the fixture, record for record: launches, timer events, outputs, saved tensors, slab
    claims, gradient notifications and the backward's return pattern of every Function call;
(b) for every ResidualBlock of the benchmarked fp32 networks, the launches of the real Function are those of the
    conv_routes.block_cases records of that block — which ties tests/golden/conv_routes_fp32.json.gz to the Functions.
"""
import pytest

import block_launches as bl
import conv_routes as cr


def test_replay_equals_the_recording_of_the_previous_glue():
    want = cr.expand(bl.load_fixture())
    got = bl.generate()
    assert list(got) == list(want), "case tables differ: %s" % (sorted(set(got) ^ set(want)),)
    n = 0
    for case, rows in want.items():
        new = got[case]
        assert [name for name, _ in new] == [name for name, _ in rows], "Function calls of case %s differ" % case
        for (name, a), (_, b) in zip(rows, new):
            if isinstance(a, dict):
                for k in sorted(set(a) | set(b)):
                    assert a.get(k) == b.get(k), "[%s] %s %s\n  recorded: %s\n  now:      %s" % (
                        case, name, k, a.get(k), b.get(k))
            assert a == b, "[%s] %s\n  recorded: %s\n  now:      %s" % (case, name, a, b)
            n += 1
    assert len(want) >= 200 and n >= 1400, (len(want), n)  # (sanity: the networks and the variants were there)


# launches of a block that conv_routes.block_cases does not model: BatchNorm statistics and apply, and the elementwise
# adjoints of the Upsample / the skip add
_NOT_MODELLED = ("sivae_bn_stats_from_conv", "sivae_bn_apply_act", "sivae_upsample2_bwd", "sivae_add_inplace")


def _entries(events):
    return [ev[1] for ev in events if ev[0] == "call" and not ev[1].startswith("sivae_pack_")]


@pytest.mark.parametrize("net,channels,size,B", cr.NETWORKS, ids=[n[0] for n in cr.NETWORKS])
@pytest.mark.parametrize("nseg", [1, 2])
def test_block_cases_are_what_the_functions_launch(net, channels, size, B, nseg):
    seen = 0
    for which in ("enc", "dec"):
        with bl.recording() as sess:
            bl.walk(sess, channels, size, B, which, nseg)
            real = [_entries(node["fwd"] + node["bwd"]) for node in sess.nodes if node["fn"] == "ResBlockFn"]
        real = [[e for e in calls if not e.startswith(_NOT_MODELLED)] for calls in real]
        with cr.recording() as (ops, events):
            blocks, last = [], None
            for layer, kind, p in cr.network_cases(ops, channels, size, B * nseg, nseg):
                if not layer.startswith(which + ".block"):
                    last = None
                    continue
                if layer != last:
                    blocks.append([])
                    last = layer
                rec = cr.record_case(ops, events, kind, p)
                assert rec[-1][0] == "ret", (layer, kind, p, rec[-1])
                blocks[-1].extend(_entries(rec))
        assert len(real) == len(blocks) and real, (which, len(real), len(blocks))
        for i, (a, b) in enumerate(zip(real, blocks)):
            assert a == b, "%s %s block %d\n  function:    %s\n  block_cases: %s" % (net, which, i, a, b)
            seen += 1
    assert seen >= 7



def test_assigning_a_switch_forgets_the_memoised_plans(monkeypatch):
    """the plans are memoised with the conv routes: a switch of ops, functional, functional16, ops16 or nn assigned with
    monkeypatch.setattr (or plainly) must show in the next plan, and undoing it must too"""
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    from sivae_hip import ops, ops16
    kw = dict(x_up=True, post="up_deferred", nseg=1, has_exp=False, training=True)
    before, before16 = SF.resblock_plan(16, 64, 64, 64, 64, 64, **kw), SF16.resblock_plan16(16, 64, 64, 64, 64, 64, **kw)
    assert (before.h_saved, before.signmask, before.dgrad1, before16.dx) == (SF.MATERIALIZE_H, ops.SIGNMASK and True,
                                                                             "phase" if ops.WINO_UP else "reduce",
                                                                             "pool" if ops16.POOL_DGRAD else "conv")
    with monkeypatch.context() as m:
        m.setattr(SF, "MATERIALIZE_H", not SF.MATERIALIZE_H)
        m.setattr(ops, "SIGNMASK", not ops.SIGNMASK)
        m.setattr(ops, "WINO_UP", not ops.WINO_UP)
        m.setattr(ops16, "POOL_DGRAD", not ops16.POOL_DGRAD)
        m.setattr(SF16, "SIGNMASK", not SF16.SIGNMASK)
        now, now16 = SF.resblock_plan(16, 64, 64, 64, 64, 64, **kw), SF16.resblock_plan16(16, 64, 64, 64, 64, 64, **kw)
        assert (now.h_saved, now.signmask) == (not before.h_saved, not before.signmask)
        assert now.dgrad1 != before.dgrad1 and now16.dx != before16.dx and now16.signmask != before16.signmask
    assert SF.resblock_plan(16, 64, 64, 64, 64, 64, **kw) == before
    assert SF16.resblock_plan16(16, 64, 64, 64, 64, 64, **kw) == before16
