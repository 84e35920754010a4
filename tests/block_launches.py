"""Characterisation of the autograd Functions of sivae_hip.functional / functional16, recorded without a GPU.

tests/conv_routes.py records what the launch functions of `ops` do; this module drives the REAL Functions (ResBlockFn,
StemFn, ConvBiasFn, their bf16 twins, LinearFn and the loss Functions) on device="meta" tensors under that recorder and
records, per Function call:

  fwd / bwd   every C entry point with its scalar arguments and pointer pattern and every timer event, in order; in
              the backward also ["grad", parameter] where `_sivae_on_grad` fired (dp.GradSync depends on that order)
  out         shape and dtype of the output
  saved       shape, dtype and storage group of every tensor saved for the backward (the activation footprint)
  use         the slab index each parameter use claimed
  grads       the None / (shape, dtype) pattern of the backward's return tuple
  raise       the exception type and message where the call is refused

The recorder additions live here, not in the package (what `ops16` needs is in conv_routes.recording, which the bf16
dispatch recording shares): `ops._ld` asks for a device tensor; the sign-mask backwards check `mask.is_cuda` (they are
handed a stand-in); and a meta tensor's data_ptr() is 0, so while recording meta tensors answer with a storage identity
instead (the replay caches and the pack caches compare data_ptr()).

    python tests/block_launches.py            # writes tests/golden/block_launches.json.gz
    python tests/block_launches.py --trace    # also lists the lines of the block Functions that never ran

The committed fixture was recorded on the commit that folded the per-variant fp32 BatchNorm entry points into the general
ones (every fp32 BatchNorm apply / replay call is a _seg entry with seg_images = B // nseg).
tests/test_block_launches_host.py replays it in-process and compares with the committed fixture.
"""
import contextlib
import gzip
import json
import os
import sys

import torch

import conv_routes as CR
from conv_routes import M

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_launches.json.gz")

# the switches of the glue, set explicitly like conv_routes.SWITCHES (module name -> {switch: value})
GLUE = dict(functional=dict(MATERIALIZE_H=False, DIRECT_GRADS=True), nn=dict(DEFER_UPSAMPLE=True),
            functional16=dict(MATERIALIZE_H=True, SIGNMASK=True, KWPACK=True), ops16=dict(POOL_DGRAD=True))


def _desc(t):
    return [list(t.shape), str(t.dtype)[6:]]


def _meta_ptr(t):
    return t.untyped_storage()._cdata + t.storage_offset() * t.element_size()


def _functions(*modules):
    out = []
    for m in modules:
        for v in vars(m).values():
            if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == m.__name__:
                out.append(v)
    return out


class Session:
    """what one `recording` collects: `nodes` (one record per Function call, in forward order)"""

    def __init__(self, ops, events):
        self.ops, self.events = ops, events
        self.nodes, self.by_ctx, self.keep = [], {}, []

    def reset(self):
        del self.events[:]
        self.nodes, self.by_ctx, self.keep = [], {}, []

    def run(self, fn, thunk):
        """one forward of Function `fn`"""
        n0 = len(self.events)
        node = {"fn": fn.__name__}
        self.nodes.append(node)
        try:
            y = thunk()
        except Exception as e:  # noqa: BLE001  (a refusal is part of the behaviour recorded)
            node["fwd"] = [ev for ev in self.events[n0:] if not (ev[0] == "call" and ev[1].startswith("sivae_pack_"))]
            node["raise"] = [type(e).__name__, str(e)]
            raise
        node["fwd"] = self.events[n0:]
        node["out"] = _desc(y)
        ctx = y.grad_fn
        if ctx is not None and type(ctx).__name__ == fn.__name__ + "Backward":
            if hasattr(ctx, "use"):
                node["use"] = list(ctx.use)
            groups = {}
            node["saved"] = [None if t is None else _desc(t) + [groups.setdefault(t.untyped_storage()._cdata, len(groups))]
                             for t in ctx.saved_tensors]
            self.by_ctx[id(ctx)] = node
            self.keep.append(ctx)
        return y

    def backward_of(self, fn):
        orig = fn.__dict__["backward"].__func__
        sess = self

        def backward(ctx, *grads):
            node = sess.by_ctx.get(id(ctx))
            if node is None:
                return orig(ctx, *grads)
            n0 = len(sess.events)
            try:
                ret = orig(ctx, *grads)
            except Exception as e:  # noqa: BLE001
                node["bwd"] = sess.events[n0:]
                node["bwd_raise"] = [type(e).__name__, str(e)]
                raise
            node["bwd"] = sess.events[n0:]
            node["grads"] = [None if r is None else _desc(r) for r in (ret if isinstance(ret, tuple) else (ret,))]
            return ret
        return staticmethod(backward)


@contextlib.contextmanager
def recording(switches=None, glue=None):
    """conv_routes.recording plus what the Functions need (module docstring); yields a Session.
    glue: {module name: {switch: value}} overrides of GLUE"""
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    from sivae_hip import nn as N
    from sivae_hip import ops16
    mods = dict(functional=SF, functional16=SF16, nn=N, ops16=ops16)
    with CR.recording(switches) as (ops, events):
        sess = Session(ops, events)
        undo = []

        def patch(obj, name, value):
            undo.append((obj, name, obj.__dict__.get(name, undo) if isinstance(obj, type) else getattr(obj, name)))
            setattr(obj, name, value)

        try:
            for mname, sw in GLUE.items():
                for k, v in dict(sw, **(glue or {}).get(mname, {})).items():
                    patch(mods[mname], k, v)
            patch(ops, "_ld", lambda t: t.stride(0))
            signmask, bn_bwd16, ptr, apply_ = ops.bn_bwd_signmask, ops16.bn_bwd, torch.Tensor.data_ptr, SF._apply
            patch(ops, "bn_bwd_signmask", lambda dy, mask, *a, **k: signmask(dy, CR._MaskOf(mask), *a, **k))
            patch(ops16, "bn_bwd", lambda dy, y, *a, **k: bn_bwd16(
                dy, CR._MaskOf(y) if (y is not None and y.dtype == torch.uint8) else y, *a, **k))
            patch(torch.Tensor, "data_ptr", lambda t: _meta_ptr(t) if t.device.type == "meta" else ptr(t))
            patch(SF, "_apply", lambda fn, *args: sess.run(fn, lambda: apply_(fn, *args)))
            for fn in _functions(SF, SF16):
                patch(fn, "backward", sess.backward_of(fn))
            yield sess
        finally:
            for obj, name, value in reversed(undo):
                if value is undo:  # (the name was inherited: torch.Tensor.data_ptr)
                    delattr(obj, name)
                else:
                    setattr(obj, name, value)


# ---- drivers ---------------------------------------------------------------------------------------------------------
def _nets(channels, size, cdim=3):
    from sivae_hip import nn as N
    with torch.device("meta"), contextlib.redirect_stdout(None):  # (the constructors print their shapes)
        enc = N.Encoder(cdim, 8, channels, size)
        dec = N.Decoder(cdim, 8, channels, size, conv_input_size=enc.conv_output_size)
    return enc.train(), dec.train()


def _prepare(sess, module, slabs=True, frozen=False, nslabs=3):
    """fake gradient slabs and recording callbacks on every parameter"""
    for name, p in module.named_parameters():
        p.requires_grad_(not frozen)
        p.grad = None
        p.__dict__.pop("_sivae_use", None)
        p.__dict__.pop("_sivae_slabs", None)
        if slabs:
            p.__dict__["_sivae_slabs"] = [M(*p.shape) for _ in range(nslabs)]
        p.__dict__["_sivae_on_grad"] = lambda p_, name=name: sess.events.append(["grad", name])


def _input(which, enc, B, bf16, x_grad=True):
    from sivae_hip import ops16
    if which == "enc":
        x = M(B, enc.cdim, enc.image_size, enc.image_size)
    else:
        C, H, W = enc.conv_output_size
        x = M(B, ops16.cblocks(C), H, W, 8, dtype=torch.bfloat16) if bf16 else M(B, C, H, W)
    return x.requires_grad_(x_grad)


def _main(net, x, bf16, nseg=1, cache=None, replay_update=True, backward=True):
    from sivae_hip import nn as N
    y = N._run_main(net.main, x, cache, bf16=True if bf16 else None, nseg=nseg, replay_update=replay_update)
    if backward:
        y.backward(torch.empty_like(y))
    return y


def walk(sess, channels, size, B, which, nseg=1, bf16=False, slabs=True, frozen=False, x_grad=True, train=True,
         cdim=3):
    enc, dec = _nets(channels, size, cdim)
    net = enc if which == "enc" else dec
    net.train(train)
    _prepare(sess, net, slabs, frozen)
    _main(net, _input(which, enc, B * nseg, bf16, x_grad), bf16, nseg)


def cached_decoder(sess, channels, size, B, bf16=False):
    """fill, then replay (both with a backward)"""
    enc, dec = _nets(channels, size)
    _prepare(sess, dec)
    x, cache = _input("dec", enc, B, bf16), {}
    _main(dec, x, bf16, cache=cache)
    _main(dec, x, bf16, cache=cache)


def segment_view(sess, channels, size, B, bf16=False, stale=False):
    """a pair filled as one segmented batch without a graph, then pass 0 replayed from its `cache_segment` view with
    replay_update=False; stale: the weights changed since the fill — the view cannot be replayed and is refused"""
    from sivae_hip import functional as SF
    enc, dec = _nets(channels, size)
    _prepare(sess, dec)
    x, cache = _input("dec", enc, 2 * B, bf16, x_grad=False), {}
    with torch.no_grad():
        _main(dec, x, bf16, nseg=2, cache=cache, backward=False)
    if stale:
        SF.bump_generation(dec.parameters())
    view = SF.cache_segment(cache, 0, 2)
    _main(dec, x[:B].detach().requires_grad_(True), bf16, cache=view, replay_update=False)


def _st(C, training=True):
    from sivae_hip import functional as SF
    with torch.device("meta"):
        return SF.BNState(torch.nn.BatchNorm2d(C).train(training))


def _leaf(sess, name, *shape):
    p = M(*shape).requires_grad_(True)
    p.__dict__["_sivae_on_grad"] = lambda p_: sess.events.append(["grad", name])
    return p


def one_block(sess, B, Ci, Co, H, W, x_up=False, post=None, nseg=1, bf16=False, training=True):
    """one ResidualBlock call at a shape the networks do not have (odd maps: the forms without a fused kernel)"""
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    from sivae_hip import ops16
    Hs, Ws = (H // 2, W // 2) if x_up else (H, W)
    x = (M(B, ops16.cblocks(Ci), Hs, Ws, 8, dtype=torch.bfloat16) if bf16 else M(B, Ci, Hs, Ws)).requires_grad_(True)
    w_exp = _leaf(sess, "w_exp", Co, Ci, 1, 1) if Ci != Co else None
    args = (x, w_exp, _leaf(sess, "w1", Co, Ci, 3, 3), _leaf(sess, "g1", Co), _leaf(sess, "b1", Co),
            _leaf(sess, "w2", Co, Co, 3, 3), _leaf(sess, "g2", Co), _leaf(sess, "b2", Co), _st(Co, training),
            _st(Co, training))
    y = (SF16 if bf16 else SF).residual_block(*args, post=post, x_up=x_up, nseg=nseg)
    y.backward(torch.empty_like(y))


def one_stem(sess, B, Ci, Co, H, W, nseg=1, bf16=False, training=True):
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    y = (SF16 if bf16 else SF).stem(M(B, Ci, H, W).requires_grad_(True), _leaf(sess, "w", Co, Ci, 5, 5),
                                     _leaf(sess, "g", Co), _leaf(sess, "b", Co), _st(Co, training), nseg)
    y.backward(torch.empty_like(y))


def one_predict(sess, B, Ci, Co, H, W, ks=5, bias=True, bf16=False, cached=False):
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    from sivae_hip import ops16
    x = (M(B, ops16.cblocks(Ci), H, W, 8, dtype=torch.bfloat16) if bf16 else M(B, Ci, H, W)).requires_grad_(True)
    w, b = _leaf(sess, "w", Co, Ci, ks, ks), (_leaf(sess, "bias", Co) if bias else None)
    cache = {} if cached else None
    for _ in range(2 if cached else 1):
        y = (SF16 if bf16 else SF).conv_bias(x, w, b, cache)
        y.backward(torch.empty_like(y))


def loss_functions(sess):
    from sivae_hip import functional as SF

    def go(fn, thunk):
        y = sess.run(fn, thunk)
        y.backward(torch.empty_like(y))

    def leaf(*shape):
        return M(*shape).requires_grad_(True)

    for B, K, N_, relu in ((16, 8192, 1024, False), (16, 512, 8192, True), (3, 10, 7, False), (3, 10, 7, True)):
        x, w, b = leaf(B, K), _leaf(sess, "w", N_, K), _leaf(sess, "bias", N_)
        y = SF.linear(x, w, b, relu)
        y.backward(torch.empty_like(y))
    mu, lv, eps = leaf(16, 512), leaf(16, 512), M(16, 512)
    go(SF.ReparamFn, lambda: SF.reparameterize(mu, lv, eps))
    for reduce in ("none", "sum", "mean"):
        go(SF.KLFn, lambda: SF.kl(lv, mu, reduce=reduce))
        go(SF.KLFn, lambda: SF.kl(lv, mu, M(16, 512), 0.5, reduce=reduce))
    x, r = leaf(16, 3, 32, 32), leaf(16, 3, 32, 32)
    for mode in ("rows", "total", "elem"):
        go(SF.ReconFn, lambda: SF.ReconFn.apply(x, r, "mse", mode, 0.5))
    L, KL = leaf(16), leaf(16)
    go(SF.ExpElboFn, lambda: SF.expelbo(L, KL, 0.5, 1.0, 256.0))
    # (SF.lincomb itself asks for device scalars; the Function behind it does not)
    go(SF.LinCombFn, lambda: SF.LinCombFn.apply((0.5, 1.0, 2.0), leaf(), M(), leaf()))


# ---- case table ------------------------------------------------------------------------------------------------------
def _bf16_nets():
    import block_checks16 as BC
    return BC.PRODUCTION


def cases():
    """[(case name, switches of ops, glue switches, thunk(sess))]"""
    out = []

    def add(name, thunk, switches=None, glue=None):
        out.append((name, switches or {}, glue or {}, thunk))

    for net, ch, size, B in CR.NETWORKS:
        for nseg in (1, 2):
            for which in ("enc", "dec"):
                add("fp32 %s nseg=%d %s" % (net, nseg, which),
                    lambda s, ch=ch, size=size, B=B, which=which, nseg=nseg: walk(s, ch, size, B, which, nseg))
    for net, ch, size, B in _bf16_nets():
        for nseg in (1, 2):
            for which in ("enc", "dec"):
                add("bf16 %s nseg=%d %s" % (net, nseg, which),
                    lambda s, ch=ch, size=size, B=B, which=which, nseg=nseg: walk(s, ch, size, B, which, nseg, bf16=True))
    nets = {n[0]: n[1:] for n in CR.NETWORKS}
    for net in ("celeb256_bs16", "cifar10_bs256"):
        ch, size, B = nets[net]
        for which in ("enc", "dec"):
            for vname, kw in (("frozen", dict(frozen=True)), ("no slabs", dict(slabs=False)),
                              ("no input grad", dict(x_grad=False)), ("eval", dict(train=False))):
                add("fp32 %s %s: %s" % (net, which, vname),
                    lambda s, ch=ch, size=size, B=B, which=which, kw=kw: walk(s, ch, size, B, which, **kw))
            for vname, sw, gl in (("SF.MATERIALIZE_H=1", {}, dict(functional=dict(MATERIALIZE_H=True))),
                                  ("ops.SIGNMASK=0", dict(SIGNMASK=False), {}),
                                  ("ops.WINO_UP=0", dict(WINO_UP=False), {}),
                                  ("ops.FUSE_BN_BWD=1", dict(FUSE_BN_BWD=True), {}),
                                  ("ops.SIGNMASK=0 ops.WINO_UP=0", dict(SIGNMASK=False, WINO_UP=False), {}),
                                  ("nn.DEFER_UPSAMPLE=0", {}, dict(nn=dict(DEFER_UPSAMPLE=False))),
                                  ("SF.DIRECT_GRADS=0", {}, dict(functional=dict(DIRECT_GRADS=False)))):
                for nseg in (1, 2):
                    add("fp32 %s nseg=%d %s: %s" % (net, nseg, which, vname),
                        lambda s, ch=ch, size=size, B=B, which=which, nseg=nseg: walk(s, ch, size, B, which, nseg),
                        sw, gl)
        add("fp32 %s dec: cache fill + replay" % net, lambda s, ch=ch, size=size, B=B: cached_decoder(s, ch, size, B))
        add("fp32 %s dec: cache_segment view" % net, lambda s, ch=ch, size=size, B=B: segment_view(s, ch, size, B))
        add("fp32 %s dec: stale cache_segment view" % net,
            lambda s, ch=ch, size=size, B=B: segment_view(s, ch, size, B, stale=True))
    nets16 = {n[0]: n[1:] for n in _bf16_nets()}
    for net in ("celeb256_bf16_bs16_shard", "celeb128_bf16_bs128"):
        ch, size, B = nets16[net]
        for which in ("enc", "dec"):
            for vname, sw, gl, segs in (("SF16.MATERIALIZE_H=0", {}, dict(functional16=dict(MATERIALIZE_H=False)), (1, 2)),
                                        ("SF16.SIGNMASK=0", {}, dict(functional16=dict(SIGNMASK=False)), (1, 2)),
                                        ("ops16.POOL_DGRAD=0", {}, dict(ops16=dict(POOL_DGRAD=False)), (1, 2)),
                                        ("SF16.KWPACK=0", {}, dict(functional16=dict(KWPACK=False)), (1, 2)),
                                        ("ops.BN_FUSED=0", dict(BN_FUSED=False), {}, (1, 2))):
                for nseg in segs:
                    add("bf16 %s nseg=%d %s: %s" % (net, nseg, which, vname),
                        lambda s, ch=ch, size=size, B=B, which=which, nseg=nseg: walk(s, ch, size, B, which, nseg,
                                                                                      bf16=True), sw, gl)
            for vname, kw in (("frozen", dict(frozen=True)), ("no slabs", dict(slabs=False)),
                              ("no input grad", dict(x_grad=False)), ("eval", dict(train=False))):
                add("bf16 %s %s: %s" % (net, which, vname),
                    lambda s, ch=ch, size=size, B=B, which=which, kw=kw: walk(s, ch, size, B, which, bf16=True, **kw))
        add("bf16 %s dec: cache fill + replay" % net,
            lambda s, ch=ch, size=size, B=B: cached_decoder(s, ch, size, B, bf16=True))
        add("bf16 %s dec: cache_segment view" % net,
            lambda s, ch=ch, size=size, B=B: segment_view(s, ch, size, B, bf16=True))
        add("bf16 %s dec: stale cache_segment view" % net,
            lambda s, ch=ch, size=size, B=B: segment_view(s, ch, size, B, bf16=True, stale=True))
    # single calls at shapes the networks do not have
    for bf16 in (False, True):
        t = "bf16" if bf16 else "fp32"
        for name, kw in (("6x6 pool", dict(B=4, Ci=16, Co=16, H=6, W=6, post="pool")),
                         ("6x6 x_up", dict(B=4, Ci=16, Co=16, H=6, W=6, x_up=True)),
                         ("6x6 exp x_up up", dict(B=4, Ci=32, Co=16, H=6, W=6, x_up=True, post="up")),
                         ("6x6 exp pool", dict(B=4, Ci=16, Co=32, H=6, W=6, post="pool")),
                         ("16x16 x_up pool", dict(B=4, Ci=16, Co=16, H=16, W=16, x_up=True, post="pool")),
                         ("16x16 exp x_up pool", dict(B=4, Ci=32, Co=16, H=16, W=16, x_up=True, post="pool")),
                         ("16x16 up", dict(B=4, Ci=16, Co=16, H=16, W=16, post="up"))):
            add("%s block %s" % (t, name), lambda s, kw=kw, bf16=bf16: one_block(s, bf16=bf16, **kw))
            add("%s block %s: ops.SIGNMASK=0 / SF16.SIGNMASK=0" % (t, name),
                lambda s, kw=kw, bf16=bf16: one_block(s, bf16=bf16, **kw), dict(SIGNMASK=False),
                dict(functional16=dict(SIGNMASK=False)))
        add("%s block eval" % t, lambda s, bf16=bf16: one_block(s, 4, 16, 32, 16, 16, post="pool", bf16=bf16,
                                                                training=False))
        for name, kw in (("3->64 32x32", dict(B=4, Ci=3, Co=64, H=32, W=32)),
                         ("3->64 32x32 nseg=2", dict(B=8, Ci=3, Co=64, H=32, W=32, nseg=2)),
                         ("3->64 6x6", dict(B=4, Ci=3, Co=64, H=6, W=6)),
                         ("4->64 32x32", dict(B=4, Ci=4, Co=64, H=32, W=32)),
                         ("3->64 32x32 eval", dict(B=4, Ci=3, Co=64, H=32, W=32, training=False))):
            add("%s stem %s" % (t, name), lambda s, kw=kw, bf16=bf16: one_stem(s, bf16=bf16, **kw))
        for name, kw in (("64->3 32x32", dict(B=4, Ci=64, Co=3, H=32, W=32)),
                         ("64->4 32x32", dict(B=4, Ci=64, Co=4, H=32, W=32)),
                         ("64->3 32x32 no bias", dict(B=4, Ci=64, Co=3, H=32, W=32, bias=False)),
                         ("64->64 3x3", dict(B=4, Ci=64, Co=64, H=32, W=32, ks=3)),
                         ("64->3 32x32 cached", dict(B=4, Ci=64, Co=3, H=32, W=32, cached=True))):
            add("%s predict %s" % (t, name), lambda s, kw=kw, bf16=bf16: one_predict(s, bf16=bf16, **kw))
    add("fp32 stem 3->64 32x32 nseg=3 of 4 images", lambda s: one_stem(s, 4, 3, 64, 32, 32, nseg=3))
    add("bf16 stem 3->64 32x32: SF16.KWPACK=0", lambda s: one_stem(s, 4, 3, 64, 32, 32, bf16=True), {},
        dict(functional16=dict(KWPACK=False)))
    add("loss functions", loss_functions)
    return out


# ---- recording -------------------------------------------------------------------------------------------------------
def record_case(sess, thunk):
    """-> [(row name, record)]: one row per Function call, and the case's own row (its refusal, if any)"""
    sess.reset()
    end = ["ok"]
    try:
        thunk(sess)
    except Exception as e:  # noqa: BLE001
        end = ["raise", type(e).__name__, str(e)]
    rows = [("#%02d %s" % (i, node["fn"]), node) for i, node in enumerate(sess.nodes)]
    rows.append(("end", end))
    sess.reset()
    return rows


def generate(select=None):
    """-> {case name: [(row name, record)]}"""
    out = {}
    for name, switches, glue, thunk in cases():
        if select is not None and not select(name):
            continue
        with recording(switches, glue) as sess:
            out[name] = json.loads(json.dumps(record_case(sess, thunk)))
    return out


def load_fixture(path=FIXTURE):
    with gzip.open(path, "rt", encoding="utf-8") as f:
        return json.load(f)


def write_fixture(path=FIXTURE):
    gen = generate()
    data = json.dumps(CR.compact(gen), separators=(",", ":")).encode("utf-8")
    with open(path, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0, compresslevel=9) as f:
            f.write(data)
    return len(gen), sum(len(rows) for rows in gen.values()), len(data), os.path.getsize(path)


# ---- line coverage of the block Functions ----------------------------------------------------------------------------
TRACED = ("ResBlockFn", "StemFn", "ConvBiasFn", "ResBlockFn16", "StemFn16", "PredictFn16")


def unexecuted_lines():
    """run every case under a line tracer -> [(file, line, text)] of forward / backward of the TRACED Functions"""
    import dis
    import linecache
    from sivae_hip import functional as SF
    from sivae_hip import functional16 as SF16
    codes = {}
    for m in (SF, SF16):
        for cname in TRACED:
            cls = getattr(m, cname, None)
            if cls is not None:
                for meth in ("forward", "backward"):
                    code = cls.__dict__[meth].__func__.__code__
                    codes[code] = {ln for _, ln in dis.findlinestarts(code) if ln is not None and ln != code.co_firstlineno}
    seen = {c: set() for c in codes}

    def local(frame, event, arg):
        if event == "line":
            seen[frame.f_code].add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        return local if frame.f_code in codes else None

    sys.settrace(tracer)
    try:
        generate()
    finally:
        sys.settrace(None)
    out = []
    for code, lines in codes.items():
        for ln in sorted(lines - seen[code]):
            out.append((os.path.basename(code.co_filename), ln, linecache.getline(code.co_filename, ln).strip()))
    return sorted(out)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--trace"]
    path = args[0] if args else FIXTURE
    print("wrote %s: %d cases, %d records, %d bytes of JSON, %d compressed" % ((path,) + write_fixture(path)))
    if "--trace" in sys.argv:
        for f, ln, text in unexecuted_lines():
            print("never ran: %s:%d  %s" % (f, ln, text))
