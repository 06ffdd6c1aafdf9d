#!/usr/bin/env python3
"""Pins the HOST path of the four modules outside the Swin blocks (swinvox_amd/models/_base.py, encoder.py, decoder.py, merger.py, refiner.py,
cross_view_attention.py and the stream helpers of ops.py) as the sequence of library calls AND stream operations it issues, on CPU tensors.
The Recorder of make_swin_host_trace.py stands in for call / ptr in every module that binds them, hip.check_cuda is a no-op, and the five torch
stream names the modules use (torch.cuda.current_stream / stream / Stream / Event, Tensor.record_stream) are stand-ins that append to the same
list:  ["@wait_stream", waiter, awaited]  ["@wait_event", stream, k]  ["@record", k, stream]  ["@enter", stream]  ["@exit", stream]
["@record_stream", pointer name, stream]  - streams "s<k>" and events "e<k>" numbered by first appearance in the case.  So every launch
carries which buffer goes to which argument (see make_swin_host_trace.py for the record format) and which stream it is enqueued on,
relative to the forks and joins.  Not pinned: buffer sizes and values (nothing runs).

Only the HipModule contract is driven: mod._fwd(*inputs, save=...) and mod._bwd(tape, grads, in_needs, *douts) with a real GradStore; parts of
the model are selected through cfg and the ops.set_* switches.  One image size, B = 1 x V = 2 (B = 2 for the Refiner), torch.manual_seed(0)
before every case.  A grad_ready_hook case records ["@hook", group, stream, views] (on CPU tensors _announce calls the hook directly: its
staging-stream branch needs GPU tensors and is not pinned).  Likewise the Merger's "view" cases hand it the Decoder's strided storage-dtype
view, which a CPU tensor takes through the transposing branch of as_channels_last12, not the zero-copy one.

Writes tests/golden/module_host_trace.json: "tail" = the Decoder / Merger / Refiner cases packed as the Swin fixture is (a SHA-1 per distinct
trace, a few traces in full that together show every entry point), "encoder" = per distinct Encoder trace its SHA-1 and the bare sequence of
entry-point names and @ records, one character per record (ALPHABET[index into "entries"]).  tests/test_cpu_module_host_trace.py runs the
same cases and asserts equality.  The fixture is generated ONCE, from the code whose behaviour is to be kept, and not again after that code changed.

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_module_host_trace.py
"""
import contextlib
import importlib.util
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "module_host_trace.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("make_swin_host_trace", os.path.join(HERE, "make_swin_host_trace.py"))
swin = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(swin)
sha1 = swin.sha1

ENV = ("SV_BN_DUAL", "SV_BN_SIGNS", "SV_INPUT_PREP", "SV_BN_POOL_FUSED")
CUDA_NAMES = ("current_stream", "stream", "Stream", "Event")
ALPHABET = "".join(chr(c) for c in range(35, 127) if chr(c) != "\\")      # printable, and itself in a JSON string
T, F = True, False


def _named(kind, rows, defaults):
    out = []
    for s in rows:
        s = {k: v for k, v in s.items() if defaults[k] != v}
        out.append((kind + "".join(f" {k}={s[k]}" for k in defaults if k in s), kind, dict(defaults, **s)))
    return out


DECODER = dict(math="bf16", train=T, bias=F, save=T, draw=T, dvol=T)
MERGER = dict(math="bf16", raw="view", needs=(T, T), leaky=0.2)
REFINER = dict(fused=T, leaky=0.2, bias=F, needs=T, aw=F)
ENCODER = dict(math="bf16", multi=T, stages=(0, 1, 2, 3), cva=2, prep=T, fused=T, dual=T, signs=T, overlap=T, aw=T, needs=F, train=T, save=T,
               sto=F, hook=F, cache=F, mx=F)


def cases():
    """[(name, kind, settings)]"""
    dec = []
    for math, train, bias in itertools.product(("bf16", "f32"), (T, F), (F, T)):
        dec.append(dict(math=math, train=train, bias=bias))
    for math in ("bf16", "f32"):
        dec += [dict(math=math, save=F), dict(math=math, train=F, save=F), dict(math=math, draw=F), dict(math=math, dvol=F)]
    mer = [dict(math=m, raw=r, needs=n, leaky=lk) for m, r, n, lk in
           itertools.product(("bf16", "f32"), ("view", "f32"), ((T, T), (T, F), (F, T)), (0.2, 0.1))]
    ref = [dict(fused=f, leaky=lk, bias=b, needs=n, aw=a) for f, lk, b, n, a in itertools.product((T, F), (0.2, 0.1), (F, T), (T, F), (F, T))]
    enc = [dict(), dict(multi=F), dict(stages=(1, 3)), dict(stages=(0, 1, 2)), dict(cva=0), dict(cva=1), dict(cva=4), dict(prep=F),
           dict(fused=F), dict(dual=F), dict(signs=F), dict(overlap=F, aw=F), dict(overlap=F), dict(aw=F), dict(needs=T), dict(needs=T, prep=F),
           dict(needs=T, aw=F), dict(train=F, save=F), dict(sto=T), dict(sto=T, multi=F), dict(hook=T), dict(hook=T, multi=F), dict(hook=T, aw=F),
           dict(math="f32"), dict(cache=T), dict(mx=T), dict(mx=T, needs=T)]
    out = _named("decoder", dec, DECODER) + _named("merger", mer, MERGER) + _named("refiner", ref, REFINER) + _named("encoder", enc, ENCODER)
    assert len({n for n, _, _ in out}) == len(out)
    return out


class _Stream:
    def __init__(self, log, device=None, priority=0):
        self.log = log

    def wait_stream(self, other):
        self.log.add("@wait_stream", self.log.stream(self), self.log.stream(other))

    def wait_event(self, ev):
        self.log.add("@wait_event", self.log.stream(self), self.log.event(ev))


class _Event:
    def __init__(self, log):
        self.log = log

    def record(self, stream=None):
        self.log.add("@record", self.log.event(self), self.log.stream(stream if stream is not None else self.log.current_stream()))


class StreamLog:
    """The stand-ins of torch.cuda.current_stream / stream / Stream / Event and Tensor.record_stream: they append to rec.calls"""

    def __init__(self, rec):
        self.rec = rec
        self.reset()

    def reset(self):
        self.stack, self.streams, self.events = [_Stream(self)], {}, {}

    def add(self, *record):
        self.rec.calls.append(list(record))

    def stream(self, s):
        return self.streams.setdefault(id(s), (s, f"s{len(self.streams)}"))[1]

    def event(self, e):
        return self.events.setdefault(id(e), (e, f"e{len(self.events)}"))[1]

    def current_stream(self, device=None):
        return self.stack[-1]

    @contextlib.contextmanager
    def enter(self, s):
        self.add("@enter", self.stream(s))
        self.stack.append(s)
        try:
            yield
        finally:
            self.stack.pop()
            self.add("@exit", self.stream(s))

    def Stream(self, device=None, priority=0):
        return _Stream(self, device, priority)

    def Event(self, *a, **k):
        return _Event(self)

    def record_stream(self, tensor, s):
        self.add("@record_stream", self.rec._p(self.rec.ptr(tensor)), self.stream(s))


def _modules():
    from swinvox_amd import ops
    from swinvox_amd.models import _base, cross_view_attention, decoder, encoder, merger, refiner, swin_transformer
    return (ops, _base, encoder, decoder, merger, refiner, cross_view_attention, swin_transformer)


def snapshot():
    """everything recording() replaces, for the test's before == after"""
    from swinvox_amd import hip, ops
    ctx = ops._CTX
    return ([(m.call, m.ptr) for m in _modules()], hip.check_cuda, hip.ACT, hip.TRACE, dict(ops._STATE), [getattr(torch.cuda, n) for n in CUDA_NAMES],
            torch.Tensor.__dict__.get("record_stream"), torch.Tensor.record_stream, dict(ops._SIDE), dict(ops._COMM), dict(ops.AsyncWgrad._streams),
            (ctx.packs, ctx.arena, ctx.awg, ctx.bn_tick, ctx.dyq), dict(os.environ))


@contextlib.contextmanager
def recording():
    """swin.recording() (Recorder in place of ops / swin_transformer call and ptr, switches, storage code, environment restored) widened to the
    other model modules, hip.check_cuda, the torch stream names and the per-device stream caches -> (recorder, stream log)"""
    from swinvox_amd import hip, ops
    mods, ctx = _modules(), ops._CTX
    with swin.recording() as rec:
        log = StreamLog(rec)
        saved = ([(m.call, m.ptr) for m in mods[1:-1]], hip.check_cuda, [getattr(torch.cuda, n) for n in CUDA_NAMES],
                 dict(ops._SIDE), dict(ops._COMM), dict(ops.AsyncWgrad._streams), (ctx.arena, ctx.awg, ctx.bn_tick),
                 {k: os.environ.pop(k) for k in ENV if k in os.environ})
        own = "record_stream" in torch.Tensor.__dict__ and torch.Tensor.__dict__["record_stream"]
        try:
            for m in mods[1:-1]:
                m.call, m.ptr = rec.call, rec.ptr
            hip.check_cuda = lambda *tensors: None
            torch.cuda.current_stream, torch.cuda.stream, torch.cuda.Stream, torch.cuda.Event = log.current_stream, log.enter, log.Stream, log.Event
            torch.Tensor.record_stream = lambda t, s: log.record_stream(t, s)
            yield rec, log
        finally:
            for m, (c, p) in zip(mods[1:-1], saved[0]):
                m.call, m.ptr = c, p
            hip.check_cuda = saved[1]
            for n, v in zip(CUDA_NAMES, saved[2]):
                setattr(torch.cuda, n, v)
            if own:
                torch.Tensor.record_stream = own
            else:
                del torch.Tensor.record_stream
            for cache, was in zip((ops._SIDE, ops._COMM, ops.AsyncWgrad._streams), saved[3:6]):
                cache.clear()
                cache.update(was)
            ctx.arena, ctx.awg, ctx.bn_tick = saved[6]
            os.environ.update(saved[7])


_BUILT = [None, None]     # (key, module): the cases of one cfg follow each other


def _module(kind, **net):
    import swinvox_amd as S
    from swinvox_amd import models
    key = (kind, tuple(sorted((k, str(v)) for k, v in net.items())))
    if _BUILT[0] != key:
        cfg = S.default_cfg()
        cfg.NETWORK.update(net)
        torch.manual_seed(0)
        _BUILT[:] = [key, getattr(models, kind.capitalize())(cfg)]
    return _BUILT[1]


def _grads(mod):
    from swinvox_amd.models._base import GradStore
    return GradStore(mod._param_list(), mod._grad_layout())


def _math(mode):
    from swinvox_amd import ops
    ops.set_math(mode)
    ops.set_storage(mode)


@contextlib.contextmanager
def _wgrad_stream(on):
    """the weight-gradient stream of a module backward, as _ModuleFn.backward sets it up and joins it"""
    from swinvox_amd import ops
    aw = ops.AsyncWgrad(torch.device("cpu")) if on else None
    ops.set_async_wgrad(aw)
    try:
        yield
    finally:
        ops.set_async_wgrad(None)
        if aw is not None:
            aw.join()


def _decoder(s, log):
    _math(s["math"])
    mod = _module("decoder", TCONV_USE_BIAS=s["bias"]).train(s["train"])
    (raw, vol), tape = mod._fwd(torch.empty(1, 2, 256, 7, 7), save=s["save"])
    if s["save"]:
        draw = torch.empty(raw.shape, dtype=raw.dtype) if s["draw"] else None
        mod._bwd(tape, _grads(mod), [True], draw, torch.empty(vol.shape) if s["dvol"] else None)


def _merger(s, log):
    from swinvox_amd import ops
    _math(s["math"])
    mod = _module("merger", LEAKY_VALUE=s["leaky"]).train()
    if s["raw"] == "view":      # what Decoder returns: a [B,V,9,32,32,32] view of channels-last storage [B,V,32,32,32,12] in the storage dtype
        raw = ops.empty(1, 2, 32, 32, 32, 12, device="cpu")[..., :9].permute(0, 1, 5, 2, 3, 4)
    else:
        raw = torch.empty(1, 2, 9, 32, 32, 32)
    out, tape = mod._fwd(raw, torch.empty(1, 2, 32, 32, 32), save=True)
    mod._bwd(tape, _grads(mod), list(s["needs"]), torch.empty(out.shape))


def _refiner(s, log):
    from swinvox_amd import ops
    _math("bf16")
    ops.set_bn_pool_fused(s["fused"])
    mod = _module("refiner", LEAKY_VALUE=s["leaky"], TCONV_USE_BIAS=s["bias"]).train()
    out, tape = mod._fwd(torch.empty(2, 32, 32, 32), save=True)
    with _wgrad_stream(s["aw"]):
        mod._bwd(tape, _grads(mod), [s["needs"]], torch.empty(out.shape))


def _encoder(s, log):
    from swinvox_amd import ops
    _math(s["math"])
    ops.set_input_prep(s["prep"])
    ops.set_bn_pool_fused(s["fused"])
    ops.set_bn_dual(s["dual"])
    ops.set_bn_signs(s["signs"])
    ops.set_overlap(s["overlap"])
    if s["mx"]:
        ops.set_linear_fp8(True, backward=True, recipe="mx", backward_recipe="mx")
        ops.set_mx_dual_quant(True)
        ops.set_fused_attn_block(False)
        ops.set_fused_mlp(False)
    mod = _module("encoder", USE_SWIN_T_MULTI_STAGE=s["multi"], SWIN_T_STAGES=list(s["stages"]), USE_CROSS_VIEW_ATTENTION=s["cva"] > 0,
                  ATT_SPATIAL_DOWNSAMPLE_RATIO=s["cva"] or 2).train(s["train"])
    mod.stochastic = s["sto"]
    mod.grad_ready_hook = (lambda k, views: log.add("@hook", k, log.stream(log.current_stream()), len(views))) if s["hook"] else None
    images = torch.empty(1, 2, 3, 224, 224)
    try:
        if s["cache"]:      # two forwards as _ModuleFn.forward sets them up: the first registers the packs, the second makes them in one launch
            packs, arena = ops.PackCache(), ops.ZeroArena()
            for _ in range(2):
                ops.set_pack_cache(packs)
                ops.set_arena(arena)
                try:
                    packs.refresh()
                    arena.begin(images.device)
                    out, tape = mod._fwd(images, save=s["save"])
                finally:
                    ops.bn_tick_flush()
                    arena.end()
                    ops.set_pack_cache(None)
                    ops.set_arena(None)
            ops.set_pack_cache(packs)
        else:
            out, tape = mod._fwd(images, save=s["save"])
        if s["save"]:
            with _wgrad_stream(s["aw"]):
                mod._bwd(tape, _grads(mod), [s["needs"]], torch.empty(out.shape))
    finally:
        mod.stochastic, mod.grad_ready_hook = True, None
        ops.set_pack_cache(None)


def trace_all(kinds=("decoder", "merger", "refiner", "encoder")):
    """{case name: trace} of every case of cases() of the given kinds"""
    from swinvox_amd import ops
    run = dict(decoder=_decoder, merger=_merger, refiner=_refiner, encoder=_encoder)
    out = {}
    with recording() as (rec, log):
        state = dict(ops._STATE)
        for name, kind, s in cases():
            if kind not in kinds:
                continue
            ops._STATE.clear()
            ops._STATE.update(state)                     # every case starts from the switches recording() found
            for cache in (ops._SIDE, ops._COMM, ops.AsyncWgrad._streams):
                cache.clear()
            rec.reset()
            log.reset()
            torch.manual_seed(0)
            run[kind](s, log)
            ops.bn_tick_flush()
            out[name] = json.loads(json.dumps(rec.calls))
            rec.reset()
    _BUILT[:] = [None, None]
    return out


def split(traces):
    """{case: trace} -> ({tail-module case: trace}, {Encoder case: trace})"""
    return ({n: t for n, t in traces.items() if not n.startswith("encoder")}, {n: t for n, t in traces.items() if n.startswith("encoder")})


def pack(traces):
    """-> the fixture: "tail" = swin.pack of the Decoder / Merger / Refiner cases; "encoder" = names / cases / sha1 the same way and, per distinct
    trace, "sequences": the record heads (entry point or @ name, no arguments), ALPHABET[index into "entries"] per record."""
    tail, enc = split(traces)
    fx = swin.pack(enc)
    distinct = {k: t for t, k in zip(enc.values(), fx["cases"])}
    entries = sorted({c[0] for t in enc.values() for c in t})
    assert len(entries) <= len(ALPHABET)
    at = {e: ALPHABET[i] for i, e in enumerate(entries)}
    seqs = ["".join(at[c[0]] for c in distinct[k]) for k in range(len(fx["sha1"]))]
    return {"tail": swin.pack(tail), "encoder": {"names": fx["names"], "cases": fx["cases"], "sha1": fx["sha1"], "entries": entries, "sequences": seqs}}


def main():
    sys.dont_write_bytecode = True
    from swinvox_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        sys.exit(f"{hip.LIB_PATH} is missing: build the library first (its *_supported queries decide the paths)")
    traces = trace_all()
    again = trace_all()
    assert json.dumps(traces) == json.dumps(again), "two runs differ"
    fx = pack(traces)
    t, e = fx["tail"], fx["encoder"]
    with open(FIXTURE, "w") as f:                           # one call per line: a changed call shows as one changed line
        f.write('{"tail": {"names": "%s",\n"cases": %s,\n"sha1": [\n%s\n],\n"traces": {\n' % (
            t["names"], json.dumps(t["cases"]), ",\n".join(json.dumps(h) for h in t["sha1"])))
        f.write(",\n".join('"%s": [\n' % i + ",\n".join(" " + json.dumps(c) for c in tr) + "\n]" for i, tr in t["traces"].items()) + "\n}},\n")
        f.write('"encoder": {"names": "%s",\n"cases": %s,\n"sha1": [\n%s\n],\n"entries": %s,\n"sequences": [\n%s\n]}}\n' % (
            e["names"], json.dumps(e["cases"]), ",\n".join(json.dumps(h) for h in e["sha1"]), json.dumps(e["entries"]),
            ",\n".join(json.dumps(s) for s in e["sequences"])))
    tail, enc = split(traces)
    entries = sorted({c[0] for tr in traces.values() for c in tr})
    print(f"{len(tail)} tail cases, {len(t['sha1'])} distinct ({len(t['traces'])} in full), at most {max(map(len, tail.values()))} records; "
          f"{len(enc)} Encoder cases, {len(e['sha1'])} distinct, at most {max(map(len, enc.values()))} records "
          f"({max(sum(c[0][0] == '@' for c in tr) for tr in enc.values())} stream records); {len(entries)} record heads; {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
