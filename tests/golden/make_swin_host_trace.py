#!/usr/bin/env python3
"""Pins the HOST path of the Swin blocks (swinvox_amd/ops.py swin_linear_* / quantize_* / layernorm_quant*, models/swin_transformer.py
block_forward / block_backward / stage_forward / stage_backward) as the sequence of library calls it issues, on CPU tensors: ops.call and
swin_transformer.call are replaced by a recorder, ops.ptr and swin_transformer.ptr by a wrapper that keeps every tensor alive (so every address
is unique for the life of a case), and the library is only dlopen'ed for its *_supported / *_workspace_floats queries - no GPU call is made.
A trace is the list of calls of one case: [entry point, arguments ..., act dtype code or null, booked [flops, bytes, tag] or null] with every
pointer written "p<k>" (k = order of first appearance in the case: WHICH buffer is wired to which argument), None as null, scalars as they are
and a byref'd struct as {"Epilogue" / "Geom": [fields ...]} with its pointers numbered the same way.  A block case ends with one more record,
["*_site", answers ...]: what the public per-site predicates (ln_quant_site, ln_quant_mx_site, mx_store_site, mx_emit_site) say under its switches.

Cases: set_linear_fp8 off / on x recipe x backward x backward_recipe x store x set_ln_quant_mx x set_mx_producer_quant x set_mx_dual_quant x
fused (set_fused_mlp, set_fused_attn_block, set_fused_mlp_mx(on, backward=on) together) x save at (C = 96, 3 heads, res 14) and (C = 192,
6 heads, res 7), one image, bf16 math and storage; plus fp8 attention, the fused forward over the unfused backward, drop-path, the row
recipe without the quantising LayerNorm, a weight-pack cache, f32 math with every switch on, and a patch-merging stage of two blocks.

Writes tests/golden/swin_host_trace.json (case -> index of its trace among the distinct ones, the SHA-1 of every distinct trace, and the few
traces that together show every entry point in full); tests/test_cpu_swin_host_trace.py runs the same cases and asserts equality.  The fixture is generated ONCE, from the code whose behaviour is to be kept, and not again after that code changed.

  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_swin_host_trace.py
"""
import contextlib
import hashlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "swin_host_trace.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULTS = dict(math="bf16", fp8=False, recipe="row", bwd=False, brec="row", store="bf16", lnq=True, lnmx=False, prod=True, dual=False, fused=True,
                attn_bwd=True, attn8=0, save=True, drop=False, cache=False)
SHAPES = {"c96": (96, 3, 14), "c192": (192, 6, 7)}     # (C, heads, res)
ENV = ("SV_MX_PRODUCER_QUANT", "SV_LN_QUANT_FUSED", "SV_LN_QUANT_MX", "SV_MX_DUAL_QUANT", "SV_FUSED_MLP_MX", "SV_FUSED_MLP_MX_BWD", "SV_FUSED_MLP_MAX_C",
       "SV_FUSED_ATTN_BLOCK", "SV_FUSED_ATTN_BWD")


def cases():
    """[(name, what, settings)]: what = a key of SHAPES or "stage"; settings = the entries that differ from DEFAULTS"""
    out = []
    for shape in SHAPES:
        for fused, save in itertools.product((True, False), repeat=2):
            out.append((shape, dict(fused=fused, save=save)))
        for recipe, bwd, brec, store, lnmx, prod, dual, fused, save in itertools.product(("row", "mx"), (False, True), ("row", "mx"), ("bf16", "mx"),
                                                                                         *[(False, True)] * 5):
            out.append((shape, dict(fp8=True, recipe=recipe, bwd=bwd, brec=brec, store=store, lnmx=lnmx, prod=prod, dual=dual, fused=fused, save=save)))
    row, mx = dict(fp8=True, bwd=True), dict(fp8=True, bwd=True, recipe="mx", brec="mx")
    full = dict(mx, store="mx", lnmx=True, dual=True)
    for extra in (dict(), row, dict(mx), dict(mx, store="mx")):
        out.append(("stage", extra))
        out.append(("stage", dict(extra, cache=True)))
    for attn8 in (1, 2):                                   # fp8 attention switches the fused attention branches off
        out.append(("c96", dict(attn8=attn8)))
        out.append(("c96", dict(full, attn8=attn8)))
    for extra in (dict(), dict(mx, store="mx"), full):     # fused forward, unfused backward of the attention branch
        out.append(("c96", dict(extra, attn_bwd=False)))
    for extra in (dict(), dict(fused=False), dict(row, fused=False), dict(full, fused=False)):
        out.append(("c96", dict(extra, drop=True)))
    for extra in (dict(fp8=True, fused=False), dict(row, fused=False)):        # row recipe, LayerNorm + stand-alone quantiser
        out.append(("c192", dict(extra, lnq=False)))
    for extra in (full, dict(full, fused=False)):
        out.append(("c96", dict(extra, cache=True)))
    for fused in (True, False):
        out.append(("c96", dict(math="f32", fused=fused)))
        out.append(("c96", dict(full, math="f32", fused=fused)))
    named = []
    for what, s in out:
        s = {k: v for k, v in s.items() if DEFAULTS[k] != v}
        named.append((what + "".join(f" {k}={s[k]}" for k in DEFAULTS if k in s), what, s))
    assert len({n for n, _, _ in named}) == len(named)
    return named


class _Tracer:
    """hip.TRACE stand-in that listens to every entry point: begin() keeps what the caller books, nothing is timed"""

    class _All:
        def __contains__(self, name):
            return True

    names = _All()

    def __init__(self):
        self.open = None

    def begin(self, name, flops=0.0, nbytes=0.0, tag=""):
        self.open = [float(flops), float(nbytes), tag]

    def end(self):
        self.open = None


class Recorder:
    def __init__(self, hip):
        self.hip, self.tracer = hip, _Tracer()
        self.reset()

    def reset(self):
        self.keep, self.names, self.calls = [], {}, []

    def ptr(self, t):
        if t is None:
            return None
        self.keep.append(t)
        return t.data_ptr()

    def _p(self, v):
        return None if v is None else self.names.setdefault(int(v), f"p{len(self.names)}")

    def _struct(self, s):
        import ctypes as C
        return {type(s).__name__: [self._p(getattr(s, f)) if t is C.c_void_p else getattr(s, f) for f, t in s._fields_]}

    def call(self, name, *args, act=None):
        import ctypes as C
        types = self.hip._argtypes(name)
        assert len(args) + (2 if name in self.hip._ACT_TYPED else 1) == len(types), (name, len(args), len(types))
        rec = [name]
        for a, t in zip(args, types):
            if hasattr(a, "_obj"):
                rec.append(self._struct(a._obj))
            elif t is C.c_void_p:
                rec.append(self._p(a))
            else:
                assert isinstance(a, (int, float)), (name, a)
                rec.append(a)
        rec.append((self.hip.ACT if act is None else act) if name in self.hip._ACT_TYPED else None)
        rec.append(self.tracer.open)
        self.calls.append(rec)


@contextlib.contextmanager
def recording():
    """Recorder in place of call / ptr (and a tracer that books without timing); on exit every replaced function, every switch, the storage
    dtype code, the pack cache, the counters and the environment are what they were."""
    from swinvox_amd import hip, ops
    from swinvox_amd.models import swin_transformer as st
    rec = Recorder(hip)
    saved = (dict(ops._STATE), hip.ACT, hip.TRACE, ops.call, ops.ptr, st.call, st.ptr, ops._CTX.packs, ops._CTX.dyq, ops._MX_ACT_QUANT[0],
             {k: os.environ.pop(k) for k in ENV if k in os.environ})
    try:
        ops.call = st.call = rec.call
        ops.ptr = st.ptr = rec.ptr
        hip.TRACE = rec.tracer
        yield rec
    finally:
        state, hip.ACT, hip.TRACE, ops.call, ops.ptr, st.call, st.ptr, ops._CTX.packs, ops._CTX.dyq, ops._MX_ACT_QUANT[0], env = saved
        ops._STATE.clear()
        ops._STATE.update(state)
        os.environ.update(env)


def _apply(s):
    from swinvox_amd import ops
    ops.set_math(s["math"])
    ops.set_storage(s["math"])
    ops.set_linear_fp8(s["fp8"], backward=s["bwd"], recipe=s["recipe"], backward_recipe=s["brec"], store=s["store"])
    ops.set_ln_quant_fused(s["lnq"])
    ops.set_ln_quant_mx(s["lnmx"])
    ops.set_mx_producer_quant(s["prod"])
    ops.set_mx_dual_quant(s["dual"])
    ops.set_fused_mlp(s["fused"])
    ops.set_fused_attn_block(s["fused"])
    ops.set_fused_mlp_mx(s["fused"], backward=s["fused"])
    ops.set_fused_attn_block_bwd(s["attn_bwd"])
    ops.set_attention_fp8(s["attn8"] > 0, backward=s["attn8"] > 1)
    ops.set_pack_cache(ops.PackCache() if s["cache"] else None)


def _site_answers(blk, x):
    """["*_site", answers ...]: the public per-site predicates under the current switches, for qkv, proj, fc1 and fc2 with the epilogue forms
    block_forward uses: ln_quant_site, ln_quant_mx_site, mx_store_site, mx_emit_site each, then mx_emit_site of fc2 behind the linear fc1"""
    from swinvox_amd import ops
    a, m, tail = blk.attn, blk.mlp, dict(residual=x, ldr=blk.dim, rows_per_scale=blk.res * blk.res)
    fc1, fc2 = dict(bias=m.fc1.bias, act=ops.ACT_GELU), dict(bias=m.fc2.bias, **tail)
    out = ["*_site"]
    for spec, w, epi in ((blk.s_qkv, a.qkv.weight, dict(bias=a.qkv.bias)), (blk.s_proj, a.proj.weight, dict(bias=a.proj.bias, **tail)),
                         (blk.s_fc1, m.fc1.weight, fc1), (blk.s_fc2, m.fc2.weight, fc2)):
        out += [ops.ln_quant_site(spec, w, **epi), ops.ln_quant_mx_site(spec, w, **epi), ops.mx_store_site(spec, w, **epi), ops.mx_emit_site(spec, w, epi)]
    out.append(ops.mx_emit_site(blk.s_fc2, m.fc2.weight, fc2, blk.s_fc1, m.fc1.weight, fc1))
    assert all(v is True or v is False for v in out[1:]), out
    return out


def trace_all():
    """{case name: trace} of every case of cases()"""
    from swinvox_amd import ops
    from swinvox_amd.models import swin_transformer as st
    torch.manual_seed(0)
    blocks = {k: st.SwinBlock(C, res, heads, 3, 0.0) for k, (C, heads, res) in SHAPES.items()}
    stage = st.SwinStage(96, 192, 7, 2, 6, [0.0, 0.0], True)
    out = {}
    with recording() as rec:
        for name, what, diff in cases():
            s = dict(DEFAULTS, **diff)
            _apply(s)
            rec.reset()
            mod = stage if what == "stage" else blocks[what]
            for b in (stage.blocks if what == "stage" else [mod]):
                b.drop_path = 0.1 if s["drop"] else 0.0
            grads = {p: torch.zeros_like(p) for p in mod.parameters()}
            seeds = itertools.count(1000).__next__
            rows, Cin = (14 * 14, 96) if what == "stage" else (mod.res * mod.res, mod.dim)
            x = ops.empty(rows, Cin, device="cpu")
            fwd, bwd = (st.stage_forward, st.stage_backward) if what == "stage" else (st.block_forward, st.block_backward)
            y, tape = fwd(mod, x, 1, s["drop"], s["drop"], seeds, s["save"])
            if s["save"]:
                bwd(mod, tape, ops.empty(*y.shape, device="cpu"), grads, *([1] if what == "stage" else []))
            if what != "stage":
                rec.calls.append(_site_answers(mod, x))
            out[name] = json.loads(json.dumps(rec.calls))      # what the fixture holds: lists, no tuples
            rec.reset()
    return out


def sha1(obj):
    return hashlib.sha1(json.dumps(obj).encode()).hexdigest()


def pack(traces):
    """{case: trace} -> the fixture: "names" = SHA-1 of the case names in order, "cases" = index of every case's trace among the distinct
    ones, "sha1" = SHA-1 of every distinct trace, "traces" = {index: the full trace} for a few of them that together show every entry
    point (a greedy cover, largest gain first): what a reader looks at, and where a mismatch is reported call by call."""
    distinct, index, of = [], {}, []
    for t in traces.values():
        key = json.dumps(t)
        if key not in index:
            index[key] = len(distinct)
            distinct.append(t)
        of.append(index[key])
    shown, seen = {}, set()
    while True:
        gain, i = max((len({c[0] for c in t} - seen), -i) for i, t in enumerate(distinct))
        if gain == 0:
            break
        shown[str(-i)] = distinct[-i]
        seen |= {c[0] for c in distinct[-i]}
    return {"names": sha1(list(traces)), "cases": of, "sha1": [sha1(t) for t in distinct], "traces": shown}


def main():
    sys.dont_write_bytecode = True
    from swinvox_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        sys.exit(f"{hip.LIB_PATH} is missing: build the library first (its *_supported queries decide the paths)")
    traces = trace_all()
    again = trace_all()
    assert json.dumps(traces) == json.dumps(again), "two runs differ"
    fx = pack(traces)
    with open(FIXTURE, "w") as f:                           # one call per line: a changed call shows as one changed line
        rows = [", ".join(map(str, fx["cases"][i:i + 64])) for i in range(0, len(fx["cases"]), 64)]
        f.write('{"names": "%s",\n"cases": [\n%s\n],\n"sha1": [\n%s\n],\n"traces": {\n' % (
            fx["names"], ",\n".join(rows), ",\n".join(json.dumps(h) for h in fx["sha1"])))
        f.write(",\n".join('"%s": [\n' % i + ",\n".join(" " + json.dumps(c) for c in t) + "\n]" for i, t in fx["traces"].items()) + "\n}}\n")
    entries = sorted({c[0] for t in traces.values() for c in t} - {"*_site"})
    print(f"{len(fx['cases'])} cases, {len(fx['sha1'])} distinct traces ({len(fx['traces'])} in full), at most {max(len(t) for t in traces.values())} "
          f"calls per case, {len(entries)} entry points: {' '.join(entries)}; {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    main()
