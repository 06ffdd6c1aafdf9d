"""Host-side operator layer over the C ABI: geometry bookkeeping, weight packing, forward / data-grad /
weight-grad calls of the contraction engine, and the normalisation / pooling wrappers.

Everything here only enqueues HIP kernels on the current torch stream; torch is used for buffer
allocation (caching allocator) and nothing else.  Activations are channels-last and live in HBM in the current STORAGE
dtype (fp32, or bf16 under set_storage("bf16")); parameters, their gradients and all statistics are always fp32.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from dataclasses import dataclass
from typing import Any, NamedTuple, Optional, Tuple

import torch

from . import hip
from .hip import ACT_GELU, ACT_LRELU, ACT_NONE, ACT_RELU, Epilogue, Geom, call, ptr  # noqa: F401

# Process-wide CONFIGURATION (set_math / set_storage / set_overlap): read-only while modules run.
_STATE = {"math": hip.MATH_F32, "store": torch.float32}


class _CallContext(threading.local):
    """Per-thread context of the module pass that is running on this thread (weight-pack cache, zero arena, weight-gradient
    stream, BatchNorm tick list).  torch.nn.DataParallel (reference core/train.py:156-161) calls the modules' forward from
    one Python thread per device, so nothing mutable on the launch path may be shared between threads."""
    packs = None
    arena = None
    awg = None
    bn_tick = None
    dyq = None      # one-slot stash of the MX dual quantiser: (dy, rows, N, row bytes, row scales) between swin_linear_wgrad and swin_linear_dgrad


_CTX = _CallContext()


def named_tape(name: str, fields: str):
    """The type of what a forward keeps for its backward: a tuple whose entries are read by name."""
    return NamedTuple(name, [(f, Any) for f in fields.split()])

BN_SLOTS = 16   # SV_BN_SLOTS of include/swinvox_hip.h
BN_BWD_SLOTS, LN_BWD_SLOTS = 16, 32   # slot counts behind sv_bn_bwd_workspace_doubles / sv_layernorm_bwd_workspace_floats


def _switch(key: str, env: str, default: bool) -> bool:
    """An A/B switch: the flag set_X() keeps in _STATE, or the environment variable.  A default-on switch is switched OFF by set_X(False) or
    VAR=0, a default-off switch is switched ON by set_X(True) or VAR=1."""
    if default:
        return bool(_STATE.get(key, True)) and os.environ.get(env, "1") != "0"
    return bool(_STATE.get(key, False)) or os.environ.get(env, "0") == "1"


def set_math(mode: str) -> None:
    """'f32' = exact fp32 MFMA (parity mode); 'bf16' = bf16 MFMA inputs, fp32 accumulate.  Switching to 'f32' also
    switches the activation storage back to fp32 (bf16 storage needs bf16 math)."""
    _STATE["math"] = {"f32": hip.MATH_F32, "fp32": hip.MATH_F32, "bf16": hip.MATH_BF16}[mode]
    if _STATE["math"] == hip.MATH_F32:
        set_storage("f32")


def get_math() -> str:
    return "bf16" if _STATE["math"] == hip.MATH_BF16 else "f32"


def set_storage(mode: str) -> None:
    """HBM element type of the activations (and activation gradients) INSIDE the four modules: 'f32' or 'bf16'.
    Module inputs / outputs stay fp32 torch tensors (converted at the boundary); arithmetic, statistics, parameters and
    parameter gradients stay fp32.  'bf16' halves the activation traffic of the path and requires set_math('bf16')."""
    dt = {"f32": torch.float32, "fp32": torch.float32, "bf16": torch.bfloat16}[mode]
    if dt == torch.bfloat16 and _STATE["math"] != hip.MATH_BF16:
        raise RuntimeError("swinvox_amd: bf16 activation storage requires set_math('bf16')")
    _STATE["store"] = dt
    hip.ACT = hip.BF16 if dt == torch.bfloat16 else hip.F32


def get_storage() -> str:
    return "bf16" if _STATE["store"] == torch.bfloat16 else "f32"


def empty(*shape, like: torch.Tensor = None, device=None) -> torch.Tensor:
    """ACTIVATION buffer (current storage dtype)."""
    return torch.empty(*shape, dtype=_STATE["store"], device=like.device if like is not None else device)


def zeros(*shape, like: torch.Tensor = None, device=None) -> torch.Tensor:
    """Zero-filled ACTIVATION buffer (current storage dtype)."""
    return torch.zeros(*shape, dtype=_STATE["store"], device=like.device if like is not None else device)


def fempty(*shape, like: torch.Tensor = None, device=None) -> torch.Tensor:
    """fp32 buffer: weight packs, statistics, workspaces, parameter-shaped scratch."""
    return torch.empty(*shape, dtype=torch.float32, device=like.device if like is not None else device)


def fzeros(*shape, like: torch.Tensor = None, device=None) -> torch.Tensor:
    return torch.zeros(*shape, dtype=torch.float32, device=like.device if like is not None else device)


def to_store(t: torch.Tensor) -> torch.Tensor:
    """fp32 module input -> contiguous activation in the current storage dtype (no-op copy avoided for fp32 storage)."""
    t = t.contiguous()
    if t.dtype == _STATE["store"]:
        return t
    out = torch.empty(t.shape, dtype=_STATE["store"], device=t.device)
    call("sv_cast", ptr(t), hip.F32 if t.dtype == torch.float32 else hip.BF16, ptr(out), hip.ACT, t.numel())
    return out


def to_f32(t: torch.Tensor) -> torch.Tensor:
    """contiguous activation -> fp32 module output."""
    if t.dtype == torch.float32:
        return t
    assert t.is_contiguous()
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    call("sv_cast", ptr(t), hip.BF16, ptr(out), hip.F32, t.numel())
    return out


def _t3(v) -> Tuple[int, int, int]:
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(x) for x in v)
    return (1,) * (3 - len(v)) + v if len(v) < 3 else v


def _pad3(v, fill) -> Tuple[int, int, int]:
    """2-D parameters are lifted to 3-D with a unit depth axis."""
    if isinstance(v, int):
        return (v, v, v)
    v = tuple(int(x) for x in v)
    return (fill,) * (3 - len(v)) + v


def _epilogue(ldc, col_off=0, bias=None, residual=None, ldr=0, row_scale=None, rows_per_scale=1, pre_act=None, stats=None,
              act=ACT_NONE, slope=0.0, act_grad_src=None, act_grad_kind=ACT_NONE) -> Epilogue:
    return Epilogue(ptr(bias), ptr(residual), ldr, ptr(row_scale), rows_per_scale, ptr(pre_act), ptr(stats), act, slope,
                    ptr(act_grad_src), act_grad_kind, ldc, col_off)


@dataclass
class ConvSpec:
    """Geometry of one Linear / Conv / ConvTranspose layer (3-D form; 2-D layers use a unit depth axis)."""
    cin: int
    cout: int
    k: Tuple[int, int, int] = (1, 1, 1)
    s: Tuple[int, int, int] = (1, 1, 1)
    p: Tuple[int, int, int] = (0, 0, 0)
    transposed: bool = False
    cin_mem: Optional[int] = None    # channels the input activation holds in memory (zero-padded), default cin
    cout_mem: Optional[int] = None   # channels the output-gradient holds in memory, default cout
    og_fixed: Optional[Tuple[int, int, int]] = None   # output grid when it is not the symmetric-padding formula (asymmetric pads)

    def __post_init__(self):
        self.cin_mem = self.cin_mem or self.cin
        self.cout_mem = self.cout_mem or self.cout
        self.taps = self.k[0] * self.k[1] * self.k[2]

    @staticmethod
    def conv2d(cin, cout, k, s=1, p=0, **kw):
        return ConvSpec(cin, cout, _pad3(k if not isinstance(k, int) else (k, k), 1), _pad3(s if not isinstance(s, int) else (s, s), 1),
                        _pad3(p if not isinstance(p, int) else (p, p), 0), False, **kw)

    @staticmethod
    def conv3d(cin, cout, k, s=1, p=0, transposed=False, **kw):
        return ConvSpec(cin, cout, _t3(k), _t3(s), _t3(p), transposed, **kw)

    @staticmethod
    def linear(cin, cout):
        return ConvSpec(cin, cout)

    def out_grid(self, g):
        if self.og_fixed is not None:
            return tuple(self.og_fixed)
        if self.transposed:
            return tuple((g[i] - 1) * self.s[i] - 2 * self.p[i] + self.k[i] for i in range(3))
        return tuple((g[i] + 2 * self.p[i] - self.k[i]) // self.s[i] + 1 for i in range(3))

    # ---- weight packs (device copies made once per step; element type = the activation storage dtype) --------
    def pack_args(self, kind: str):
        """(A, B, T, swap, pad_to, rows_out, inner_out) of sv_pack_weight for the forward ('f': [cout][tap][cin_mem]) or the
        data-gradient ('d': [cin][tap][cout_mem]) pack of the native parameter ([cout,cin,k..] conv / [cin,cout,k..] tconv)."""
        A, B = (self.cin, self.cout) if self.transposed else (self.cout, self.cin)
        if kind == "f":
            swap, pad = (1 if self.transposed else 0), self.cin_mem
        else:
            swap, pad = (0 if self.transposed else 1), self.cout_mem
        rows, inner = (B, max(A, pad)) if swap else (A, max(B, pad))
        return A, B, self.taps, swap, pad, rows, inner

    def _pack(self, w: torch.Tensor, kind: str) -> torch.Tensor:
        dt = _STATE["store"]
        if kind == "f" and dt == torch.float32 and not self.transposed and self.taps == 1 and self.cin_mem == self.cin:
            return w  # Linear / 1x1 conv in fp32: the native layout already is the packed layout
        cache = _CTX.packs
        if cache is not None and isinstance(w, torch.nn.Parameter):   # temporaries (re-indexed copies) would add an entry per step
            return cache.get(self, w, kind)
        return pack_one(self, w, kind)

    def pack_fwd(self, w: torch.Tensor) -> torch.Tensor:
        return self._pack(w, "f")

    def pack_dgrad(self, w: torch.Tensor) -> torch.Tensor:
        return self._pack(w, "d")

    def _geom(self, n, gathered_grid, produced_grid, ci, co, ldi) -> Geom:
        return Geom(n, *gathered_grid, *produced_grid, ci, co, *self.k, *self.s, *self.p, ldi)

    def _traced(self, name, n, in_grid, *args):
        """Launch a contraction; when bench.py's tracer is active, bracket it with HIP events and book its ALGORITHMIC
        work: 2 * positions * taps_that_contribute * cin * cout flops (no channel padding, no masked taps)."""
        tr = hip.TRACE
        if tr is None or name not in tr.names:
            return call(name, *args)
        og = self.out_grid(in_grid)
        if self.transposed:   # every input position meets every tap exactly once
            pairs = n * in_grid[0] * in_grid[1] * in_grid[2] * self.taps
        else:                 # interior count; border taps falling into the padding are a small over-estimate (<3%)
            pairs = n * og[0] * og[1] * og[2] * self.taps
        flops = 2.0 * pairs * self.cin * self.cout
        nin, nout = n * in_grid[0] * in_grid[1] * in_grid[2], n * og[0] * og[1] * og[2]
        esz = 2.0 if _STATE["store"] == torch.bfloat16 else 4.0
        nbytes = esz * (nin * self.cin + nout * self.cout) + 4.0 * self.taps * self.cin * self.cout
        tr.begin(name, flops, nbytes, tag=f"n={n} grid={in_grid} cin={self.cin} cout={self.cout} k={self.k} s={self.s} t={int(self.transposed)}")
        call(name, *args)
        tr.end()

    def _halo_tconv(self, in_grid, ldi, ldc, epi) -> bool:
        return (self.transposed and self.k == (4, 4, 4) and self.s == (2, 2, 2) and self.p == (1, 1, 1) and self.cin == 32
                and self.cin_mem == 32 and self.cout == 8 and _STATE["store"] == torch.bfloat16 and _STATE["math"] != hip.MATH_F32
                and ldi in (None, 32) and ldc in (None, 8) and not (set(epi) - {"bias", "stats"})
                and in_grid[0] % 4 == 0 and in_grid[1] % 4 == 0 and in_grid[2] % 8 == 0)

    # ---- forward ------------------------------------------------------------------------------------
    def forward(self, x, n, in_grid, w_packed, out, *, ldi=None, ldc=None, **epi):
        og = self.out_grid(in_grid)
        if isinstance(w_packed, torch.nn.Parameter) or w_packed.dtype != _STATE["store"]:
            w_packed = self.pack_fwd(w_packed)     # raw parameter: pack / convert (identity for a Linear in fp32 storage)
        if self._halo_tconv(in_grid, ldi, ldc, epi):
            # k4 s2 p1, 32 -> 8 channels (decoder layer4): parity-class stencils on an LDS halo brick instead of L2 gathers
            self._traced("sv_tconv4s2_fwd", n, in_grid, ptr(x), ptr(w_packed), ptr(epi.get("bias")), ptr(out), ptr(epi.get("stats")),
                         n, *in_grid, self.cin, self.cout)
            return og
        g = self._geom(n, in_grid, og, self.cin_mem, self.cout, ldi or self.cin_mem)
        e = _epilogue(ldc or self.cout, **epi)
        self._traced("sv_tconv_gather" if self.transposed else "sv_conv_gather", n, in_grid, ptr(x), ptr(w_packed), ptr(out),
                     C.byref(g), C.byref(e), _STATE["math"])
        return og

    # ---- data gradient: dx[., cin] from dy[., cout_mem] -----------------------------------------------
    def dgrad(self, dy, n, in_grid, w_dgrad, dx, *, lddy=None, lddx=None, **epi):
        og = self.out_grid(in_grid)
        g = self._geom(n, og, in_grid, self.cout_mem, self.cin, lddy or self.cout_mem)
        e = _epilogue(lddx or self.cin_mem, **epi)
        # 1x1 / stride 1 / pad 0 (every Linear and 1x1 conv): the data-gradient is the same dense gather with the
        # transposed weight pack -> use the plain gather kernel, no parity classes
        dense = self.taps == 1 and self.s == (1, 1, 1) and self.p == (0, 0, 0)
        self._traced("sv_conv_gather" if (self.transposed or dense) else "sv_tconv_gather", n, in_grid, ptr(dy), ptr(w_dgrad), ptr(dx),
                     C.byref(g), C.byref(e), _STATE["math"])

    # ---- weight gradient, accumulated into dw (native layout) ------------------------------------------
    def wgrad(self, dy, x, n, in_grid, dw, *, lddy=None, ldx=None, db=None, async_ok=True):
        """dw += ...; for (non-transposed) conv / Linear layers db (bias gradient = column sums of dy) is folded into the
        same kernel; transposed convs anchor on x, so their bias gradient needs the separate column-sum kernel.
        Inside a module backward the launch goes to the weight-gradient stream (AsyncWgrad): nothing on the data-gradient
        chain waits for a weight gradient.  async_ok=False keeps it on the caller's stream - required when dy or x is
        modified in place afterwards."""
        run_on_wgrad_stream((dy, x), lambda: self._wgrad(dy, x, n, in_grid, dw, lddy, ldx, db), enable=async_ok)

    def _wgrad(self, dy, x, n, in_grid, dw, lddy, ldx, db):
        og = self.out_grid(in_grid)
        if self.transposed:   # anchor = x (cin), gathered = dy (cout)
            g = self._geom(n, og, in_grid, self.cout_mem, self.cin, lddy or self.cout_mem)
            ws = fempty(self.cin * self.taps * self.cout_mem, like=dw) if self.taps > 1 else None
            self._traced("sv_conv_wgrad", n, in_grid, ptr(x), ldx or self.cin_mem, ptr(dy), ptr(dw), C.byref(g), self.cout, ptr(ws),
                         None, _STATE["math"])
            if db is not None:
                colsum(dy, n * og[0] * og[1] * og[2], self.cout, lddy or self.cout_mem, db)
        else:                 # anchor = dy (cout), gathered = x (cin)
            g = self._geom(n, in_grid, og, self.cin_mem, self.cout, ldx or self.cin_mem)
            ws = fempty(self.cout * self.taps * self.cin_mem, like=dw) if self.taps > 1 else None
            self._traced("sv_conv_wgrad", n, in_grid, ptr(dy), lddy or self.cout_mem, ptr(x), ptr(dw), C.byref(g), self.cin, ptr(ws),
                         ptr(db), _STATE["math"])


def pack_one(spec: "ConvSpec", w: torch.Tensor, kind: str) -> torch.Tensor:
    """One weight pack with its own launch (first step of a module, tests)."""
    A, B, T, swap, pad, rows, inner = spec.pack_args(kind)
    out = torch.empty(rows * T * inner, dtype=_STATE["store"], device=w.device)
    call("sv_pack_weight", ptr(w), ptr(out), A, B, T, swap, pad, hip.ACT)
    return out


class PackCache:
    """All weight packs of one module from ONE batched launch per forward (sv_pack_weights).

    The first forward/backward of a module packs each weight individually and registers the request; from the next
    refresh() on, every registered pack is produced by one launch into a flat buffer and get() only hands out views.
    Packs made at forward time serve the backward of the same step (weights change only in optimizer.step())."""

    def __init__(self):
        self.tables = {}   # storage dtype -> dict(entries={key: [spec, w, kind, view]}, dirty, flat, descs, sig, nblocks)
        self.w8 = {}       # id(parameter) -> (e4m3 rows, row scales) of the running forward (quantize_weight_fp8); dropped by refresh()
        self.w8t = {}      # id(parameter) -> (e4m3 rows of W^T, their scales) for the fp8 data gradient (quantize_weight_t_fp8); same lifetime
        self.w8mx = {}     # id(parameter) -> (e4m3 rows, E8M0 block scales) of the MX recipe (quantize_weight_mx); same lifetime
        self.w8mxt = {}    # id(parameter) -> (e4m3 rows of W^T, their E8M0 block scales) for the MX data gradient (quantize_weight_t_mx); same lifetime

    def __deepcopy__(self, memo):
        return PackCache()    # keyed by parameter identity: a copied module starts with an empty cache

    def _table(self):
        return self.tables.setdefault(_STATE["store"], dict(entries={}, dirty=False, flat=None, descs=None, sig=None, nblocks=0))

    def get(self, spec, w, kind):
        t = self._table()
        key = (id(w), kind, spec.cin_mem, spec.cout_mem)
        e = t["entries"].get(key)
        if e is not None and e[3] is not None:
            return e[3]
        if e is None:
            t["entries"][key] = [spec, w, kind, None]
            t["dirty"] = True
        return pack_one(spec, w, kind)

    def refresh(self):
        """(Re)build the descriptor table when the set of packs or a parameter's address changed, then pack everything."""
        self.w8, self.w8t, self.w8mx, self.w8mxt = {}, {}, {}, {}
        t = self._table()
        ents = list(t["entries"].values())
        if not ents:
            return
        sig = tuple(e[1].data_ptr() for e in ents)
        if t["dirty"] or sig != t["sig"]:
            per_block = int(hip.load().sv_pack_weights_block_elems())
            dev = ents[0][1].device
            offs, total, blocks = [], 0, 0
            descs = (hip.PackDesc * len(ents))()
            for i, (spec, w, kind, _) in enumerate(ents):
                A, B, T, swap, pad, rows, inner = spec.pack_args(kind)
                n = rows * T * inner
                offs.append((total, n))
                descs[i].src, descs[i].A, descs[i].B, descs[i].T, descs[i].swap = w.data_ptr(), A, B, T, swap
                descs[i].rows_out, descs[i].inner_out, descs[i].block0 = rows, inner, blocks
                blocks += (n + per_block - 1) // per_block
                total += (n + 7) // 8 * 8          # every pack starts on a 16-byte boundary
            flat = torch.empty(max(total, 8), dtype=_STATE["store"], device=dev)
            esz = flat.element_size()
            for i, (o, n) in enumerate(offs):
                descs[i].dst = flat.data_ptr() + o * esz
                ents[i][3] = flat[o:o + n]
            raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
            t.update(dirty=False, flat=flat, descs=raw, sig=sig, nblocks=blocks)
        call("sv_pack_weights", ptr(t["descs"]), len(ents), t["nblocks"], hip.ACT)


class ZeroArena:
    """Zero-filled double scratch (BatchNorm statistic accumulators) for one module pass from ONE fill launch: the first
    pass measures the demand with individual torch.zeros calls, later passes slice one pre-zeroed buffer."""

    def __init__(self):
        self.need, self.used, self.buf, self.off = 0, 0, None, 0

    def begin(self, dev):
        self.used, self.off = 0, 0
        self.buf = torch.zeros(self.need, dtype=torch.float64, device=dev) if self.need else None

    def take(self, n, dev):
        self.used += n
        if self.buf is not None and self.off + n <= self.buf.numel():
            s = self.buf[self.off:self.off + n]
            self.off += n
            return s
        return torch.zeros(n, dtype=torch.float64, device=dev)

    def end(self):
        self.need, self.buf = max(self.need, self.used), None

    def __deepcopy__(self, memo):
        return ZeroArena()


def zeros_f64(n, dev):
    a = _CTX.arena
    return a.take(n, dev) if a is not None else torch.zeros(n, dtype=torch.float64, device=dev)


def bn_bwd_workspace(C, dev, layers=1):
    """[layers][sv_bn_bwd_workspace_doubles(C)] doubles, zero on entry: the slot images of one BatchNorm backward launch per row"""
    return zeros_f64(layers * ((BN_BWD_SLOTS + 1) * 2 * C + 2), dev).view(layers, -1)


def attn_bwd_workspace(heads, dev):
    """sv_window_attention_bwd_workspace_floats(heads) floats, zero on entry: the relative-position-bias gradient's slot images"""
    return zeros_f64(8 * 169 * heads, dev)


def set_arena(arena) -> None:
    _CTX.arena = arena


def bn_tick_flush() -> None:
    """num_batches_tracked += 1 for every BatchNorm that ran since the last flush, in one foreach launch."""
    lst = _CTX.bn_tick
    if lst:
        torch._foreach_add_(lst, 1)
    _CTX.bn_tick = []


class AsyncWgrad:
    """Weight-gradient stream of one module backward (see ConvSpec.wgrad).  join() makes the caller's stream wait for every
    weight gradient and releases the operand references."""
    _streams = {}

    def __init__(self, dev):
        key = (dev.type, dev.index)
        if key not in AsyncWgrad._streams:
            AsyncWgrad._streams[key] = torch.cuda.Stream(device=dev)
        self.stream, self.held = AsyncWgrad._streams[key], []

    def join(self):
        torch.cuda.current_stream().wait_stream(self.stream)
        self.held.clear()
        _CTX.dyq = None


def set_async_wgrad(aw) -> None:
    _CTX.awg = aw
    _CTX.dyq = None


def run_on_wgrad_stream(held, fn, wait=True, enable=True) -> bool:
    """fn() - launches that produce or move a weight gradient - on the weight-gradient stream of the running module backward; in place, on the
    caller's stream, when there is none or `enable` is False.  -> whether it went to that stream.
    held: the tensors fn reads that the caller's stream made; they stay referenced (alive and unrecycled) until AsyncWgrad.join().
    wait=True: the stream first waits for the caller's stream, where those tensors are complete.  wait=False is for a launch that only follows
    one already sent to that stream (it reads what that launch wrote): stream order is all it needs, and the caller's stream is not waited for.
    Temporaries fn allocates belong to the weight-gradient stream's pool and are recycled in its order."""
    aw = _CTX.awg
    if aw is None or not enable:
        fn()
        return False
    if wait:
        aw.stream.wait_stream(torch.cuda.current_stream())
    aw.held.append(held)
    with torch.cuda.stream(aw.stream):
        fn()
    return True


_SIDE = {}


def side_stream(dev) -> "torch.cuda.Stream":
    """Second HIP stream of a device for the independent ResNet / Swin branches of the encoder (forward and backward).
    Usage: side.wait_stream(main) [fork] ... with torch.cuda.stream(side): branch ... main.wait_stream(side) [join].
    Allocator safety: tensors allocated while the side stream is current return to ITS pool and are only re-used by later
    side-stream allocations, which follow a later fork (= wait on everything the main stream had queued); main-stream
    tensors read by the side branch must stay referenced until the join (callers keep them in locals / the tape)."""
    key = (dev.type, dev.index)
    if key not in _SIDE:
        # high priority: the Swin backbone that runs here is the longer of the two encoder branches (measured +0.35 %)
        _SIDE[key] = torch.cuda.Stream(device=dev, priority=-1)
    return _SIDE[key]


def set_seed_epoch(t: Optional[torch.Tensor]) -> None:
    """Device word (int32/uint32 tensor with one element, or None) that every stochastic launch mixes into its scalar seed ON
    THE DEVICE.  A captured hipGraph freezes scalar kernel arguments; a caller that replays a graph advances this word once per
    replay (graph.GraphedStep does) so that dropout / drop-path masks differ from step to step.  Process-wide configuration."""
    if t is not None and (not t.is_cuda or t.numel() != 1 or t.element_size() != 4):
        raise ValueError("seed epoch must be a one-element 32-bit tensor on the GPU")
    _STATE["seed_epoch"] = t


def seed_epoch_ptr():
    t = _STATE.get("seed_epoch")
    return t.data_ptr() if t is not None else None


_COMM = {}


def comm_stream(dev) -> "torch.cuda.Stream":
    """Staging stream of the data-parallel gradient hand-off (HipModule._announce)."""
    key = (dev.type, dev.index)
    if key not in _COMM:
        _COMM[key] = torch.cuda.Stream(device=dev)
    return _COMM[key]


def overlap_enabled() -> bool:
    return _STATE.get("overlap", True)


def set_overlap(on: bool) -> None:
    """Run the encoder's two backbone branches on two HIP streams (default on)."""
    _STATE["overlap"] = bool(on)


def set_pack_cache(cache) -> None:
    """Route ConvSpec.pack_fwd / pack_dgrad through `cache` (a PackCache, or None for one launch per pack)."""
    _CTX.packs = cache


def traced_call(name, flops, nbytes, *args, tag=""):
    """call() that books ALGORITHMIC flops / bytes with bench.py's tracer when it listens to `name`."""
    tr = hip.TRACE
    if tr is None or name not in tr.names:
        return call(name, *args)
    tr.begin(name, flops, nbytes, tag=tag)
    call(name, *args)
    tr.end()


def fused_mlp_enabled(C: int) -> bool:
    """The fused Swin MLP kernels (csrc/swin_mlp.hip) serve bf16 MFMA + bf16 storage and the channel counts they are built for."""
    # C = 192 (Swin-T stage 1) is built too, but since the wide dense kernels (csrc/igemm.hip) serve K = 192 the unfused chain is the faster
    # one there: 123.0 -> 121.7 ms per step at B = 64.  SV_FUSED_MLP_MAX_C overrides the limit for measurements.
    lim = int(os.environ.get("SV_FUSED_MLP_MAX_C", "128"))
    return (_STATE.get("fused_mlp", True) and _STATE["math"] == hip.MATH_BF16 and _STATE["store"] == torch.bfloat16
            and C <= lim and hip.load().sv_swin_mlp_supported(C) == 1)


def fused_attn_block_enabled(C: int, heads: int) -> bool:
    """The fused attention branch (LayerNorm -> qkv -> window attention -> proj -> residual, csrc/attn.hip) serves stage 0 of Swin-T
    (C = 96, 3 heads) in bf16 MFMA + bf16 storage; fp8 attention keeps the unfused chain (its core kernel is a separate build)."""
    if not _switch("fused_attn_block", "SV_FUSED_ATTN_BLOCK", True) or _STATE.get("attn_fp8"):
        return False
    return (_STATE["math"] == hip.MATH_BF16 and _STATE["store"] == torch.bfloat16
            and hip.load().sv_swin_attn_block_supported(C, heads, hip.BF16, hip.MATH_BF16) == 1)


def fused_attn_block_bwd_enabled(C: int, heads: int) -> bool:
    """The fused BACKWARD of the attention branch (csrc/attn.hip swin_attn_block_bwd_kernel) serves the same blocks as the fused forward; it
    reads what either forward stores (qkv, LayerNorm statistics), so fp8 attention in the forward does not switch it off.
    A/B: SV_FUSED_ATTN_BWD=0 or set_fused_attn_block_bwd(False) route the branch through the unfused four-kernel chain.  The fp8
    backward (set_attention_fp8(True, backward=True)) switches it off: its core kernel is a separate build."""
    if not _switch("fused_attn_block_bwd", "SV_FUSED_ATTN_BWD", True):
        return False
    if _STATE.get("attn_fp8") and _STATE.get("attn_fp8_bwd"):
        return False
    return (_STATE["math"] == hip.MATH_BF16 and _STATE["store"] == torch.bfloat16
            and hip.load().sv_swin_attn_block_supported(C, heads, hip.BF16, hip.MATH_BF16) == 1)


def set_fused_attn_block_bwd(on: bool) -> None:
    _STATE["fused_attn_block_bwd"] = bool(on)


def set_fused_attn_block(on: bool) -> None:
    """A/B switch: False routes the attention branch of every Swin block through the unfused LayerNorm / qkv / core / proj chain."""
    _STATE["fused_attn_block"] = bool(on)


def set_fused_attn_block_mx(on: bool) -> None:
    """Opt-in (off by default; SV_FUSED_ATTN_BLOCK_MX=1 in the environment switches it on as well): under set_linear_fp8(True, recipe="mx") the
    blocks that run the fused attention branch take its MXFP8 forward (sv_swin_attn_block_fwd_mx: the unfused MX chain norm1 -> qkv -> window
    attention -> proj in one kernel, qkv and proj on MX operands quantised in registers, the attention core in bf16).  The backward is the fused
    bf16 backward on the stored bf16 tensors, unchanged: the quantisers are straight-through, and the tape stays bf16 also under store "mx"."""
    _STATE["fused_attn_block_mx"] = bool(on)


def fused_attn_block_mx_enabled(C: int, heads: int) -> bool:
    """The MXFP8 forward of the fused attention branch: the switch, the fused branch itself (so it is inert under set_attention_fp8 and
    set_fused_attn_block(False)), MX linears, bf16 math and storage, C = 96 with 3 heads.  Inert everywhere else."""
    if not _switch("fused_attn_block_mx", "SV_FUSED_ATTN_BLOCK_MX", False):
        return False
    return (fused_attn_block_enabled(C, heads) and linear_fp8_enabled() and linear_fp8_recipe() == "mx"
            and _STATE["math"] == hip.MATH_BF16 and _STATE["store"] == torch.bfloat16
            and hip.load().sv_swin_attn_block_mx_supported(C, heads) == 1)


def swin_attn_block_mx_launches() -> int:
    """sv_swin_attn_block_fwd_mx launches of this process so far."""
    return int(hip.load().sv_swin_attn_block_mx_launches())


def swin_attn_block_mx_packs(wqkv: torch.Tensor, wproj: torch.Tensor, C: int) -> torch.Tensor:
    """The MX rows of qkv.weight / proj.weight (quantize_weight_mx: the unfused sites' bytes, from the module's pack cache) in the fragment
    order of sv_swin_attn_block_fwd_mx."""
    (wqq, wqs), (wpq, wps) = quantize_weight_mx(wqkv), quantize_weight_mx(wproj)
    packs = torch.empty(int(hip.load().sv_swin_attn_block_mx_pack_bytes(C)), dtype=torch.uint8, device=wqkv.device)
    call("sv_swin_attn_block_mx_pack", ptr(wqq), ptr(wqs), ptr(wpq), ptr(wps), ptr(packs), C)
    return packs


def set_attention_fp8(on: bool, backward: bool = False) -> None:
    """BASELINE configuration 5: QK^T and PV of the Swin window attention FORWARD on fp8 (OCP e4m3) MFMA operands with per-(window, head)
    scales; everything else keeps bf16 operands.  With backward=True the window-attention backward differentiates that fp8 forward
    (quantisers straight-through) with all five of its contractions on e4m3 operands; otherwise it is the bf16 backward.
    Needs set_math('bf16')."""
    _STATE["attn_fp8"] = bool(on)
    _STATE["attn_fp8_bwd"] = bool(on) and bool(backward)


def attention_math() -> int:
    """math code of the window-attention forward call"""
    return hip.MATH_FP8 if (_STATE.get("attn_fp8") and _STATE["math"] == hip.MATH_BF16) else _STATE["math"]


def attention_bwd_math() -> int:
    """math code of the window-attention backward call"""
    if _STATE.get("attn_fp8") and _STATE.get("attn_fp8_bwd") and _STATE["math"] == hip.MATH_BF16:
        return hip.MATH_FP8_FULL
    return _STATE["math"]


def set_fused_mlp(on: bool) -> None:
    """A/B switch: False routes every Swin MLP through the unfused LayerNorm / fc1 / fc2 chain of the contraction engine."""
    _STATE["fused_mlp"] = bool(on)


def set_fused_mlp_mx(on: bool, backward: bool = False, wgrad: bool = False) -> None:
    """Opt-in (off by default; SV_FUSED_MLP_MX=1 in the environment switches it on as well): under set_linear_fp8(True, recipe="mx") the blocks
    that run the fused Swin MLP take its MXFP8 forward (sv_swin_mlp_fwd_mx: the unfused MX chain in one kernel).  Without `backward` the backward
    is the fused bf16 backward, unchanged: the quantisers are straight-through.  backward=True (effective only with `on`; SV_FUSED_MLP_MX_BWD=1
    sets it as well) lets the data gradient of those blocks differentiate that very forward on MX operands (sv_swin_mlp_bwd_mx: the unfused MX
    backward chain in one kernel) while set_linear_fp8(..., backward=True, backward_recipe="mx") holds.  wgrad=True (effective only with `on`;
    SV_FUSED_MLP_MX_WGRAD=1 sets it as well; independent of `backward`) does the same for the weight gradients of those blocks
    (sv_swin_mlp_wgrad_mx: the unfused MX weight-gradient chain in one kernel, blocks of 32 tokens per column); without it they stay on
    sv_swin_mlp_wgrad (bf16 operands)."""
    _STATE["fused_mlp_mx"] = bool(on)
    _STATE["fused_mlp_mx_bwd"] = bool(on) and bool(backward)
    _STATE["fused_mlp_mx_wgrad"] = bool(on) and bool(wgrad)


def fused_mlp_mx_enabled(C: int) -> bool:
    """The MXFP8 forward of the fused Swin MLP: the switch, the fused MLP itself, MX linears, bf16 math and storage, C in {96, 128}."""
    if not _switch("fused_mlp_mx", "SV_FUSED_MLP_MX", False):
        return False
    return (fused_mlp_enabled(C) and linear_fp8_enabled() and linear_fp8_recipe() == "mx"
            and _STATE["math"] == hip.MATH_BF16 and _STATE["store"] == torch.bfloat16 and hip.load().sv_swin_mlp_mx_supported(C) == 1)


def swin_mlp_mx_launches() -> int:
    """sv_swin_mlp_fwd_mx launches of this process so far."""
    return int(hip.load().sv_swin_mlp_mx_launches())


def swin_mlp_mx_packs(w1: torch.Tensor, w2: torch.Tensor, C: int) -> torch.Tensor:
    """The MX rows of fc1.weight / fc2.weight (quantize_weight_mx: the unfused sites' bytes, from the module's pack cache) in the fragment
    order of sv_swin_mlp_fwd_mx."""
    (w1q, w1s), (w2q, w2s) = quantize_weight_mx(w1), quantize_weight_mx(w2)
    packs = torch.empty(int(hip.load().sv_swin_mlp_mx_pack_bytes(C)), dtype=torch.uint8, device=w1.device)
    call("sv_swin_mlp_mx_pack", ptr(w1q), ptr(w1s), ptr(w2q), ptr(w2s), ptr(packs), C)
    return packs


def fused_mlp_mx_bwd_enabled(C: int) -> bool:
    """The MXFP8 data gradient of the fused Swin MLP: its switch, the MX forward of the same block (fused_mlp_mx_enabled), the MX backward recipe
    of the Swin linears and a C the library serves.  Inert everywhere else."""
    if not _switch("fused_mlp_mx_bwd", "SV_FUSED_MLP_MX_BWD", False):
        return False
    return (fused_mlp_mx_enabled(C) and linear_fp8_bwd_enabled() and linear_fp8_bwd_recipe() == "mx"
            and hip.load().sv_swin_mlp_bwd_mx_supported(C) == 1)


def swin_mlp_mx_bwd_launches() -> int:
    """sv_swin_mlp_bwd_mx launches of this process so far."""
    return int(hip.load().sv_swin_mlp_bwd_mx_launches())


def swin_mlp_mx_bwd_packs(w1: torch.Tensor, w2: torch.Tensor, C: int) -> torch.Tensor:
    """The MX rows of fc1.weight, of fc2.weight^T and of fc1.weight^T (quantize_weight_mx / quantize_weight_t_mx: the unfused sites' bytes, from
    the module's pack cache) in the fragment order of sv_swin_mlp_bwd_mx."""
    (w1q, w1s), (w2tq, w2ts), (w1tq, w1ts) = quantize_weight_mx(w1), quantize_weight_t_mx(w2), quantize_weight_t_mx(w1)
    packs = torch.empty(int(hip.load().sv_swin_mlp_bwd_mx_pack_bytes(C)), dtype=torch.uint8, device=w1.device)
    call("sv_swin_mlp_bwd_mx_pack", ptr(w1q), ptr(w1s), ptr(w2tq), ptr(w2ts), ptr(w1tq), ptr(w1ts), ptr(packs), C)
    return packs


def fused_mlp_mx_wgrad_enabled(C: int) -> bool:
    """The MXFP8 weight gradients of the fused Swin MLP: their switch, the MX forward of the same block (fused_mlp_mx_enabled), the MX backward
    recipe of the Swin linears and a C the library serves.  Independent of the data-gradient switch; inert everywhere else."""
    if not _switch("fused_mlp_mx_wgrad", "SV_FUSED_MLP_MX_WGRAD", False):
        return False
    return (fused_mlp_mx_enabled(C) and linear_fp8_bwd_enabled() and linear_fp8_bwd_recipe() == "mx"
            and hip.load().sv_swin_mlp_wgrad_mx_supported(C) == 1)


def swin_mlp_mx_wgrad_launches() -> int:
    """sv_swin_mlp_wgrad_mx launches of this process so far."""
    return int(hip.load().sv_swin_mlp_wgrad_mx_launches())


def colsum(x, rows, cols, ld, out, accumulate=True):
    call("sv_colsum", ptr(x), rows, cols, ld, ptr(out), 1 if accumulate else 0)


# ---------------------------------------------------------------------------------------------------
# Linear helpers (rows x K) used by the Swin blocks
# ---------------------------------------------------------------------------------------------------
def linear_fwd(x, rows, spec: ConvSpec, w, out, **epi):
    spec.forward(x, rows, (1, 1, 1), w, out, **epi)


def set_linear_fp8(on: bool, backward: bool = False, recipe: str = "row", backward_recipe: str = "row", store: str = "bf16") -> None:
    """BASELINE configuration 5, linear part: the FORWARD of the Swin linears (qkv, proj, fc1, fc2, patch-merge reduction) on e4m3 operands
    with per-row scales and the block-scaled K = 128 MFMA (csrc/linear_fp8.hip).  The stored tensors are unchanged.  Without `backward` the
    backward is unchanged too (bf16 data and weight gradients: the quantisers are straight-through); with backward=True (effective only
    together with `on`) the data and weight gradients of the unfused Swin sites run on e4m3 operands as well (swin_linear_dgrad /
    swin_linear_wgrad).  Active only under set_math('bf16'); independent of set_attention_fp8.
    Blocks that run the fused stage-0 kernels keep their bf16 operands (set_fused_attn_block(False) / set_fused_mlp(False) unfuse them).
    Under recipe "mx" set_fused_mlp_mx(True) (off by default) gives the fused MLP an MXFP8 forward of its own (sv_swin_mlp_fwd_mx), and
    set_fused_mlp_mx(True, backward=True) under backward_recipe "mx" an MXFP8 data gradient as well (sv_swin_mlp_bwd_mx), wgrad=True its MXFP8
    weight gradients (sv_swin_mlp_wgrad_mx).  set_fused_attn_block_mx(True) (off by default) does the same for the FORWARD of the fused attention
    branch (sv_swin_attn_block_fwd_mx, C = 96 with 3 heads: qkv and proj on MX operands, the attention core in bf16); its backward stays the
    fused bf16 backward on the bf16 tape.  With both switches on no Swin linear of the forward is left on bf16 operands.
    The LayerNorms that feed qkv, fc1 and the reduction emit the quantised rows themselves (set_ln_quant_fused).
    recipe = "row" (default): one fp32 scale per operand row, divided out in the epilogue.  recipe = "mx": the FORWARD of the same call sites
    on MX operands - one E8M0 power-of-two scale per 32 consecutive elements of the contraction, applied by the MFMA (sv_linear_mxfp8).  A block
    scale depends on 32 neighbours only, so fc1 emits the operand rows of fc2 and the window attention those of proj (set_mx_producer_quant);
    the LayerNorm sites take the stand-alone MX quantiser unless set_ln_quant_mx(True) (off by default) lets norm1 / norm2 / the patch-merge
    norm emit the MX rows and block scales themselves (sv_layernorm_quant_mx_fwd), which leaves the unfused Swin forward without a stand-alone
    activation quantiser.  `backward` means the same under either recipe: its quantisers read the stored
    tensors, which do not change.
    backward_recipe = "row" (default): the backward above, whatever the forward recipe.  backward_recipe = "mx" (effective only with `on` and
    `backward`; combines with either forward recipe; inert under f32 math): both gradients on MX operands - dy per row and W^T, dy^T, x^T by the
    one-launch MX column quantiser (a block = 32 tokens of a column), sv_linear_mxfp8_dgrad and the atomic-free, deterministic
    sv_linear_mxfp8_wgrad.
    store = "bf16" (default): the training tape keeps the inputs of the linears (ln1, att, ln2, h, the patch-merge norm's output) in the storage
    type and the weight gradient quantises them again.  store = "mx" (effective only with `on`, `backward`, recipe "mx" and backward_recipe "mx"
    under bf16 math; inert otherwise): at the sites mx_store_site names the tape keeps the MX rows the forward GEMM consumed, (bytes, block scales),
    the tensor itself is not stored (an emitting producer does not write it at all) and the weight gradient re-blocks the rows along the tokens
    (sv_mx_rows_to_cols).  Outputs, data gradients and the fused stage-0 blocks do not change."""
    if recipe not in ("row", "mx"):
        raise ValueError(f"set_linear_fp8: recipe must be 'row' or 'mx', not {recipe!r}")
    if backward_recipe not in ("row", "mx"):
        raise ValueError(f"set_linear_fp8: backward_recipe must be 'row' or 'mx', not {backward_recipe!r}")
    if store not in ("bf16", "mx"):
        raise ValueError(f"set_linear_fp8: store must be 'bf16' or 'mx', not {store!r}")
    _STATE["linear_fp8"] = bool(on)
    _STATE["linear_fp8_bwd"] = bool(on) and bool(backward)
    _STATE["linear_fp8_recipe"] = recipe
    _STATE["linear_fp8_bwd_recipe"] = backward_recipe if (on and backward) else "row"
    _STATE["linear_fp8_store"] = store if (on and backward and recipe == "mx" and backward_recipe == "mx") else "bf16"


def linear_fp8_enabled() -> bool:
    return bool(_STATE.get("linear_fp8")) and _STATE["math"] == hip.MATH_BF16


def linear_fp8_recipe() -> str:
    """"row" or "mx": the recipe the fp8 forward of the Swin linears runs (meaningful while linear_fp8_enabled())."""
    return _STATE.get("linear_fp8_recipe", "row")


def _mx() -> bool:
    return linear_fp8_enabled() and linear_fp8_recipe() == "mx"


def set_mx_producer_quant(on: bool) -> None:
    """A/B switch of the MX producers: True (default) lets fc1 emit the MX operand rows of fc2 and the window attention those of proj; False
    sends every site through the stand-alone quantiser (sv_quant_rows_mx_e4m3), with bit-identical results.  SV_MX_PRODUCER_QUANT=0 in the
    environment switches it off as well.  Effective only under recipe "mx"."""
    _STATE["mx_producer_quant"] = bool(on)


def mx_producer_quant_enabled() -> bool:
    return _mx() and _switch("mx_producer_quant", "SV_MX_PRODUCER_QUANT", True)


_MX_ACT_QUANT = [0]


def mx_act_quant_launches() -> int:
    """Stand-alone MX quantiser launches on ACTIVATIONS of this process so far (weights are not counted)."""
    return _MX_ACT_QUANT[0]


def linear_mxfp8_launches() -> int:
    """sv_linear_mxfp8 launches of this process so far."""
    return int(hip.load().sv_linear_mxfp8_launches())


def _dtype_code(t: torch.Tensor) -> int:
    return hip.BF16 if t.dtype == torch.bfloat16 else hip.F32


def operand_buffers(rows: int, K: int, mx: bool, device):
    """The uninitialised (e4m3 bytes [rows, roundup(K, 128)], scales) pair of a quantised operand: fp32 scales [rows], one per row, or - mx -
    E8M0 block scales [rows, roundup(K, 128) / 32] uint8, one per 32 consecutive elements of a row."""
    Kp = (K + 127) // 128 * 128
    q = torch.empty(rows, Kp, dtype=torch.uint8, device=device)
    if mx:
        return q, torch.empty(rows, Kp // 32, dtype=torch.uint8, device=device)
    return q, torch.empty(rows, dtype=torch.float32, device=device)


def quantize_rows_mx(t: torch.Tensor, rows: int, K: int, ld: Optional[int] = None, activation: bool = True):
    """t [rows, K] (fp32 or bf16, row stride ld) -> (e4m3 bytes [rows, roundup(K, 128)], E8M0 block scales [rows, roundup(K, 128) / 32] uint8)
    by sv_quant_rows_mx_e4m3."""
    q, sc = operand_buffers(rows, K, True, t.device)
    call("sv_quant_rows_mx_e4m3", ptr(t), _dtype_code(t), rows, K, ld or K, ptr(q), q.shape[1], ptr(sc))
    if activation:
        _MX_ACT_QUANT[0] += 1
    return q, sc


def _weight_operand(w: torch.Tensor, table: str, quantise):
    """quantise(w, N, K) of a Linear weight [N, K]: one small launch, kept in PackCache table `table` for the running forward of the module
    (weights change only in optimizer.step(), the lifetime of the weight packs)."""
    cache = _CTX.packs
    if cache is None or not isinstance(w, torch.nn.Parameter):
        return quantise(w, w.shape[0], w.shape[1])
    held = getattr(cache, table)
    hit = held.get(id(w))
    if hit is None:
        hit = held[id(w)] = quantise(w, w.shape[0], w.shape[1])
    return hit


def quantize_weight_mx(w: torch.Tensor):
    """MX rows of a Linear weight [N, K] (not counted as an activation quantiser launch)."""
    return _weight_operand(w, "w8mx", lambda t, N, K: quantize_rows_mx(t, N, K, activation=False))


def mx_emit_site(cons_spec: ConvSpec, cons_w, cons_epi: dict, prod_spec: Optional[ConvSpec] = None, prod_w=None, prod_epi: Optional[dict] = None) -> bool:
    """Whether the producer of a Swin linear's input emits that linear's MX operand rows (LinearPlan.prod_emits); prod_*: the producer when it is
    a linear itself (fc1 in front of fc2).  With set_linear_fp8 off this is one flag test."""
    producer = True if prod_spec is None else swin_linear_plan(prod_spec, prod_w, False, **prod_epi)
    return swin_linear_plan(cons_spec, cons_w, False, producer=producer, **cons_epi).prod_emits


def linear_fp8_bwd_enabled() -> bool:
    return bool(_STATE.get("linear_fp8_bwd")) and linear_fp8_enabled()


def linear_fp8_bwd_recipe() -> str:
    """"row" or "mx": the recipe the fp8 backward of the Swin linears runs (meaningful while linear_fp8_bwd_enabled())."""
    return _STATE.get("linear_fp8_bwd_recipe", "row")


def linear_fp8_store() -> str:
    """"bf16" or "mx": what the training tape keeps of the inputs of the Swin linears - the EFFECTIVE value ("mx" only while the MX forward and
    the MX backward both run, which needs bf16 math)."""
    return "mx" if (_STATE.get("linear_fp8_store", "bf16") == "mx" and linear_fp8_bwd_enabled()) else "bf16"


def mx_store_site(spec: ConvSpec, w, **epi) -> bool:
    """Whether the tape keeps the MX rows of this Swin linear's input in place of the tensor (**epi: the linear's epilogue form;
    LinearPlan.keep of a forward that saves).  With the switch off this is one flag test."""
    return linear_fp8_store() == "mx" and swin_linear_plan(spec, w, True, **epi).keep


def mx_rows_to_cols_launches() -> int:
    """sv_mx_rows_to_cols launches of this process so far."""
    return int(hip.load().sv_mx_rows_to_cols_launches())


def mx_rows_to_cols(xq: torch.Tensor, xs: torch.Tensor, rows: int, K: int):
    """MX rows (xq [rows, roundup(K, 128)] e4m3 bytes, xs [rows, roundup(K, 128) / 32] E8M0 bytes) -> the MX column operand of the weight
    gradient (bytes [K, roundup(rows, 128)], block scales [K, roundup(rows, 128) / 32]; a block = 32 tokens of a column) by sv_mx_rows_to_cols:
    equal to quantize_cols_mx on the dequantised rows."""
    q, sc = operand_buffers(K, rows, True, xq.device)
    call("sv_mx_rows_to_cols", ptr(xq), xq.shape[1], ptr(xs), rows, K, ptr(q), q.shape[1], ptr(sc))
    return q, sc


def linear_mxfp8_bwd_launches() -> Tuple[int, int]:
    """(sv_linear_mxfp8_dgrad, sv_linear_mxfp8_wgrad) launches of this process so far; linear_fp8_bwd_launches() counts neither."""
    lib = hip.load()
    return int(lib.sv_linear_mxfp8_bwd_launches(0)), int(lib.sv_linear_mxfp8_bwd_launches(1))


def linear_fp8_bwd_launches() -> Tuple[int, int]:
    """(sv_linear_fp8_dgrad, sv_linear_fp8_wgrad) launches of this process so far; linear_fp8_launches() counts neither."""
    lib = hip.load()
    return int(lib.sv_linear_fp8_bwd_launches(0)), int(lib.sv_linear_fp8_bwd_launches(1))


def linear_fp8_launches() -> int:
    """sv_linear_fp8 launches of this process so far."""
    return int(hip.load().sv_linear_fp8_launches())


def quantize_rows_fp8(t: torch.Tensor, rows: int, K: int, ld: Optional[int] = None):
    """t [rows, K] (fp32 or bf16, row stride ld) -> (e4m3 bytes [rows, roundup(K, 128)], fp32 row scales [rows]) by sv_quant_rows_e4m3."""
    q, sc = operand_buffers(rows, K, False, t.device)
    call("sv_quant_rows_e4m3", ptr(t), _dtype_code(t), rows, K, ld or K, ptr(q), q.shape[1], ptr(sc))
    return q, sc


def quantize_weight_fp8(w: torch.Tensor):
    """Quantised rows and row scales of a Linear weight [N, K]."""
    return _weight_operand(w, "w8", quantize_rows_fp8)


def swin_linear_fp8_epilogue(spec: ConvSpec, w, **epi):
    """The sv_epilogue of a Swin linear that takes the fp8 kernel, None when it does not: set_linear_fp8(True) under bf16 math, a plain
    Linear on an unpadded input whose weight is a Parameter, and an epilogue form sv_linear_fp8 serves.  The one copy of these conditions:
    swin_linear_fwd runs on it, and the LayerNorm sites ask it BEFORE they normalise (with the epilogue keywords of the linear that follows;
    the query looks at the form, not at the output pointers) whether to emit the quantised rows from the LayerNorm kernel."""
    if not (linear_fp8_enabled() and spec.taps == 1 and spec.cin_mem == spec.cin and isinstance(w, torch.nn.Parameter)):
        return None
    e = _epilogue(spec.cout, **epi)
    return e if hip.load().sv_linear_fp8_supported(spec.cin, spec.cout, C.byref(e), _STATE["math"], hip.ACT) == 1 else None


# What the row and the MX recipe of the fp8 Swin linears differ in besides their MX-only parts: the three entry points, and the quantisers of
# activation rows, of their transpose, of W and of W^T BY NAME - looked up in the module's globals at every call (_fn), so that a replaced
# ops.quantize_* is the one that runs.
_Recipe = NamedTuple("_Recipe", [("mx", bool)] + [(f, str) for f in ("fwd", "dgrad", "wgrad", "rows", "cols", "weight", "weight_t")])
_RECIPES = {
    "row": _Recipe(False, "sv_linear_fp8", "sv_linear_fp8_dgrad", "sv_linear_fp8_wgrad",
                   "quantize_rows_fp8", "quantize_cols_fp8", "quantize_weight_fp8", "quantize_weight_t_fp8"),
    "mx": _Recipe(True, "sv_linear_mxfp8", "sv_linear_mxfp8_dgrad", "sv_linear_mxfp8_wgrad",
                  "quantize_rows_mx", "quantize_cols_mx", "quantize_weight_mx", "quantize_weight_t_mx"),
}


def _fn(name: str):
    return globals()[name]


class LinearPlan(NamedTuple):
    """How one Swin linear runs its forward and who quantises its input rows (swin_linear_plan)."""
    kind: Optional[str]          # None: the contraction engine; "row" / "mx": the fp8 kernel of that recipe
    epi: Optional[Epilogue]      # the sv_epilogue of the fp8 kernel (of `form`)
    form: dict                   # the epilogue keywords the plan was made with
    ln_emits: bool = False       # the LayerNorm in front emits the quantised rows (row: set_ln_quant_fused, MX: set_ln_quant_mx)
    prod_emits: bool = False     # the producer in front (window attention, fc1) emits the MX rows (set_mx_producer_quant)
    keep: bool = False           # the tape keeps the MX rows of the input in place of the tensor (store "mx")
    may_emit: bool = False       # as a producer this linear can emit the MX rows of its output


def swin_linear_plan(spec: ConvSpec, w, save, producer=None, **epi) -> LinearPlan:
    """The one evaluation of swin_linear_fp8_epilogue for a Swin linear with epilogue form **epi, asked BEFORE its input is produced.
    save: a backward will read this site's tape entry.  producer: None when a LayerNorm feeds the linear, True for the window attention, the
    LinearPlan of the linear in front (fc1 in front of fc2: it emits only if it takes the MX kernel itself, carries no residual and has
    N % 128 == 0).  ln_quant_site / ln_quant_mx_site / mx_emit_site / mx_store_site are these conditions under their historical names.
    With set_linear_fp8 off this is one flag test."""
    e = swin_linear_fp8_epilogue(spec, w, **epi)
    if e is None:
        return LinearPlan(None, None, epi)
    kind = linear_fp8_recipe()
    return LinearPlan(kind, e, epi,
                      ln_emits=producer is None and (ln_quant_fused_enabled() or ln_quant_mx_enabled()),
                      prod_emits=producer is not None and mx_producer_quant_enabled() and (producer is True or producer.may_emit),
                      keep=bool(save) and linear_fp8_store() == "mx" and _fp8_bwd_site(spec, w),
                      may_emit=kind == "mx" and spec.cout % 128 == 0 and epi.get("residual") is None)


def swin_linear_fwd(x, rows, spec: ConvSpec, w, out, xq=None, emit=False, plan: Optional[LinearPlan] = None, **epi):
    """linear_fwd of the Swin call sites: with set_linear_fp8(True) (and a form sv_linear_fp8 serves) the activation rows are quantised, the
    quantised weight fetched and the product runs on the fp8 kernel; otherwise exactly linear_fwd.  plan: this site's swin_linear_plan, when
    the caller made it already; **epi then holds only the keywords that were not known at that time (pre_act).  xq = (bytes, scales): the rows
    of x already quantised by its producer (layernorm_quant_fwd; under recipe "mx" the MX pair of an emitting fc1 or window attention), which
    the caller obtained because the plan said this linear takes the fp8 kernel; the quantiser pass is skipped and x itself is not read (it may
    be None).  emit=True (recipe "mx" only, the plan of the consumer said prod_emits): the kernel also writes the MX rows of its stored
    output, returned as (bytes, scales); `out` may then be None: besides the rows only pre_act is written, when it is given (the library
    serves that form in front of an activation only: fc1)."""
    if plan is None:
        plan, epi = swin_linear_plan(spec, w, False, **epi), {}
    if emit and plan.kind != "mx":
        raise RuntimeError("swin_linear_fwd: emit=True was passed to a linear that does not take the MX kernel")
    if plan.kind is None:
        if xq is not None:
            raise RuntimeError("swin_linear_fwd: pre-quantised rows were passed to a linear that does not take the fp8 kernel")
        return linear_fwd(x, rows, spec, w, out, **plan.form, **epi)
    r = _RECIPES[plan.kind]
    e = _epilogue(spec.cout, **plan.form, **epi) if epi else plan.epi
    xq, xs = xq if xq is not None else _fn(r.rows)(x, rows, spec.cin)
    wq, ws = _fn(r.weight)(w)
    esz, emitted = (0 if out is None else out.element_size()), ()
    if r.mx:
        pre = epi.get("pre_act", plan.form.get("pre_act"))
        if out is None and pre is not None:
            esz = pre.element_size()                       # the form without out (store "mx"): pre_act is the tensor the call writes
        emitted = operand_buffers(rows, spec.cout, True, xq.device) if emit else (None, None)     # N % 128 == 0: no padding
    traced_call(r.fwd, 2.0 * rows * spec.cin * spec.cout, float(rows) * (xq.shape[1] + (esz + (1 if emit else 0)) * spec.cout) + wq.numel(),
                ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(out), rows, spec.cin, spec.cout, C.byref(e), *[ptr(t) for t in emitted],
                tag=f"M={rows} K={spec.cin} N={spec.cout}")
    return emitted if emit else None


def quantize_cols_fp8(t: torch.Tensor, rows: int, Cc: int, ld: Optional[int] = None, colsum: Optional[torch.Tensor] = None):
    """t [rows, Cc] (fp32 or bf16, row stride ld) -> (e4m3 bytes of the TRANSPOSE [Cc, roundup(rows, 128)], fp32 column scales [Cc]) by
    sv_quant_cols_e4m3; colsum (fp32 [Cc]) += the column sums of the unquantised values."""
    q, sc = operand_buffers(Cc, rows, False, t.device)
    call("sv_quant_cols_e4m3", ptr(t), _dtype_code(t), rows, Cc, ld or Cc, ptr(q), q.shape[1], ptr(sc), ptr(colsum))
    return q, sc


def quantize_weight_t_fp8(w: torch.Tensor):
    """Quantised rows of W^T for a Linear weight W [N, K] (one scale per column k of W): the operand of the fp8 data gradient."""
    return _weight_operand(w, "w8t", quantize_cols_fp8)


def quantize_cols_mx(t: torch.Tensor, rows: int, Cc: int, ld: Optional[int] = None, colsum: Optional[torch.Tensor] = None):
    """t [rows, Cc] (fp32 or bf16, row stride ld) -> (e4m3 bytes of the TRANSPOSE [Cc, roundup(rows, 128)], E8M0 block scales
    [Cc, roundup(rows, 128) / 32] uint8, a block = 32 consecutive rows of one column) by sv_quant_cols_mx_e4m3: one launch, t read once;
    colsum (fp32 [Cc]) += the column sums of the unquantised values."""
    q, sc = operand_buffers(Cc, rows, True, t.device)
    call("sv_quant_cols_mx_e4m3", ptr(t), _dtype_code(t), rows, Cc, ld or Cc, ptr(q), q.shape[1], ptr(sc), ptr(colsum))
    return q, sc


def quant_rows_cols_mx_launches() -> int:
    """sv_quant_rows_cols_mx_e4m3 launches of this process so far."""
    return int(hip.load().sv_quant_rows_cols_mx_launches())


def quantize_rows_cols_mx(t: torch.Tensor, rows: int, N: int, ld: Optional[int] = None, colsum: Optional[torch.Tensor] = None, rows_out: bool = True):
    """t [rows, N] (fp32 or bf16, row stride ld) -> ((dq, ds), (dyt, dys)) by sv_quant_rows_cols_mx_e4m3, one launch and one read of t: (dq, ds)
    equals quantize_rows_mx(t) and (dyt, dys) equals quantize_cols_mx(t), bit for bit; colsum (fp32 [N]) += the column sums of the unquantised
    values.  rows_out=False: the column form alone, (None, (dyt, dys))."""
    dq, ds = operand_buffers(rows, N, True, t.device) if rows_out else (None, None)
    q, sc = operand_buffers(N, rows, True, t.device)
    call("sv_quant_rows_cols_mx_e4m3", ptr(t), _dtype_code(t), rows, N, ld or N, ptr(dq), (N + 127) // 128 * 128, ptr(ds), ptr(q), q.shape[1],
         ptr(sc), ptr(colsum))
    return ((dq, ds) if rows_out else None), (q, sc)


def set_mx_dual_quant(on: bool) -> None:
    """A/B switch of the MX dual quantiser (csrc/linear_fp8.hip, sv_quant_rows_cols_mx_e4m3): True lets swin_linear_wgrad quantise dy ONCE, on the
    caller's stream, into the column operand of the weight gradient and the row operand the data gradient of the same site takes from a one-slot
    stash, and gives the column operand of a stored bf16 x the same loader; False (default) keeps the row and the column quantiser, with
    bit-identical data and weight gradients.  Effective only under backward_recipe "mx" with bf16 math; SV_MX_DUAL_QUANT=1 in the environment
    switches it on as well."""
    _STATE["mx_dual_quant"] = bool(on)
    _CTX.dyq = None


def mx_dual_quant_enabled() -> bool:
    return linear_fp8_bwd_enabled() and linear_fp8_bwd_recipe() == "mx" and _switch("mx_dual_quant", "SV_MX_DUAL_QUANT", False)


def quantize_weight_t_mx(w: torch.Tensor):
    """MX rows of W^T for a Linear weight W [N, K] ([K][Np] bytes, a block = 32 consecutive n of one column k): the operand of the MX data
    gradient."""
    return _weight_operand(w, "w8mxt", quantize_cols_mx)


def _fp8_bwd_site(spec: ConvSpec, w) -> bool:
    return (linear_fp8_bwd_enabled() and spec.taps == 1 and spec.cin_mem == spec.cin and spec.cout_mem == spec.cout
            and isinstance(w, torch.nn.Parameter))


def _fp8_dgrad_epilogue(spec: ConvSpec, **epi):
    """The sv_epilogue of the fp8 data gradient of an _fp8_bwd_site, None when the library does not serve the form."""
    e = _epilogue(spec.cin, **epi)
    return e if hip.load().sv_linear_fp8_dgrad_supported(spec.cout, spec.cin, C.byref(e), _STATE["math"], hip.ACT) == 1 else None


def swin_linear_dgrad(dy, rows, spec: ConvSpec, w, dx, **epi):
    """linear_dgrad of the unfused Swin call sites (w is the PARAMETER): with set_linear_fp8(True, backward=True) (and a form
    sv_linear_fp8_dgrad serves) dy is quantised per row, the quantised W^T fetched and the product runs on the fp8 kernel; otherwise exactly
    linear_dgrad on the data-gradient weight pack.  Under the MX recipe the rows of dy come from the stash of the dual quantiser when it holds
    this very tensor (set_mx_dual_quant, swin_linear_wgrad); the slot is emptied by the look either way."""
    e = _fp8_dgrad_epilogue(spec, **epi) if _fp8_bwd_site(spec, w) else None
    if e is None:
        return linear_dgrad(dy, rows, spec, spec.pack_dgrad(w), dx, **epi)
    r = _RECIPES[linear_fp8_bwd_recipe()]
    if r.mx:
        st, _CTX.dyq = _CTX.dyq, None                      # the dual quantiser's rows of this very dy (swin_linear_wgrad), taken once
        if st is not None and st[0] is dy and st[1] == rows and st[2] == spec.cout:
            dq, ds = st[3], st[4]
        else:
            dq, ds = quantize_rows_mx(dy, rows, spec.cout, activation=False)
    else:
        dq, ds = quantize_rows_fp8(dy, rows, spec.cout)
    wtq, wts = _fn(r.weight_t)(w)
    traced_call(r.dgrad, 2.0 * rows * spec.cin * spec.cout, float(rows) * (dq.shape[1] + dy.element_size() * spec.cin) + wtq.numel(),
                ptr(dq), ptr(ds), ptr(wtq), ptr(wts), ptr(dx), rows, spec.cout, spec.cin, C.byref(e), tag=f"M={rows} N={spec.cout} K={spec.cin}")


def swin_linear_wgrad(dy, x, rows, spec: ConvSpec, w, dw, db=None, async_ok=True):
    """linear_wgrad of the unfused Swin call sites (w is the PARAMETER dw belongs to): with set_linear_fp8(True, backward=True) dy and x are
    quantised per column into transposed e4m3 copies (db from the unquantised dy in the same pass) and the product over the tokens runs on
    the fp8 kernel; otherwise exactly linear_wgrad.  The whole sequence follows linear_wgrad's stream rule: on the weight-gradient stream
    (temporaries allocated inside that stream context) unless async_ok is False, in which case it stays in order on the caller's stream (the
    quantised copies are complete before the caller overwrites dy).  The transposed copies, rows x (N + K) bytes, are freed on return either
    way; only dy and x are held until the join.  backward_recipe "mx": the same sequence on the MX column quantiser and sv_linear_mxfp8_wgrad,
    whose workspace of fp32 partials is one more temporary of that stream context.
    x = (bytes, scales): the MX rows of x that the tape kept in place of the tensor (store "mx", the caller asked mx_store_site): the
    re-blocker (mx_rows_to_cols) takes the place of the column quantiser of x, and the pair's tensors are what is held until the join.
    set_mx_dual_quant(True) at an MX site: dy is quantised ONCE, on the caller's stream and before anything else (quantize_rows_cols_mx with
    colsum=db): the column pair feeds the GEMM on the weight-gradient stream (recorded on that stream, not held until the join), the row pair
    waits in the one-slot stash _CTX.dyq for the swin_linear_dgrad of the same dy, which every call site issues next; it is emitted only when
    that data gradient (the site's plain form) takes the MX kernel.  A stored bf16 x goes through the same kernel's column-only form.  The slot
    is cleared here on entry, by AsyncWgrad.join() and by set_async_wgrad()."""
    pair = isinstance(x, tuple)
    _CTX.dyq = None
    site, r = _fp8_bwd_site(spec, w), _RECIPES[linear_fp8_bwd_recipe()]
    if pair and not (site and r.mx):
        raise RuntimeError("swin_linear_wgrad: stored MX rows were passed to a linear whose weight gradient does not take the MX kernel")
    if not site:
        return linear_wgrad(dy, x, rows, spec, dw, db, async_ok=async_ok)

    dual = r.mx and mx_dual_quant_enabled()
    dcols = None
    if dual:                                               # dy is read once, on the caller's stream: db, the column pair, and the row pair
        rows_out = _fp8_dgrad_epilogue(spec) is not None   # when the data gradient of this site (its plain form) takes the MX kernel
        drows, dcols = quantize_rows_cols_mx(dy, rows, spec.cout, colsum=db, rows_out=rows_out)
        if rows_out:
            _CTX.dyq = (dy, rows, spec.cout) + drows

    def run():
        dyt, dys = dcols if dual else _fn(r.cols)(dy, rows, spec.cout, colsum=db)
        if pair:
            xt, xs = mx_rows_to_cols(x[0], x[1], rows, spec.cin)
        elif dual:
            xt, xs = quantize_rows_cols_mx(x, rows, spec.cin, rows_out=False)[1]
        else:
            xt, xs = _fn(r.cols)(x, rows, spec.cin)
        nws, ws = 0, ()
        if r.mx:
            nws = int(hip.load().sv_linear_mxfp8_wgrad_workspace_floats(rows, spec.cout, spec.cin, 0))
            ws = (fempty(nws, like=dw) if nws else None,)  # the splits' fp32 partials: written before they are read, dropped once enqueued
        traced_call(r.wgrad, 2.0 * rows * spec.cin * spec.cout, float(dyt.numel() + xt.numel()) + 8.0 * spec.cin * spec.cout + 8.0 * nws,
                    ptr(dyt), ptr(dys), ptr(xt), ptr(xs), ptr(dw), rows, spec.cout, spec.cin, spec.cin, 0, *[ptr(t) for t in ws],
                    tag=f"M={rows} N={spec.cout} K={spec.cin}")

    # run()'s temporaries are allocated on the weight-gradient stream and dropped there: its allocator recycles them in stream order
    if run_on_wgrad_stream((dy,) + x if pair else (dy, x), run, enable=async_ok) and dual:
        for t in dcols:    # the column pair of dy was allocated on the caller's stream and is read on that one: not held, recorded
            t.record_stream(_CTX.awg.stream)


def linear_dgrad(dy, rows, spec: ConvSpec, w_t, dx, **epi):
    spec.dgrad(dy, rows, (1, 1, 1), w_t, dx, **epi)


def linear_wgrad(dy, x, rows, spec: ConvSpec, dw, db=None, async_ok=True):
    spec.wgrad(dy, x, rows, (1, 1, 1), dw, db=db, async_ok=async_ok)


# ---------------------------------------------------------------------------------------------------
# normalisation wrappers
# ---------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, rows, Cdim, merge_hw=(0, 0), eps=1e-5):
    y = empty(rows, Cdim, like=x)
    mean = fempty(rows, like=x)
    rstd = fempty(rows, like=x)
    call("sv_layernorm_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), rows, Cdim, eps, merge_hw[0], merge_hw[1])
    return y, mean, rstd


def set_ln_quant_fused(on: bool) -> None:
    """A/B switch of the quantising LayerNorm (csrc/norm.hip, sv_layernorm_quant_fwd): True (default) lets norm1 / norm2 / the patch-merge
    norm emit the e4m3 rows and scales of the fp8 linear they feed; False keeps LayerNorm + the stand-alone row quantiser.  Effective only
    while linear_fp8_enabled(); SV_LN_QUANT_FUSED=0 in the environment switches it off as well."""
    _STATE["ln_quant_fused"] = bool(on)


def ln_quant_fused_enabled() -> bool:
    # recipe "mx": this form writes per-row scales; the MX form has a switch of its own (ln_quant_mx_enabled)
    return linear_fp8_enabled() and linear_fp8_recipe() == "row" and _switch("ln_quant_fused", "SV_LN_QUANT_FUSED", True)


def ln_quant_site(spec: ConvSpec, w, **epi) -> bool:
    """Whether the LayerNorm in front of this Swin linear takes the quantising form: the linear will run on the fp8 kernel and the fused
    quantiser is on (LinearPlan.ln_emits under the row recipe).  With set_linear_fp8 off this is one flag test."""
    return ln_quant_fused_enabled() and swin_linear_plan(spec, w, False, **epi).ln_emits


def layernorm_quant_launches() -> int:
    """sv_layernorm_quant_fwd launches of this process so far."""
    return int(hip.load().sv_layernorm_quant_launches())


def layernorm_quant_fwd(x, gamma, beta, rows, Cdim, merge_hw=(0, 0), eps=1e-5, store=True):
    """layernorm_fwd that also returns the operand rows of the fp8 linear it feeds: (y, mean, rstd, xq, sx) with xq [rows, roundup(Cdim, 128)]
    e4m3 bytes and sx [rows] fp32 scales, equal to quantize_rows_fp8(y).  store=False (no backward follows): y, mean and rstd are neither
    allocated nor written and come back as None."""
    return _layernorm_quant(False, x, gamma, beta, rows, Cdim, merge_hw, eps, store, True)


def _layernorm_quant(mx, x, gamma, beta, rows, Cdim, merge_hw, eps, store, store_y):
    y = mean = rstd = None
    if store:
        y = empty(rows, Cdim, like=x) if store_y else None
        mean = fempty(rows, like=x)
        rstd = fempty(rows, like=x)
    xq, sx = operand_buffers(rows, Cdim, mx, x.device)
    call("sv_layernorm_quant_mx_fwd" if mx else "sv_layernorm_quant_fwd", ptr(x), ptr(gamma), ptr(beta), ptr(y), ptr(mean), ptr(rstd), ptr(xq),
         xq.shape[1], ptr(sx), rows, Cdim, eps, merge_hw[0], merge_hw[1])
    return y, mean, rstd, xq, sx


def set_ln_quant_mx(on: bool) -> None:
    """A/B switch of the MX quantising LayerNorm (csrc/norm.hip, sv_layernorm_quant_mx_fwd): True lets norm1 / norm2 / the patch-merge norm
    emit the MX rows and E8M0 block scales of the MXFP8 linear they feed; False (default) keeps LayerNorm + the stand-alone MX quantiser, with
    bit-identical results.  Effective only under recipe "mx" with bf16 math; SV_LN_QUANT_MX=1 in the environment switches it on as well.
    Independent of set_mx_producer_quant (the proj / fc2 sites) and of set_ln_quant_fused (the row recipe)."""
    _STATE["ln_quant_mx"] = bool(on)


def ln_quant_mx_enabled() -> bool:
    return _mx() and _switch("ln_quant_mx", "SV_LN_QUANT_MX", False)


def ln_quant_mx_site(spec: ConvSpec, w, **epi) -> bool:
    """MX counterpart of ln_quant_site: the linear behind this LayerNorm will run on the MX kernel and the MX quantising LayerNorm is on
    (LinearPlan.ln_emits under recipe "mx").  With set_linear_fp8 off this is one flag test."""
    return ln_quant_mx_enabled() and swin_linear_plan(spec, w, False, **epi).ln_emits


def layernorm_quant_mx_launches() -> int:
    """sv_layernorm_quant_mx_fwd launches of this process so far (layernorm_quant_launches() counts none of them)."""
    return int(hip.load().sv_layernorm_quant_mx_launches())


def layernorm_quant_mx_fwd(x, gamma, beta, rows, Cdim, merge_hw=(0, 0), eps=1e-5, store=True, store_y=True):
    """layernorm_fwd that also returns the MX operand rows of the MXFP8 linear it feeds: (y, mean, rstd, xq, xs) with xq [rows,
    roundup(Cdim, 128)] e4m3 bytes and xs [rows, roundup(Cdim, 128) / 32] E8M0 bytes, equal to quantize_rows_mx(y) (which is not launched:
    mx_act_quant_launches() does not move).  store=False (no backward follows): y, mean and rstd are neither allocated nor written and come
    back as None.  store_y=False (the tape keeps the MX rows, store "mx"): the statistics are kept for layernorm_bwd, y is neither allocated
    nor written."""
    return _layernorm_quant(True, x, gamma, beta, rows, Cdim, merge_hw, eps, store, store_y)


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, Cdim, merge_hw=(0, 0), accumulate_dx=False):
    ws = zeros_f64(LN_BWD_SLOTS * Cdim + 1, dy.device)     # sv_layernorm_bwd_workspace_floats(C) floats, zero on entry
    call("sv_layernorm_bwd", ptr(dy), ptr(x), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), rows, Cdim,
         merge_hw[0], merge_hw[1], 1 if accumulate_dx else 0)


class BatchNormState:
    """Per-call state of one BatchNorm layer on channels-last [M, C] data."""

    def __init__(self, bn: torch.nn.Module, M: int, training: bool):
        self.bn, self.M, self.training, self.C = bn, M, training, bn.num_features
        dev = bn.weight.device
        self.sums = zeros_f64(BN_SLOTS * 2 * self.C, dev) if training else None   # [slot][2C] doubles
        buf = fempty(4 * self.C, device=dev)
        self.scale, self.shift, self.mean, self.rstd = buf[:self.C], buf[self.C:2 * self.C], buf[2 * self.C:3 * self.C], buf[3 * self.C:]

    def finalize(self):
        bn = self.bn
        if self.training and bn.num_batches_tracked is not None:
            if _CTX.bn_tick is None:
                _CTX.bn_tick = []
            _CTX.bn_tick.append(bn.num_batches_tracked)   # += 1 in one foreach launch (bn_tick_flush)
        mom = bn.momentum if bn.momentum is not None else 0.1
        call("sv_bn_finalize", ptr(self.sums), self.M, ptr(bn.weight), ptr(bn.bias), ptr(bn.running_mean), ptr(bn.running_var),
             float(mom), float(bn.eps), 1 if self.training else 0, ptr(self.scale), ptr(self.shift), ptr(self.mean), ptr(self.rstd), self.C)

    def probe(self, x, ldx):
        probe = _STATE.get("bn_probe")
        if probe is not None:        # debug hook (tests): the producer's statistics next to the output it stored
            probe(self, x, ldx)

    def apply(self, x, ldx, y, ldy, act=ACT_NONE, slope=0.0, residual=None, ldr=0):
        self.probe(x, ldx)
        self.signs = None
        if (residual is not None and act != ACT_NONE and self.training and _bn_signs_on() and self.C % 256 == 0
                and self.C % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and ldr % 4 == 0):
            # BatchNorm in front of a residual sum: the backward's activation mask as sign words (1/16 of the output's bytes) - see backward()
            self.signs = torch.empty(self.M * (self.C // 64), dtype=torch.int64, device=x.device)
            call("sv_scale_shift_act_signs", ptr(x), ldx, ptr(self.scale), ptr(self.shift), ptr(residual), ldr, ptr(y), ldy, self.M, self.C, act, slope,
                 ptr(self.signs))
            return
        call("sv_scale_shift_act", ptr(x), ldx, ptr(self.scale), ptr(self.shift), ptr(residual), ldr, ptr(y), ldy, self.M, self.C, act, slope)

    def backward(self, dz, lddz, z, ldz, x, ldx, dx, lddx, dgamma, dbeta, act=ACT_NONE, slope=0.0, dres=None, lddres=0):
        ws = bn_bwd_workspace(self.C, dz.device)
        if getattr(self, "signs", None) is not None and dres is not None:
            # mask from the forward's sign words: the reduce pass reads (dz, x, words) and stores the masked gradient in dres, the apply pass
            # reads (dres, x): 6 passes over the tensor instead of the 8 of (dz, z, x) + (dz, z, x, dx, dres)
            call("sv_bn_bwd_signs", ptr(dz), lddz, ptr(self.signs), ptr(x), ldx, ptr(self.bn.weight), ptr(self.mean), ptr(self.rstd), self.M, self.C,
                 act, slope, 1 if self.training else 0, ptr(dx), lddx, ptr(dres), lddres, ptr(dgamma), ptr(dbeta), ptr(ws))
            return
        # z = None: the forward added no residual, so the activation mask is recomputed from x (one tensor read less per pass)
        call("sv_bn_bwd", ptr(dz), lddz, ptr(z), ldz, ptr(x), ldx, ptr(self.bn.weight), ptr(self.mean), ptr(self.rstd), self.M, self.C,
             act, slope, 1 if self.training else 0, ptr(dx), lddx, ptr(dres), lddres, ptr(dgamma), ptr(dbeta), ptr(ws),
             ptr(self.scale), ptr(self.shift))


def bn_dual_enabled(training: bool, C: int, act: int) -> bool:
    """bn3 and the down-sampling BatchNorm of a layer's first bottleneck in the same passes (bn_dual_apply / bn_dual_backward): the
    switch (set_bn_dual / SV_BN_DUAL, default on) and what the kernels need - train mode, ReLU, sign words in use, C % 256 == 0."""
    on = _STATE.get("bn_dual", os.environ.get("SV_BN_DUAL", "1") != "0")
    return bool(on and training and act == ACT_RELU and _bn_signs_on() and C % 256 == 0)


def set_bn_dual(on: bool) -> None:
    """A/B switch: False runs the two BatchNorms of a down-sampling bottleneck as two layers (sv_scale_shift_act + sv_scale_shift_act_signs,
    sv_bn_bwd_signs + sv_bn_bwd)."""
    _STATE["bn_dual"] = bool(on)


def bn_dual_apply(st3: "BatchNormState", x3, ldx3, std: "BatchNormState", xd, ldxd, y, ldy) -> None:
    """y = relu(bn3(x3) + bn_d(xd)) in one pass, both layers finalized before; st3 keeps the sign words of the sum"""
    std.probe(xd, ldxd)
    st3.probe(x3, ldx3)
    st3.signs = torch.empty(st3.M * (st3.C // 64), dtype=torch.int64, device=x3.device)
    call("sv_scale_shift_act2_signs", ptr(x3), ldx3, ptr(st3.scale), ptr(st3.shift), ptr(xd), ldxd, ptr(std.scale), ptr(std.shift), ptr(y), ldy,
         st3.M, st3.C, ptr(st3.signs))


def bn_dual_backward(st3: "BatchNormState", std: "BatchNormState", dz, lddz, x3, ldx3, xd, ldxd, dx3, lddx3, dxd, lddxd, grads) -> None:
    """both layers' input gradients from dz and st3's sign words; grads[...] of the four BatchNorm parameters +="""
    ws = bn_bwd_workspace(st3.C, dz.device, layers=2)
    call("sv_bn_bwd2_signs", ptr(dz), lddz, ptr(st3.signs), ptr(x3), ldx3, ptr(st3.bn.weight), ptr(st3.mean), ptr(st3.rstd),
         ptr(xd), ldxd, ptr(std.bn.weight), ptr(std.mean), ptr(std.rstd), st3.M, st3.C, ptr(dx3), lddx3, ptr(dxd), lddxd,
         ptr(grads[st3.bn.weight]), ptr(grads[st3.bn.bias]), ptr(grads[std.bn.weight]), ptr(grads[std.bn.bias]), ptr(ws[0]), ptr(ws[1]))


def _bn_signs_on() -> bool:
    return _STATE.get("bn_signs", os.environ.get("SV_BN_SIGNS", "1") != "0")


def set_bn_signs(on: bool) -> None:
    """A/B switch: False keeps the stored output as the activation mask of the BatchNorms in front of a residual sum."""
    _STATE["bn_signs"] = bool(on)


def input_prep_enabled() -> bool:
    return _STATE.get("input_prep", os.environ.get("SV_INPUT_PREP", "1") != "0")


def set_input_prep(on: bool) -> None:
    """A/B switch of the encoder's input: True (default) = sv_encoder_prep (renderings -> stem space-to-depth image + Swin patch rows in one
    pass, patch embedding as a Linear(48, C)), False = cast + NCHW -> NHWC transpose + sv_stem_space_to_depth + the 4 x 4 / stride-4 convolution."""
    _STATE["input_prep"] = bool(on)


def bn_pool_fused_enabled() -> bool:
    return _STATE.get("bn_pool_fused", os.environ.get("SV_BN_POOL_FUSED", "1") != "0")


def set_bn_pool_fused(on: bool) -> None:
    """A/B switch of the BatchNorm -> activation -> max-pool chains (ResNet stem, the Refiner's three down-sampling layers): True (default) =
    one forward pass and the pool's backward inside the BatchNorm backward (sv_bn_act_maxpool*_fwd / sv_bn_maxpool*_bwd: neither the
    activation nor its gradient is stored), False = the separate passes."""
    _STATE["bn_pool_fused"] = bool(on)


def set_conv_halo(mode: int) -> None:
    """Halo-tile kernels behind the contraction engine (csrc/conv_halo.hip: 3 x 3 / 64 -> 64 and the ResNet stem): 0 off, 1 calls of
    >= 256 tiles (default), 2 every call of those shapes.  Process-wide; the library reads SV_CONV_HALO for its initial mode."""
    rc = hip.load().sv_set_conv_halo(int(mode))
    if rc != 0:
        raise RuntimeError(f"sv_set_conv_halo failed (rc={rc}): {hip.load().sv_last_error().decode()}")


def set_conv_halo_wgrad(mode: int) -> None:
    """Halo-tile weight gradient of the 3 x 3 / stride-1 convolutions with 64 k channels (csrc/conv_halo.hip) behind sv_conv_wgrad: 0 off,
    1 from 4 tiles per split on (default), 2 always.  Process-wide; SV_CONV_HALO_WGRAD sets the initial mode."""
    rc = hip.load().sv_set_conv_halo_wgrad(int(mode))
    if rc != 0:
        raise RuntimeError(f"sv_set_conv_halo_wgrad failed (rc={rc}): {hip.load().sv_last_error().decode()}")


def set_bn_probe(fn) -> None:
    """Debug hook of the tests: fn(state, stored_output, ld) is called for every BatchNorm layer right before its normalisation pass,
    when `state.sums` (the [BN_SLOTS][2C] double partial sums the producing kernel's epilogue accumulated) and the producer's stored
    output are both complete on the current stream.  None removes it.  Process-wide configuration."""
    _STATE["bn_probe"] = fn


def transpose(src, dst, batch, R, Cc, lds=None, ldd=None, sb=None, db=None):
    """dst[b][c][r] = src[b][r][c]; element type taken from the tensors (activations in the storage dtype, parameters fp32)"""
    lds = lds or Cc
    ldd = ldd or R
    assert src.dtype == dst.dtype
    call("sv_transpose", ptr(src), ptr(dst), batch, R, Cc, lds, ldd, sb if sb is not None else R * lds, db if db is not None else Cc * ldd,
         act=hip.BF16 if src.dtype == torch.bfloat16 else hip.F32)
