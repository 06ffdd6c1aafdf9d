"""The stand-alone BatchNorm passes (csrc/norm.hip: sv_bn_stats, sv_bn_finalize, sv_scale_shift_act(_signs), sv_bn_bwd(_signs)) through the C
ABI against the fp64 reference of tests/test_cpu_batchnorm_reference.py, on every launch path: the scalar, narrow and vector kernel families,
the four mask sources of the backward (stored z, sign words, recomputed from x, none), with and without dres, train and eval, equal and unequal
row strides, both storage modes.  Every output is judged element by element by bn_check: |got - ref| <= K 2^-24 bound (+ 2^-8 |ref| for a bf16
output).  Output buffers start as NaN, dgamma / dbeta from a non-zero value (the contract is +=), and every column or element outside a tensor
carries a sentinel that must come back bit-identical.

K (one constant, at most 256, kept in the recipe file) = 4 x the largest ratio |got - ref| / (2^-24 bound) that this file measured on an MI355X
with the check switched to recording, rounded up to a power of two.  The measured table (bf16 storage: after the 2^-8 |ref| term):

    output         fp32 storage   bf16 storage
    z                  3.55           0.61
    dres               1.20           0.00
    dx                15.50           1.18
    dgamma             2.33            -        (fp32 in both modes; the larger of the two runs is listed under fp32)
    dbeta              1.48            -
    mean               0.99            -
    rstd               1.68            -
    scale              2.37            -
    shift              2.90            -
    running_mean       2.21            -
    running_var        1.58            -

The largest, 15.5, is dx of the scalar family with the mask from z and LeakyReLU (M = 65, C = 18), so K = 64.  The first recording run had nine
cases between 4.6e3 and 4.7e4, all of them dx in bf16 storage with LeakyReLU and dres on the vector kernels (mask from z, recomputed, or sign
words): the apply pass read back the bf16-rounded masked gradient that the reduce pass had stored for dres, so dx carried 2^-9 |gamma rstd dz'|.
plan_bn_bwd hands the masked gradient over through dres only where the stored value is exact (ReLU, or fp32 storage).

Every apply and backward call first asks the plan query (sv_scale_shift_act_plan / sv_bn_bwd_plan) with the buffers it is about to pass: the
family must be the one the case names, and in the backward the mask hand-off the one its mask source, activation and storage imply.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_cpu_batchnorm_reference as R  # noqa: E402
from test_cpu_batchnorm_reference import ACT_LRELU, ACT_NONE, ACT_RELU, EPS, MOMENTUM, SLOPE  # noqa: E402

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -1234.5
STORES = ("f32", "bf16")
ACT_NAME = {ACT_NONE: "none", ACT_RELU: "relu", ACT_LRELU: "lrelu"}
FAMILY = {"scalar": hip.NORM_BN_SCALAR, "narrow": hip.NORM_BN_NARROW, "vec": hip.NORM_BN_VECTOR}


def _up4(c):
    return (c + 3) & ~3


class _storage:
    """ops.set_storage(mode) for the body, the defaults (fp32 math and storage) afterwards"""

    def __init__(self, store):
        self.store = store

    def __enter__(self):
        ops.set_math("bf16")
        ops.set_storage(self.store)
        return torch.bfloat16 if self.store == "bf16" else torch.float32

    def __exit__(self, *exc):
        ops.set_math("f32")
        return False


class Buf:
    """An [M, C] activation tensor as the kernels see it: rows of `ld` elements inside a flat allocation, the tensor in columns [off, off + C),
    `head` elements in front of row 0 (a misaligned view) and 8 behind the last row.  Everything that is not the tensor holds SENT.  wide: the
    narrow kernels own the whole 4-channel vectors, i.e. columns up to off + roundup4(C): NaN there on input (ignored), exact zeros on output."""

    def __init__(self, dev, dt, M, C, ld, off=0, head=0, data=None, wide=False):
        self.M, self.C, self.ld, self.off, self.head, self.w = M, C, ld, off, head, (_up4(C) if wide else C)
        assert ld >= off + self.w
        self.flat = torch.full((head + M * ld + 8,), SENT, dtype=dt, device=dev)
        self.rows = self.flat[head:head + M * ld].view(M, ld)
        self.rows[:, off:off + self.w] = float("nan")            # an output starts as NaN; the pad columns of a narrow input stay NaN
        if data is not None:
            self.rows[:, off:off + C] = data.to(dev).to(dt)
        self.before = self.flat.clone()
        self.ptr = self.rows.data_ptr() + off * self.flat.element_size()

    def _bits(self, t):
        return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)

    def value(self):
        return self.rows[:, self.off:self.off + self.C].to(torch.float64).cpu()

    def assert_unchanged(self, what):
        assert torch.equal(self._bits(self.flat), self._bits(self.before)), f"{what}: an input was written"

    def assert_outside_untouched(self, what):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        keep[self.head:self.head + self.M * self.ld].view(self.M, self.ld)[:, self.off:self.off + self.w] = False
        assert torch.equal(self._bits(self.flat)[keep], self._bits(self.before)[keep]), f"{what}: written outside the tensor"
        if self.w > self.C:
            assert bool((self.rows[:, self.off + self.C:self.off + self.w] == 0).all()), f"{what}: the pad columns must hold zeros"


def _f32(t, dev, n=None, fill=float("nan")):
    """fp32 parameter vector in a 16-byte aligned allocation of roundup4 elements; the slack keeps `fill`"""
    n = n or t.numel()
    b = torch.full((_up4(n) + 4,), fill, dtype=torch.float32, device=dev)
    b[:n] = t.to(torch.float32).to(dev)
    return b


def _check(name, store, case, got, key, ref=None, bound=None):
    ref_ = case["ref"][key] if ref is None else ref
    bound_ = case["ref"][R.BOUND_OF[key]] if bound is None else bound
    R.bn_check(f"{name}:{key}", got, ref_, bound_, R.K, stored_bf16=(store == "bf16" and key in R.STORED))


def _slack_intact(b, n, fill_nan=True):
    tail = b[n:]
    return bool(torch.isnan(tail).all()) if fill_nan else bool((tail == 0).all())


# ---- forward: statistics, finalize, apply ------------------------------------------------------------------------------------------------
def _fwd_layout(fam, C):
    """strides / offsets / alignment that select the family (bn_family in csrc/norm.hip; _forward asserts it through the plan query)"""
    if fam == "scalar":
        return {1: dict(ldx=1, ldy=1, ldr=1), 9: dict(ldx=9, ldy=9, ldr=9), 18: dict(ldx=20, ldy=20, ldr=20),
                8: dict(ldx=12, ldy=12, ldr=12, head=1)}[C]                    # C = 8 would be a vector shape: every view is off by one element
    if fam == "narrow":
        return {9: dict(ldx=12, ldy=48, offy=24, ldr=12),                       # the merger's concat: 9 channels into columns 24 .. 35 of 48
                1: dict(ldx=4, ldy=4, ldr=4), 2: dict(ldx=4, ldy=4, ldr=4), 13: dict(ldx=16, ldy=16, ldr=16)}[C]
    if C in (12, 40, 320):
        return dict(ldx=C + 4, ldy=C + 8, ldr=C + 12)                           # ldx != ldy != ldr
    return dict(ldx=C, ldy=C, ldr=C)


def _forward(dev, store, name, case, lay, wide, fam, training=True, signs=False):
    """sv_bn_stats -> sv_bn_finalize -> sv_scale_shift_act(_signs) on fresh buffers, after the plan query has named the family `fam` for them;
    checks every output and returns (y buffer, sign words)"""
    M, C, act, ref = case["M"], case["C"], case["act"], case["ref"]
    head = lay.get("head", 0)
    with _storage(store) as dt:
        x = Buf(dev, dt, M, C, lay["ldx"], head=head, data=case["x"], wide=wide)
        res = Buf(dev, dt, M, C, lay["ldr"], head=head, data=case["res"], wide=wide) if case["res"] is not None else None
        y = Buf(dev, dt, M, C, lay["ldy"], off=lay.get("offy", 0), head=head, wide=wide)
        gm, bt = _f32(case["gamma"], dev), _f32(case["beta"], dev)
        rm, rv = _f32(case["running_mean"], dev), _f32(case["running_var"], dev)
        rm0, rv0 = rm.clone(), rv.clone()
        sc, sh, mu, rs = (_f32(torch.full((C,), float("nan")), dev) for _ in range(4))
        sums = torch.zeros(ops.BN_SLOTS * 2 * C, dtype=torch.float64, device=dev)
        words = torch.full((M * (C // 64) + 2,), 0x5A5A5A5A, dtype=torch.int64, device=dev) if signs else None
        if training:
            call("sv_bn_stats", x.ptr, M, C, lay["ldx"], ptr(sums))
        call("sv_bn_finalize", ptr(sums) if training else None, M, ptr(gm), ptr(bt), ptr(rm), ptr(rv), MOMENTUM, EPS, 1 if training else 0,
             ptr(sc), ptr(sh), ptr(mu), ptr(rs), C)
        rptr, ldr = (res.ptr, lay["ldr"]) if res is not None else (None, 0)
        plan = hip.NormPlan()
        assert hip.load().sv_scale_shift_act_plan(x.ptr, lay["ldx"], ptr(sc), ptr(sh), rptr, ldr, y.ptr, lay["ldy"], M, C, act, SLOPE, ptr(words), hip.ACT,
                                                  ctypes.byref(plan)) == 0, f"{name}: {hip.load().sv_last_error().decode()}"
        assert plan.family == FAMILY[fam], f"{name}: the layout selects family {plan.family}, the case names {fam}"
        if signs:
            call("sv_scale_shift_act_signs", x.ptr, lay["ldx"], ptr(sc), ptr(sh), rptr, ldr, y.ptr, lay["ldy"], M, C, act, SLOPE, ptr(words))
        else:
            call("sv_scale_shift_act", x.ptr, lay["ldx"], ptr(sc), ptr(sh), rptr, ldr, y.ptr, lay["ldy"], M, C, act, SLOPE)
        torch.cuda.synchronize()
    if training:
        assert bool((sums[2 * C:] == 0).all()), f"{name}: sv_bn_stats wrote outside slot 0"
    x.assert_unchanged(name + ":x")
    if res is not None:
        res.assert_unchanged(name + ":res")
    y.assert_outside_untouched(name + ":z")
    for b in (sc, sh, mu, rs, rm, rv):
        assert _slack_intact(b, C), f"{name}: a parameter-sized output was written beyond C"
    _check(name, store, case, y.value(), "z")
    for key, b in (("mean", mu), ("rstd", rs), ("scale", sc), ("shift", sh), ("running_mean", rm), ("running_var", rv)):
        _check(name, store, case, b[:C], key)
    if not training:
        assert torch.equal(rm[:C], rm0[:C]) and torch.equal(rv[:C], rv0[:C]), f"{name}: eval mode changed the running statistics"
    return y, words


FWD_PARAMS = [pytest.param(fam, C, M, training, id=f"{fam}-C{C}-M{M}-{ACT_NAME[R.fwd_recipe(C, M)['act']]}-{'train' if training else 'eval'}")
              for fam, shapes in R.FWD_SHAPES.items() for C, M in shapes for training in ((True, False) if R.fwd_has_eval(M) else (True,))]


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fam,C,M,training", FWD_PARAMS)
def test_forward(dev, fam, C, M, training, store):
    r = R.fwd_recipe(C, M)
    case = R.bn_case(M, C, r["act"], r["with_res"], r["offset"], store == "bf16", 0, training)
    _forward(dev, store, f"fwd-{fam}-C{C}-M{M}-{store}", case, _fwd_layout(fam, C), wide=(fam == "narrow"), fam=fam, training=training)


@pytest.mark.parametrize("store", STORES)
def test_forward_constant_channel(dev, store):
    """variance 0: rstd = eps^-1/2, the channel's output is beta (+ res) whatever the constant; M == 1 is a shape of test_forward"""
    case = R.bn_case(*R.const_recipe(store == "bf16"))
    assert float(case["ref"]["var"][R.CONST_CHANNEL]) == 0.0
    _forward(dev, store, f"fwd-const-{store}", case, dict(ldx=12, ldy=12, ldr=12), wide=False, fam="vec")


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("act", [ACT_RELU, ACT_LRELU], ids=["relu", "lrelu"])
@pytest.mark.parametrize("C,M", R.SIGN_SHAPES)
def test_forward_sign_words(dev, C, M, act, store):
    """sv_scale_shift_act_signs: the words bit for bit in the header's layout, nothing behind them, and the output of the plain pass"""
    case = R.bn_case(*R.sign_recipe(C, M, act, store == "bf16"))
    lay = dict(ldx=C, ldy=C + 4, ldr=C)
    name = f"signs-C{C}-M{M}-{store}"
    y, words = _forward(dev, store, name, case, lay, wide=False, fam="vec", signs=True)
    y0, _ = _forward(dev, store, name + "-plain", case, lay, wide=False, fam="vec", signs=False)
    n = M * (C // 64)
    assert torch.equal(words[:n].cpu().view(M, C // 256, 4), R.sign_words(case["ref"]["p"])), f"{name}: sign words"
    assert bool((words[n:] == 0x5A5A5A5A).all()), f"{name}: written behind the sign words"
    assert torch.equal(y._bits(y.flat), y0._bits(y0.flat)), f"{name}: z differs from sv_scale_shift_act"


@pytest.mark.parametrize("store", STORES)
def test_finalize_sums_every_slot(dev, store):
    """sv_bn_stats over three disjoint row ranges into three slots of one [SV_BN_SLOTS][2C] buffer = one call over all rows, bit for bit"""
    M, C = 1031, 40
    r = R.fwd_recipe(C, M)
    case = R.bn_case(M, C, r["act"], r["with_res"], r["offset"], store == "bf16", 0, True)
    outs = []
    with _storage(store) as dt:
        x = Buf(dev, dt, M, C, C + 4, data=case["x"])
        gm, bt = _f32(case["gamma"], dev), _f32(case["beta"], dev)
        for parts in ([(0, M, 0)], [(0, 300, 0), (300, 301, 5), (301, M, ops.BN_SLOTS - 1)]):
            sums = torch.zeros(ops.BN_SLOTS * 2 * C, dtype=torch.float64, device=dev)
            for r0, r1, slot in parts:
                call("sv_bn_stats", x.rows[r0:].data_ptr(), r1 - r0, C, C + 4, sums[slot * 2 * C:].data_ptr())
            rm, rv = _f32(case["running_mean"], dev), _f32(case["running_var"], dev)
            o = [_f32(torch.full((C,), float("nan")), dev) for _ in range(4)]
            call("sv_bn_finalize", ptr(sums), M, ptr(gm), ptr(bt), ptr(rm), ptr(rv), MOMENTUM, EPS, 1, *(ptr(t) for t in o), C)
            torch.cuda.synchronize()
            outs.append(o + [rm, rv])
    for a, b in zip(*outs):
        assert torch.equal(a[:C], b[:C])
    for key, b in zip(("scale", "shift", "mean", "rstd", "running_mean", "running_var"), outs[1]):
        _check(f"slots-{store}", store, case, b[:C], key)


# ---- backward ----------------------------------------------------------------------------------------------------------------------------
BWD_LAYOUTS = {
    "scalar": dict(fam="scalar", lddz=19, ldz=20, ldx=20, lddx=18, lddres=21),
    "narrow": dict(fam="narrow", lddz=12, ldz=16, ldx=12, lddx=12, lddres=16, wide=True),
    "vec": dict(fam="vec", lddz=48, ldz=40, ldx=44, lddx=52, lddres=44),
    "vec256": dict(fam="vec", lddz=256, ldz=256, ldx=256, lddx=256, lddres=260),
    "narrow_wrap": dict(fam="narrow", lddz=12, ldz=12, ldx=12, lddx=12, lddres=12, wide=True),
    "merger12": dict(fam="narrow", lddz=48, offdz=24, ldz=48, ldx=12, lddx=12, lddres=12, wide=True),     # backward(dzk, 48, None, 0, y, 12, dy, 12, ...)
    "merger1": dict(fam="scalar", lddz=1, ldz=1, ldx=1, lddx=4, lddres=1),                   # backward(dwl, 1, None, 0, y6, 1, dy6, 4, ...)
    "fsc8": dict(fam="narrow", lddz=8, ldz=8, ldx=8, lddx=8, lddres=8, fsc_off=1),           # fwd_scale / fwd_shift 4 bytes off a 16-byte boundary
    "fsc24": dict(fam="scalar", lddz=24, ldz=24, ldx=24, lddx=24, lddres=24, fsc_off=1),
}


def _hand_off(fam, act, store, with_dres, words):
    """how the mask reaches the apply pass: through dres (premask) on the vector kernels wherever the stored masked gradient is exact (ReLU, or
    fp32 storage), from the sign words where they are given and it is not, else from the case's own mask source (z, recomputed, none)"""
    if fam == "vec" and with_dres and act != ACT_NONE and not (act == ACT_LRELU and store == "bf16"):
        return hip.MASK_PREMASK
    return hip.MASK_SIGN_APPLY if words is not None else hip.MASK_PLAIN


def _backward(dev, store, name, case, lay, mask, with_dres, words=None, null_fwd=False):
    """sv_bn_bwd / sv_bn_bwd_signs on buffers built from the reference's forward (z, mean, rstd, scale, shift as the kernels store them)"""
    M, C, act, ref, training = case["M"], case["C"], case["act"], case["ref"], case["training"]
    wide = lay.get("wide", False)
    with _storage(store) as dt:
        dz = Buf(dev, dt, M, C, lay["lddz"], off=lay.get("offdz", 0), data=case["dz"], wide=wide)
        x = Buf(dev, dt, M, C, lay["ldx"], data=case["x"], wide=wide)
        z = Buf(dev, dt, M, C, lay["ldz"], data=ref["z"], wide=wide) if mask == "z" else None
        dx = Buf(dev, dt, M, C, lay["lddx"], wide=wide)
        dres = Buf(dev, dt, M, C, lay["lddres"], wide=wide) if with_dres else None
        gm, mu, rs = _f32(case["gamma"], dev), _f32(ref["mean"], dev), _f32(ref["rstd"], dev)
        fo = lay.get("fsc_off", 0)
        fsc = fsh = None
        if mask == "recompute" or (mask == "none" and not null_fwd):
            fsc, fsh = (_f32(torch.cat([torch.zeros(fo, dtype=torch.float64), ref[k]]), dev)[fo:] for k in ("scale", "shift"))
        g0 = torch.where(torch.arange(C) % 2 == 0, 0.5, -0.25).to(torch.float64)      # dgamma / dbeta are accumulated into
        dg, db = _f32(g0, dev), _f32(-g0, dev)
        ws = torch.zeros(int(hip.load().sv_bn_bwd_workspace_doubles(C)), dtype=torch.float64, device=dev)
        dresp, lddres = (dres.ptr, lay["lddres"]) if dres is not None else (None, 0)
        wd = words.reshape(-1).to(dev) if words is not None else None
        plan = hip.NormPlan()
        assert hip.load().sv_bn_bwd_plan(dz.ptr, lay["lddz"], z.ptr if z is not None else None, lay["ldz"] if z is not None else 0, ptr(wd), x.ptr, lay["ldx"],
                                         ptr(gm), ptr(mu), ptr(rs), M, C, act, SLOPE, 1 if training else 0, dx.ptr, lay["lddx"], dresp, lddres, ptr(dg),
                                         ptr(db), ptr(ws), ptr(fsc), ptr(fsh), hip.ACT, ctypes.byref(plan)) == 0, f"{name}: {hip.load().sv_last_error().decode()}"
        assert plan.family == FAMILY[lay["fam"]], f"{name}: the layout selects family {plan.family}, the case names {lay['fam']}"
        assert plan.mask == _hand_off(lay["fam"], act, store, with_dres, words), f"{name}: mask hand-off {plan.mask}"
        if words is not None:
            call("sv_bn_bwd_signs", dz.ptr, lay["lddz"], ptr(wd), x.ptr, lay["ldx"], ptr(gm), ptr(mu), ptr(rs), M, C, act, SLOPE,
                 1 if training else 0, dx.ptr, lay["lddx"], dresp, lddres, ptr(dg), ptr(db), ptr(ws))
        else:
            call("sv_bn_bwd", dz.ptr, lay["lddz"], z.ptr if z is not None else None, lay["ldz"] if z is not None else 0, x.ptr, lay["ldx"],
                 ptr(gm), ptr(mu), ptr(rs), M, C, act, SLOPE, 1 if training else 0, dx.ptr, lay["lddx"], dresp, lddres, ptr(dg), ptr(db),
                 ptr(ws), ptr(fsc), ptr(fsh))
        torch.cuda.synchronize()
    for b, what in ((dz, "dz"), (x, "x"), (z, "z")):
        if b is not None:
            b.assert_unchanged(f"{name}:{what}")
    dx.assert_outside_untouched(name + ":dx")
    _check(name, store, case, dx.value(), "dx")
    if dres is not None:
        dres.assert_outside_untouched(name + ":dres")
        _check(name, store, case, dres.value(), "dres")
    assert _slack_intact(dg, C) and _slack_intact(db, C), f"{name}: dgamma / dbeta written beyond C"
    # += into g0: the fp32 sum of the start value and the (double) channel sum rounds at the magnitude of both
    _check(name, store, case, dg[:C], "dgamma", ref=ref["dgamma"] + g0, bound=ref["Bdgamma"] + g0.abs())
    _check(name, store, case, db[:C], "dbeta", ref=ref["dbeta"] - g0, bound=ref["Bdbeta"] + g0.abs())


def _bwd_params():
    out = []
    for fam in ("scalar", "narrow", "vec"):
        for mask, acts in (("z", (ACT_RELU, ACT_LRELU)), ("recompute", (ACT_RELU, ACT_LRELU)), ("none", (ACT_NONE,))):
            for act in acts:
                for with_dres in (True, False):
                    for training in (True, False):
                        out.append(pytest.param(fam, mask, act, with_dres, training,
                                                id=f"{fam}-mask_{mask}-{ACT_NAME[act]}-{'dres' if with_dres else 'nodres'}-{'train' if training else 'eval'}"))
    return out


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fam,mask,act,with_dres,training", _bwd_params())
def test_backward(dev, fam, mask, act, with_dres, training, store):
    """family x mask source x dres x mode, at unequal row strides; without an activation and without dres the forward scale / shift are NULL"""
    case = R.bn_case(*R.bwd_recipe(fam, act, mask, training, store == "bf16"))
    name = f"bwd-{fam}-{mask}-{ACT_NAME[act]}-{'dres' if with_dres else 'nodres'}-{'train' if training else 'eval'}-{store}"
    _backward(dev, store, name, case, BWD_LAYOUTS[fam], mask, with_dres, null_fwd=not with_dres)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("act,training", [(ACT_RELU, True), (ACT_LRELU, True), (ACT_RELU, False)], ids=["relu-train", "lrelu-train", "relu-eval"])
@pytest.mark.parametrize("C,M", R.SIGN_SHAPES)
def test_backward_sign_words(dev, C, M, act, training, store):
    """mask from the sign words (built on the host from the reference's p in the header's layout), masked gradient through dres"""
    case = R.bn_case(*R.sign_recipe(C, M, act, store == "bf16", training))
    lay = dict(fam="vec", lddz=C, ldz=C, ldx=C + 4, lddx=C, lddres=C + 8)
    _backward(dev, store, f"bwd-signs-C{C}-M{M}-{ACT_NAME[act]}-{'train' if training else 'eval'}-{store}", case, lay, "signs", True, words=R.sign_words(case["ref"]["p"]))


MODEL_PATTERNS = [
    ("merger12", "recompute", ACT_LRELU, False),       # dz: 12 of 48 columns at offset 24, x and dx in 12-wide rows of 9 channels
    ("merger1", "recompute", ACT_LRELU, False),        # one channel, dx into 4-wide rows whose three pad columns are not the kernel's
    ("vec256", "recompute", ACT_RELU, False),          # 129 row blocks over 16 reduce slots, an odd row left for the two-row loop's tail
    ("vec256", "z", ACT_LRELU, True),
    ("narrow_wrap", "recompute", ACT_LRELU, False),    # 17 workgroups of the narrow reduce over 16 slots
    ("narrow_wrap", "z", ACT_RELU, True),
    ("fsc8", "recompute", ACT_RELU, True),             # fwd_scale / fwd_shift off a 16-byte boundary: not the float4 loads of the vector reduce
    ("fsc24", "recompute", ACT_LRELU, False),          # (C = 8 lands on the narrow kernels, C = 24 on the scalar ones)
]


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("shape,mask,act,with_dres", [pytest.param(*p, id=f"{p[0]}-mask_{p[1]}-{ACT_NAME[p[2]]}-{'dres' if p[3] else 'nodres'}")
                                                      for p in MODEL_PATTERNS])
def test_backward_model_patterns(dev, shape, mask, act, with_dres, store):
    case = R.bn_case(*R.bwd_recipe(shape, act, mask, True, store == "bf16"))
    _backward(dev, store, f"bwd-{shape}-{mask}-{ACT_NAME[act]}-{store}", case, BWD_LAYOUTS[shape], mask, with_dres)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_sign_word_refusals(dev):
    """raised on the host, before any launch: the outputs keep their NaN"""
    M = 5
    with _storage("f32") as dt:
        def bufs(C):
            t = {k: Buf(dev, dt, M, C, C, data=torch.ones(M, C)) for k in ("dz", "x")}
            t.update({k: Buf(dev, dt, M, C, C) for k in ("dx", "dres", "y")})
            t.update(p=_f32(torch.ones(C), dev), dg=_f32(torch.zeros(C), dev), words=torch.zeros(M * (C // 64) + 4, dtype=torch.int64, device=dev),
                     ws=torch.zeros(int(hip.load().sv_bn_bwd_workspace_doubles(C)), dtype=torch.float64, device=dev))
            return t

        def bwd(t, C, act, dres):
            call("sv_bn_bwd_signs", t["dz"].ptr, C, ptr(t["words"]), t["x"].ptr, C, ptr(t["p"]), ptr(t["p"]), ptr(t["p"]), M, C, act, SLOPE, 1,
                 t["dx"].ptr, C, t["dres"].ptr if dres else None, C if dres else 0, ptr(t["dg"]), ptr(t["dg"]), ptr(t["ws"]))

        for C, act, dres in ((256, ACT_RELU, False), (256, ACT_NONE, True), (192, ACT_RELU, True)):
            t = bufs(C)
            with pytest.raises(RuntimeError):
                bwd(t, C, act, dres)
            torch.cuda.synchronize()
            assert bool(torch.isnan(t["dx"].rows).all()) and bool(torch.isnan(t["dres"].rows).all()) and bool((t["dg"][:C] == 0).all())
        t = bufs(192)
        with pytest.raises(RuntimeError):
            call("sv_scale_shift_act_signs", t["x"].ptr, 192, ptr(t["p"]), ptr(t["p"]), None, 0, t["y"].ptr, 192, M, 192, ACT_RELU, SLOPE,
                 ptr(t["words"]))
        torch.cuda.synchronize()
        assert bool(torch.isnan(t["y"].rows).all()) and bool((t["words"] == 0).all())
