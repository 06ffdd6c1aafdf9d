"""Launch plans of the normalisation passes (csrc/norm.hip ln_plan / plan_scale_shift_act / plan_bn_bwd behind sv_layernorm_plan,
sv_scale_shift_act_plan and sv_bn_bwd_plan): kernel family, access width, lanes and grids of a call.  The queries are pure host functions -
no GPU, fabricated addresses of which only NULL-ness and alignment are looked at.  Every expected value below was worked out by hand from
the dispatch code as it stood before the plans existed (thresholds quoted per case), not read off the function under test."""
import ctypes as C

import pytest

from swinvox_amd import hip
from swinvox_amd.hip import NormPlan

X, Y, DX, RES, P0, P1, P2, P3, WORDS, WS = (0x10000 * i for i in range(1, 11))      # "device pointers", all 16-byte aligned
ROWS = 130


@pytest.fixture(scope="module")
def lib():
    return hip.load()


def err(lib):
    return lib.sv_last_error().decode()


def ln(lib, kind, C_, rows=ROWS, dt=hip.BF16, a=X, b=Y, c=DX, merge=(0, 0)):
    q = NormPlan()
    assert lib.sv_layernorm_plan(kind, a, b, c, rows, C_, merge[0], merge[1], dt, C.byref(q)) == 0, err(lib)
    return q


def ln_geometry(q):
    return q.merge, q.storage, q.vec, q.lanes, q.nv, q.rows[0], q.grids()


def test_layernorm_forward(lib):
    """VEC 8: bf16 storage, C % 8 == 0, (merged: (C / 4) % 8 == 0), x and y on 16 bytes.  chunks = C / VEC: <= 16 -> 16 lanes per row, <= 32
    -> 32, else 64; NV = ceil(chunks / lanes) rounded up to one of 1, 2, 3, 4, 6, 12; a workgroup holds 4 waves of 64 / lanes rows each."""
    fwd = lambda *a, **k: ln_geometry(ln(lib, hip.LN_PLAIN, *a, **k))
    assert fwd(96) == (0, hip.BF16, 8, 16, 1, 16, [(9, 1)])                     # 12 chunks; 16 rows per workgroup; ceil(130 / 16) = 9
    assert fwd(192) == (0, hip.BF16, 8, 32, 1, 8, [(17, 1)])                    # 24 chunks; ceil(130 / 8) = 17
    assert fwd(384) == (0, hip.BF16, 8, 64, 1, 4, [(33, 1)])                    # 48 chunks; ceil(130 / 4) = 33
    assert fwd(3072) == (0, hip.BF16, 8, 64, 6, 4, [(33, 1)])                   # 384 chunks / 64 lanes = 6
    assert fwd(3072, dt=hip.F32) == (0, hip.F32, 4, 64, 12, 4, [(33, 1)])       # fp32 storage: 768 chunks / 64 lanes = 12
    assert fwd(100) == (0, hip.BF16, 4, 32, 1, 8, [(17, 1)])                    # 100 % 8 != 0: 25 chunks of 4
    assert fwd(96, b=Y + 8) == (0, hip.BF16, 4, 32, 1, 8, [(17, 1)])            # y 8 bytes off a 16-byte boundary: 24 chunks of 4
    assert fwd(96, a=X + 8)[2] == 4 and fwd(96, dt=hip.F32)[2] == 4
    assert fwd(96, merge=(8, 8)) == (1, hip.BF16, 8, 16, 1, 16, [(9, 1)])       # C0 = 24: 24 % 8 == 0
    assert fwd(80, merge=(8, 8)) == (1, hip.BF16, 4, 32, 1, 8, [(17, 1)])       # C0 = 20: (C / 4) % 8 != 0 although C % 8 == 0; 20 chunks
    for args in (dict(C_=96), dict(C_=3072), dict(C_=100), dict(C_=96, b=Y + 8), dict(C_=80, merge=(8, 8)), dict(C_=3072, dt=hip.F32)):
        plain = ln(lib, hip.LN_PLAIN, **args)
        assert plain.family == hip.NORM_LN_FWD and plain.launches == 1 and plain.launch[0].block == 256 and plain.launch[0].lds_bytes == 0
        for kind in (hip.LN_QUANT, hip.LN_QUANT_MX):                             # the quantising forms: the same geometry
            assert ln_geometry(ln(lib, kind, **args)) == ln_geometry(plain)
    assert ln(lib, hip.LN_QUANT, 96, b=None).vec == 8                            # y may be NULL there: nothing to be misaligned


def test_layernorm_backward(lib):
    """rows per workgroup = rows / 1024 clamped to [rows per iteration, 256], rounded up to whole iterations (16 rows at 16 lanes per row);
    2 C floats of LDS; the fold launch covers 2 C columns with 256 threads each"""
    q = ln(lib, hip.LN_BWD, 96)
    assert (q.family, q.launches) == (hip.NORM_LN_BWD, 2) and ln_geometry(q) == (0, hip.BF16, 8, 16, 1, 16, [(9, 1), (1, 1)])   # 130 / 1024 = 0 -> 16
    q = ln(lib, hip.LN_BWD, 96, rows=200000)
    assert ln_geometry(q) == (0, hip.BF16, 8, 16, 1, 208, [(962, 1), (1, 1)])     # 195 -> 13 iterations of 16; ceil(200000 / 208) = 962
    assert (q.launch[0].lds_bytes, q.launch[1].lds_bytes, q.launch[0].block, q.launch[1].block) == (768, 0, 256, 256)
    assert ln(lib, hip.LN_BWD, 96, c=DX + 8).vec == 4 and ln(lib, hip.LN_BWD, 96, rows=10 ** 6).rows[0] == 256     # dx misaligned; 976 -> 256
    assert ln(lib, hip.LN_BWD, 384, rows=200000).grids() == [(1021, 1), (3, 1)]  # 4 rows per iteration: 195 -> 196; 768 columns / 256


def test_layernorm_refusals(lib):
    q = NormPlan()
    plan = lambda kind, a, b, c, rows, C_, mh, mw, dt: lib.sv_layernorm_plan(kind, a, b, c, rows, C_, mh, mw, dt, C.byref(q))
    assert plan(hip.LN_PLAIN, X, Y, None, ROWS, 98, 0, 0, hip.BF16) == -1 and err(lib) == "layernorm_fwd: C=98 must be a multiple of 4 and <= 3072"
    assert plan(hip.LN_QUANT, X, Y, None, ROWS, 3076, 0, 0, hip.BF16) == -1 and err(lib).startswith("sv_layernorm_quant_fwd: C=3076")
    assert plan(hip.LN_QUANT_MX, None, Y, None, ROWS, 96, 0, 0, hip.BF16) == -1 and err(lib) == "sv_layernorm_quant_mx_fwd: null/empty argument"
    assert plan(hip.LN_PLAIN, X, Y, None, ROWS, 96, 0, 0, 7) == -1 and err(lib) == "layernorm_fwd: bad activation dtype 7"
    assert plan(hip.LN_PLAIN, X, Y, None, ROWS, 72, 8, 8, hip.BF16) == -1 and err(lib) == "layernorm_fwd(merge): H,W must be even and C a multiple of 16"
    assert plan(hip.LN_BWD, X, Y, DX, 0, 96, 0, 0, hip.BF16) == -1 and err(lib) == "layernorm_bwd: null/empty argument"
    assert plan(hip.LN_BWD, X, Y, None, ROWS, 96, 0, 0, hip.BF16) == -1 and plan(hip.LN_BWD, X, Y, DX, ROWS, 98, 0, 0, hip.BF16) == -1
    assert err(lib) == "layernorm_bwd: C=98 unsupported"
    assert plan(4, X, Y, DX, ROWS, 96, 0, 0, hip.BF16) == -1 and lib.sv_layernorm_plan(0, X, Y, None, ROWS, 96, 0, 0, hip.BF16, None) == -1


def apply_plan(lib, M, C_, ldx, ldy, y=Y, x=X, res=None, ldr=0, signs=None, dt=hip.F32, scale=P0, shift=P1, rc=0):
    q = NormPlan()
    assert lib.sv_scale_shift_act_plan(x, ldx, scale, shift, res, ldr, y, ldy, M, C_, hip.ACT_RELU, 0.0, signs, dt, C.byref(q)) == rc, err(lib)
    return q


def test_scale_shift_act(lib):
    """vector: C % 4 == 0, every row stride % 4 == 0, tensors on 4 elements, scale / shift on 16 bytes.  narrow: not vector, C <= 16, strides
    % 4 == 0 and >= roundup4(C), tensors on 4 elements.  scalar: the rest."""
    q = apply_plan(lib, 65, 18, 20, 20)                                          # C % 4 != 0 and C > 16; ceil(65 * 18 / 256) = 5 workgroups (<= 8192)
    assert (q.family, q.vec, q.grids(), q.launch[0].block) == (hip.NORM_BN_SCALAR, 1, [(5, 1)], 256)
    q = apply_plan(lib, 65, 9, 12, 48, y=Y + 24 * 4)                             # the merger's concat: columns 24 .. 35 of 48; ceil(65 / 64) = 2
    assert (q.family, q.vec, q.grids()) == (hip.NORM_BN_NARROW, 4, [(2, 1)])
    q = apply_plan(lib, 1000, 256, 256, 256)                                     # G = min(64, C / 4) = 64 lanes, 4 rows per step, 1 column group;
    assert (q.family, q.vec, q.lanes, q.rows[1], q.grids()) == (hip.NORM_BN_VECTOR, 4, 64, 16, [(1, 63)])     # 4096 splits capped at ceil(1000 / 16) = 63 -> 16 rows
    assert apply_plan(lib, 1000, 1024, 1024, 1024).grids() == [(4, 63)] and apply_plan(lib, 1000, 40, 40, 48).lanes == 10
    # what moves a call between the families
    assert apply_plan(lib, 65, 8, 12, 12).family == hip.NORM_BN_VECTOR and apply_plan(lib, 65, 8, 12, 12, x=X + 4).family == hip.NORM_BN_SCALAR
    assert apply_plan(lib, 65, 8, 12, 12, x=X + 8).family == hip.NORM_BN_SCALAR and apply_plan(lib, 65, 8, 12, 12, x=X + 8, dt=hip.BF16).family == hip.NORM_BN_VECTOR
    assert apply_plan(lib, 65, 8, 12, 12, shift=P1 + 4).family == hip.NORM_BN_NARROW                            # shift not a float4: narrow while C <= 16
    assert apply_plan(lib, 65, 24, 24, 24, shift=P1 + 4).family == hip.NORM_BN_SCALAR
    assert apply_plan(lib, 65, 9, 12, 12, res=RES, ldr=12).family == hip.NORM_BN_NARROW
    assert apply_plan(lib, 65, 9, 12, 12, res=RES, ldr=9).family == hip.NORM_BN_SCALAR
    assert apply_plan(lib, 65, 9, 12, 12, res=None, ldr=9).family == hip.NORM_BN_NARROW                         # no residual: its stride is not looked at
    assert apply_plan(lib, 17000, 9, 12, 12).grids() == [(266, 1)] and apply_plan(lib, 10 ** 7, 18, 20, 20).grids() == [(8192, 1)]
    # sign words: the vector family with C % 256 == 0
    assert apply_plan(lib, 1000, 256, 256, 260, signs=WORDS).grids() == [(1, 63)]
    apply_plan(lib, 1000, 128, 128, 128, signs=WORDS, rc=-1)
    assert err(lib) == "scale_shift_act_signs: needs C % 256 == 0 and 4-aligned rows (C=128)"
    apply_plan(lib, 1000, 256, 256, 256, signs=WORDS + 8, rc=-1)
    apply_plan(lib, 0, 256, 256, 256, rc=-1)
    assert err(lib) == "scale_shift_act: bad arguments"


def bwd_plan(lib, M, C_, ld, act=hip.ACT_RELU, z=None, signs=None, dres=None, dt=hip.F32, fwd=(P2, P3), dz=X, rc=0, lddz=None):
    q = NormPlan()
    ldz, lddres = (ld if z else 0), (ld if dres else 0)
    assert lib.sv_bn_bwd_plan(dz, lddz or ld, z, ldz, signs, Y, ld, P0, P0, P1, M, C_, act, 0.01, 1, DX, ld, dres, lddres, P0, P1, WS, fwd[0], fwd[1], dt,
                              C.byref(q)) == rc, err(lib)
    return q


def test_bn_bwd_families(lib):
    """reduce, fold (2 C columns, 256 per workgroup), apply (the forward's grid)"""
    q = bwd_plan(lib, 65, 18, 20)           # scalar: 32 channel lanes (next power of two of 18), 8 row lanes x 4 rows per step = 32: ceil(65 / 32) = 3 splits
    assert (q.family, q.lanes, q.rows[0], q.grids(), q.mask) == (hip.NORM_BN_SCALAR, 32, 22, [(1, 3), (1, 1), (5, 1)], hip.MASK_PLAIN)     # of ceil(65 / 3) = 22 rows
    q = bwd_plan(lib, 65, 9, 12)            # narrow: 64 row lanes x 16 rows per thread = 1024 rows per workgroup
    assert (q.family, q.rows[0], q.grids(), q.mask) == (hip.NORM_BN_NARROW, 16, [(1, 1), (1, 1), (2, 1)], hip.MASK_PLAIN)
    assert bwd_plan(lib, 17000, 9, 12).grids() == [(17, 1), (1, 1), (266, 1)]
    q = bwd_plan(lib, 1000, 256, 256)       # vector: 2 rows x 4 row lanes per step: 2048 splits capped at ceil(1000 / 8) = 125 of 8 rows; apply: 63 of 16
    assert (q.family, q.lanes, q.rows[0], q.rows[1], q.grids()) == (hip.NORM_BN_VECTOR, 64, 8, 16, [(1, 125), (2, 1), (1, 63)])
    assert all(l.block == 256 and l.lds_bytes == 0 for l in q.launch) and q.launches == 3
    assert bwd_plan(lib, 65, 8, 8, fwd=(P2, P3 + 4)).family == hip.NORM_BN_NARROW and bwd_plan(lib, 65, 24, 24, fwd=(P2 + 4, P3 + 4)).family == hip.NORM_BN_SCALAR
    assert bwd_plan(lib, 1031, 9, 12, dz=X + 24 * 4, lddz=48).family == hip.NORM_BN_NARROW and bwd_plan(lib, 1031, 1, 1).family == hip.NORM_BN_SCALAR
    assert bwd_plan(lib, 65, 8, 8, z=RES).family == hip.NORM_BN_VECTOR and bwd_plan(lib, 65, 8, 8, z=RES + 4).family == hip.NORM_BN_SCALAR


def test_bn_bwd_mask_hand_off(lib):
    """premask: dres wanted, an activation, and the stored masked gradient exact (ReLU, or fp32 storage); sign_apply: sign words without premask"""
    v = lambda **k: bwd_plan(lib, 1000, 256, 256, **k).mask
    assert v(dres=RES, act=hip.ACT_RELU) == hip.MASK_PREMASK and v(dres=RES, act=hip.ACT_RELU, dt=hip.BF16) == hip.MASK_PREMASK
    assert v(dres=RES, act=hip.ACT_LRELU, dt=hip.BF16) == hip.MASK_PLAIN and v(dres=RES, act=hip.ACT_LRELU, dt=hip.BF16, z=P2) == hip.MASK_PLAIN
    assert v(dres=RES, act=hip.ACT_LRELU, dt=hip.BF16, signs=WORDS, fwd=(None, None)) == hip.MASK_SIGN_APPLY
    assert v(dres=RES, act=hip.ACT_LRELU, dt=hip.F32) == hip.MASK_PREMASK and v(dres=RES, act=hip.ACT_LRELU, signs=WORDS, fwd=(None, None)) == hip.MASK_PREMASK
    assert v(dres=RES, act=hip.ACT_RELU, dt=hip.BF16, signs=WORDS, fwd=(None, None)) == hip.MASK_PREMASK
    assert v(act=hip.ACT_RELU) == hip.MASK_PLAIN and v(act=hip.ACT_LRELU, dt=hip.BF16) == hip.MASK_PLAIN and v(dres=RES, act=hip.ACT_NONE) == hip.MASK_PLAIN
    assert bwd_plan(lib, 65, 9, 12, dres=RES).mask == hip.MASK_PLAIN and bwd_plan(lib, 65, 18, 20, dres=RES).mask == hip.MASK_PLAIN     # a vector-family feature
    assert bwd_plan(lib, 1000, 256, 256, dres=RES, signs=WORDS, fwd=(None, None)).grids() == [(1, 125), (2, 1), (1, 63)]


def test_bn_bwd_refusals(lib):
    bwd_plan(lib, 1000, 256, 256, signs=WORDS, fwd=(None, None), rc=-1)          # sign words without dres
    assert err(lib) == "bn_bwd_signs: needs C % 256 == 0, 4-aligned rows, an activation and the residual-branch output dres (C=256)"
    bwd_plan(lib, 1000, 256, 256, signs=WORDS, dres=RES, act=hip.ACT_NONE, rc=-1)
    bwd_plan(lib, 1000, 192, 192, signs=WORDS, dres=RES, rc=-1)
    assert err(lib).endswith("(C=192)")
    bwd_plan(lib, 1000, 256, 256, fwd=(None, None), rc=-1)
    assert err(lib) == "bn_bwd: the activation mask needs the forward output z, its sign words or the forward scale/shift"
    bwd_plan(lib, 0, 256, 256, rc=-1)
    assert err(lib) == "bn_bwd: null/empty argument"
    assert lib.sv_bn_bwd_plan(X, 8, None, 0, None, Y, 8, P0, P0, P1, 65, 8, hip.ACT_NONE, 0.0, 1, DX, 8, None, 0, P0, P1, WS, None, None, hip.F32, None) == -1
