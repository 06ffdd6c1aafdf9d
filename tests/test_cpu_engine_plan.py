"""Launch plans of the contraction engine (csrc/igemm.hip plan_gather / plan_wgrad behind sv_conv_gather_plan / sv_conv_wgrad_plan): which
kernel, tile, operand variant and grid a shape gets.  The queries are pure host functions - no GPU, fabricated 16-byte aligned addresses.
Every expected value below was worked out by hand from the dispatch code as it stood before the plans existed (thresholds quoted per case),
not read off the function under test."""
import ctypes as C

import pytest

from swinvox_amd import hip
from swinvox_amd.hip import Epilogue, Geom, LaunchPlan

X, W, Y, AUX = 0x10000, 0x20000, 0x30000, 0x40000      # "device pointers": only their alignment is looked at
BF, F32S = (hip.MATH_BF16, hip.BF16), (hip.MATH_BF16, hip.F32)
NARROW, DEFAULT, T96, BIG = (128, 16, 256), (128, 64, 512), (128, 96, 512), (128, 128, 512)     # tile rows, columns, threads


@pytest.fixture()
def lib():
    lib = hip.load()
    assert lib.sv_set_conv_halo(1) == 0 and lib.sv_set_conv_halo_wgrad(1) == 0
    yield lib
    lib.sv_set_conv_halo(1)
    lib.sv_set_conv_halo_wgrad(1)


def linear(M, K, Co):
    return Geom(M, 1, 1, 1, 1, 1, 1, K, Co, 1, 1, 1, 1, 1, 1, 0, 0, 0, K)


def conv2d(N, H, W_, Ci, Co, k, p):
    return Geom(N, 1, H, W_, 1, H, W_, Ci, Co, 1, k, k, 1, 1, 1, 0, p, p, Ci)


def epi(ldc, **kw):
    e = Epilogue(None, None, 0, None, 1, None, None, hip.ACT_NONE, 0.0, None, hip.ACT_NONE, ldc, 0)
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def gather(lib, g, e, x=X, mode=BF, transposed=0):
    q = LaunchPlan()
    assert lib.sv_conv_gather_plan(x, W, Y, C.byref(g), C.byref(e), mode[0], mode[1], transposed, C.byref(q)) == 0
    return q.path, (q.tile_rows, q.tile_cols, q.block), q.operands, q.vec, (q.grid_x, q.grid_y)


def wgrad(lib, g, lda, mode=BF):
    q = LaunchPlan()
    assert lib.sv_conv_wgrad_plan(X, lda, W, C.byref(g), g.Ci, mode[0], mode[1], C.byref(q)) == 0
    return q.path, (q.tile_rows, q.tile_cols, q.block), q.vec, (q.grid_x, q.grid_y)


def test_linear_paths(lib):
    M, K, Co = 33317, 384, 392
    g, e = linear(M, K, Co), epi(Co)
    is_wide = lambda g_, e_, x=X: lib.sv_conv_gather_is_wide(x, W, Y, C.byref(g_), C.byref(e_), *BF)
    # K % 64 == 0, K >= 192, Co >= 128, 8-aligned rows, ceil(M / 256) * ceil(Co / 128) = 131 * 4 = 524 >= 256 tiles: the wide kernel
    assert gather(lib, g, e) == (hip.PATH_WIDE, (256, 128, 768), hip.OPERANDS_BF16, 8, (256, 1)) and is_wide(g, e) == 1
    assert gather(lib, g, epi(Co, residual=AUX, ldr=Co))[0] == hip.PATH_WIDE_GENERAL
    # BatchNorm producers stay off the wide kernel below K = 1024, an activation-gradient source below K = 384, rows that are not 8-aligned
    # always: the dense kernel, on the 128 x 128 tile (Co > 64, ceil(M / 128) * ceil(Co / 128) = 261 * 4 = 1044 >= 384), 2 x 256 workgroups
    dense_big = (hip.PATH_DENSE, BIG, hip.OPERANDS_BF16, 8, (512, 1))
    assert gather(lib, g, epi(Co, stats=AUX)) == dense_big and is_wide(g, epi(Co, stats=AUX)) == 0
    assert gather(lib, linear(M, 1024, Co), epi(Co, stats=AUX))[0] == hip.PATH_WIDE
    assert gather(lib, linear(M, 192, Co), epi(Co, act_grad_src=AUX, act_grad_kind=hip.ACT_GELU)) == dense_big
    assert gather(lib, linear(M, 192, Co), epi(Co))[0] == hip.PATH_WIDE
    assert gather(lib, g, epi(396)) == dense_big and is_wide(g, epi(396)) == 0
    # gathered rows that do not start on 16 bytes, fp32 storage, fp32 math: the gathering kernel, 4-element operand loads, 261 * 4 tiles
    assert gather(lib, g, e, x=X + 8) == (hip.PATH_GATHER, BIG, hip.OPERANDS_BF16, 4, (1044, 1)) and is_wide(g, e, X + 8) == 0
    assert gather(lib, g, e, mode=F32S) == (hip.PATH_GATHER, BIG, hip.OPERANDS_BF16_F32, 4, (1044, 1))
    assert gather(lib, g, e, mode=(hip.MATH_F32, hip.F32)) == (hip.PATH_GATHER, BIG, hip.OPERANDS_F32, 4, (1044, 1))
    # M = 4096: 16 * 4 = 64 wide tiles < 256 and 32 * 4 = 128 tiles of 128 x 128 < 384: dense on 128 x 64, 32 * 7 = 224 tiles
    assert gather(lib, linear(4096, K, Co), e) == (hip.PATH_DENSE, DEFAULT, hip.OPERANDS_BF16, 8, (224, 1))
    # Co = 96: the 96-wide tile wins the estimate (2 waves of 128 x 96 against 4 of 128 x 64 and 2 of 128 x 128); 392 tiles
    assert gather(lib, linear(50176, 96, 96), epi(96)) == (hip.PATH_DENSE, T96, hip.OPERANDS_BF16, 8, (392, 1))
    assert gather(lib, linear(50176, 96, 96), epi(96, stats=AUX))[1] == BIG              # statistics never take it: 392 tiles of 128 x 128 >= 384
    # Co <= 16: the gathering kernel on the 16-column tile, also for a Linear
    assert gather(lib, linear(1000, 64, 8), epi(8)) == (hip.PATH_GATHER, NARROW, hip.OPERANDS_BF16, 8, (8, 1))


def test_halo_routes_and_modes(lib):
    halo = lambda path, th, tw, grid: (path, (th, tw, 256), hip.OPERANDS_BF16, 8, (grid, 1))
    g56, g14, e64 = conv2d(64, 56, 56, 64, 64, 3, 1), conv2d(1, 14, 14, 64, 64, 3, 1), epi(64)
    # 64 images of 56 x 56: 64 * 7 * 2 = 896 tiles of 8 x 32 >= 256
    assert gather(lib, g56, e64) == halo(hip.PATH_HALO0, 8, 32, 256)
    assert gather(lib, g56, epi(64, stats=AUX))[0] == hip.PATH_HALO0 and gather(lib, g56, epi(64, bias=AUX))[0] == hip.PATH_GATHER
    # one 14 x 14 image: 2 tiles - the engine under mode 1 (128 x 64 tile, 2 x 1 tiles), halo tiles under mode 2, never under mode 0
    small = (hip.PATH_GATHER, DEFAULT, hip.OPERANDS_BF16, 8, (2, 1))
    assert gather(lib, g14, e64) == small
    lib.sv_set_conv_halo(2)
    assert gather(lib, g14, e64) == halo(hip.PATH_HALO0, 8, 32, 256)
    lib.sv_set_conv_halo(0)
    assert gather(lib, g14, e64) == small and gather(lib, g56, e64)[0] == hip.PATH_GATHER
    lib.sv_set_conv_halo(1)
    # 128 -> 128 on 28 x 28: 8 x 32 and 16 x 16 tiles both cover 784 / 1024; 128 images = 128 * 4 * 2 = 1024 items >= 1024, 64 images = 512
    g128 = conv2d(128, 28, 28, 128, 128, 3, 1)
    assert gather(lib, g128, epi(128)) == halo(hip.PATH_HALO_BLOCKED_8X32, 8, 32, 256)
    assert gather(lib, conv2d(64, 28, 28, 128, 128, 3, 1), epi(128)) == (hip.PATH_GATHER, BIG, hip.OPERANDS_BF16, 8, (392, 1))
    assert gather(lib, conv2d(1024, 14, 14, 128, 128, 3, 1), epi(128)) == halo(hip.PATH_HALO_BLOCKED_16X16, 16, 16, 256)   # 196 / 256 against 196 / 512
    # its data gradient: halo tiles for a plain store, the engine with statistics (100352 rows: 784 tiles of 128 x 128)
    assert gather(lib, g128, epi(128), transposed=1)[0] == hip.PATH_HALO_BLOCKED_8X32
    assert gather(lib, g128, epi(128, stats=AUX), transposed=1) == (hip.PATH_GATHER, BIG, hip.OPERANDS_BF16, 8, (784, 1))
    assert gather(lib, g56, epi(64, stats=AUX), transposed=1)[0] == hip.PATH_GATHER
    # the 4 x 4 stem on the space-to-depth image (16 images of 112 x 112: 14 x 4 tiles each) and its 64 -> 16 data gradient (7 x 4 tiles of 16 x 32)
    assert gather(lib, conv2d(16, 112, 112, 16, 64, 4, 2), e64) == halo(hip.PATH_HALO1, 8, 32, 512)
    assert gather(lib, conv2d(16, 112, 112, 64, 16, 4, 2), epi(16), transposed=1) == halo(hip.PATH_HALO2, 16, 32, 256)
    assert gather(lib, conv2d(16, 112, 112, 64, 16, 4, 2), epi(16))[0] == hip.PATH_GATHER      # forward of that shape: no halo kernel


def test_transposed_gather_classes(lib):
    """stride-2 3 x 3 x 3 transposed gather 4^3 -> 7^3: 8 parity classes along grid y, the largest (4^3 outputs x 2 images = 128 rows) sets grid x"""
    g = Geom(2, 4, 4, 4, 7, 7, 7, 32, 32, 3, 3, 3, 2, 2, 2, 1, 1, 1, 32)
    assert gather(lib, g, epi(32), transposed=1) == (hip.PATH_GATHER, DEFAULT, hip.OPERANDS_BF16, 8, (1, 8))


def test_weight_gradient_paths(lib):
    is_wide = lambda g_, lda: lib.sv_conv_wgrad_is_wide(X, lda, W, C.byref(g_), g_.Ci, *BF)
    M = 64 * 331
    # K = 392, N = 264: the 256-side over Ci wastes less (512 x 384 against 512 x 512): 2 x 3 tiles, 256 / 6 = 42 workgroups per tile
    assert wgrad(lib, linear(M, 392, 264), 264) == (hip.PATH_WGRAD_WIDE_SWAP, (256, 128, 768), 8, (252, 1)) and is_wide(linear(M, 392, 264), 264) == 1
    assert wgrad(lib, linear(M, 384, 512), 512)[0] == hip.PATH_WGRAD_WIDE       # 512 x 384 against 512 x 512 the other way round
    # rows % 64 != 0: the tiled kernel, 3 x 4 tiles of 128 x 128, 512 / 12 = 42 splits of 512 rows
    assert wgrad(lib, linear(M - 56, 392, 264), 264) == (hip.PATH_WGRAD_TILED, (128, 128, 512), 8, (504, 1)) and is_wide(linear(M - 56, 392, 264), 264) == 0
    # 37 x 7 = 259 tiles of 256 x 128 > 256: always ran the tiled kernel (7 x 73 = 511 tiles, one split); the query now says so
    assert wgrad(lib, linear(16384, 9344, 896), 896) == (hip.PATH_WGRAD_TILED, (128, 128, 512), 8, (511, 1)) and is_wide(linear(16384, 9344, 896), 896) == 0
    assert is_wide(linear(16384, 4992, 1664), 1664) == 0 and is_wide(linear(16384, 4992, 1536), 1536) == 1      # 20 x 13 = 260 and 6 x 39 = 234 tiles
    assert wgrad(lib, linear(1000, 64, 8), 8) == (hip.PATH_WGRAD_TILED, (16, 128, 256), 8, (2, 1))              # Co <= 16
    assert wgrad(lib, conv2d(4, 14, 14, 32, 64, 3, 1), 64) == (hip.PATH_WGRAD_TILED, (64, 128, 512), 8, (6, 1))  # Co <= 64, 9 taps: 3 tiles x 2 splits
    assert wgrad(lib, linear(4096, 192, 96), 96) == (hip.PATH_WGRAD_TILED, (96, 128, 512), 8, (16, 1))          # Co = 96: 2 tiles x 8 splits
    assert wgrad(lib, linear(4096, 32, 128), 128) == (hip.PATH_WGRAD_TILED, (128, 64, 512), 8, (8, 1))          # 32 columns: the 64-wide tile
    assert wgrad(lib, linear(4096, 32, 128), 128, mode=F32S)[2] == 4
    # 3 x 3, 64 -> 64, 80 images.  56 x 56: 80 * 14 = 1120 tiles of 8 x 32 >= 4 per split (256 splits); 7 x 7: 19 % of a tile is image
    big, small = conv2d(80, 56, 56, 64, 64, 3, 1), conv2d(80, 7, 7, 64, 64, 3, 1)
    halo = (hip.PATH_WGRAD_HALO, (8, 32, 256), 8, (256, 1))
    tiled = lambda grid: (hip.PATH_WGRAD_TILED, (64, 128, 512), 8, (grid, 1))
    expect = {0: (tiled(505), tiled(40)), 1: (halo, tiled(40)), 2: (halo, halo)}       # 5 tiles x 101 splits of 2496 rows; 5 x 8 splits of 512
    for mode, (eb, es) in expect.items():
        lib.sv_set_conv_halo_wgrad(mode)
        assert wgrad(lib, big, 64) == eb and wgrad(lib, small, 64) == es, mode
    lib.sv_set_conv_halo_wgrad(1)
    assert wgrad(lib, conv2d(8, 56, 56, 64, 64, 3, 1), 64) == tiled(245)    # 8 images: 112 tiles < 4 * 256: tiled, 5 tiles x 49 splits of 512 rows


def test_refused_arguments(lib):
    q, g, e = LaunchPlan(), linear(64, 64, 64), epi(64)
    assert lib.sv_conv_gather_plan(X, W, Y, None, C.byref(e), *BF, 0, C.byref(q)) == -1
    assert lib.sv_conv_gather_plan(X, W, Y, C.byref(g), None, *BF, 0, C.byref(q)) == -1
    assert lib.sv_conv_gather_plan(X, W, Y, C.byref(g), C.byref(e), *BF, 0, None) == -1
    assert lib.sv_conv_gather_plan(X, W, Y, C.byref(g), C.byref(e), hip.MATH_F32, hip.BF16, 0, C.byref(q)) == -1     # bf16 storage needs bf16 math
    assert lib.sv_conv_gather_plan(X, W, Y, C.byref(Geom(1, 1, 2, 2, 1, 6, 6, 8, 8, 1, 3, 3, 1, 3, 3, 0, 0, 0, 8)), C.byref(epi(8)), *BF, 1, C.byref(q)) == -1
    assert lib.sv_conv_wgrad_plan(X, 64, W, None, 64, *BF, C.byref(q)) == -1 and lib.sv_conv_wgrad_plan(X, 8, W, C.byref(g), 64, *BF, C.byref(q)) == -1
    assert lib.sv_conv_gather_is_wide(X, W, Y, None, C.byref(e), *BF) == 0 and lib.sv_conv_wgrad_is_wide(X, 64, W, None, 64, *BF) == 0
