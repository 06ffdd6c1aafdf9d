"""The merger's stencil forward / data gradient (csrc/stencil.hip, stencil3_fwd_kernel<G, NT, AT, VEC>, both storages) and its weight packs
(sv_merger_pack) against torch conv3d and its autograd in float64 on bf16-rounded operands.  Launch paths -> instantiation (the `vec`
expression of sv_stencil3_fwd decides VEC): fwd_9x9, dgrad_9x9, dgrad_9x9_inplace, dgrad_1x9_ld4 = G1 NT1 vec; fwd_9x1_scalar (ldc 1, the
product's layer 6), fwd_9x9_ld9 = G1 NT1 scalar; fwd_36x9_rows48, fwd_36x9_planes = G3 NT1 vec; fwd_36x9_scalar (ldc 9) = G3 NT1 scalar;
dgrad_9x36_planes, dgrad_9x36_rows48 = G1 NT3 vec; dgrad_9x36_scalar (ldc 37) = G1 NT3 scalar.  Grids: 8x8x8 x 1 (one brick: every halo
face outside the volume), 16x8x24 x 2 (interior faces on every axis, unequal extents, 12 bricks: the identity branch of the XCD remap) and
32^3 x 9: 576 bricks, more than the 512 workgroups that __launch_bounds__(512, 2) lets stay resident on 256 CUs, so some workgroups take
two bricks through the prefetch path and some take one - 8 images (512 bricks) would still give every workgroup exactly one.  All twelve
rows run on all three grids (no test takes more than about a second: the float64 references are computed once per channel pair and grid);
`brick` and `faces` run them once in the table's row widths and once with four spare columns per row (room4), `multi` in the table's
widths.  Every case fills `out` with a sentinel first: columns outside the window must keep it, pad columns of the vectorised path must be
exactly zero (or the residual's pad value)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from swinvox_amd import hip, ops  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

F32_BOUND = 2e-5          # test_gpu_ops.py::test_stencil3_fwd_dgrad_wgrad's bound for this kernel
BF16_ULP = 2.0 ** -8      # one bf16 ulp of the stored value
STAT_BOUND = 1e-5
SENT = 7.25               # exact in bf16
GUARD = 64                # sentinel elements in front of and behind every output buffer
XGUARD = 1 << 16          # NaN elements in front of and behind every input buffer
GRIDS = {"brick": (1, 8, 8, 8), "faces": (2, 16, 8, 24), "multi": (9, 32, 32, 32)}
CAT = torch.tensor([12 * k + j for k in range(4) for j in range(9)])      # concat map col(ci) = 12 (ci // 9) + ci % 9
PATHS = {   # id -> (cin, cout, instantiation the call must select: G, NT, VEC)
    "fwd_9x9": (9, 9, (1, 1, True)), "fwd_9x1_scalar": (9, 1, (1, 1, False)), "fwd_9x9_ld9": (9, 9, (1, 1, False)),
    "fwd_36x9_rows48": (36, 9, (3, 1, True)), "fwd_36x9_planes": (36, 9, (3, 1, True)), "fwd_36x9_scalar": (36, 9, (3, 1, False)),
    "dgrad_9x9": (9, 9, (1, 1, True)), "dgrad_9x9_inplace": (9, 9, (1, 1, True)), "dgrad_1x9_ld4": (9, 1, (1, 1, True)),
    "dgrad_9x36_planes": (36, 9, (1, 3, True)), "dgrad_9x36_rows48": (36, 9, (1, 3, True)), "dgrad_9x36_scalar": (36, 9, (1, 3, False)),
}
STORES = {"f32": (torch.float32, hip.F32), "bf16": (torch.bfloat16, hip.BF16)}


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def cl(x):      # NC... -> N...C contiguous
    n = x.dim()
    return x.permute(0, *range(2, n), 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference(cin, cout, grid):
    """float64 conv3d and its autograd data gradient on bf16-rounded operands, as [M][channels] matrices; computed once per case, never modified."""
    n, D, H, W = GRIDS[grid]
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + list(GRIDS).index(grid))
    bf = lambda t: t.bfloat16().double()
    x = bf(torch.randn(n, cin, D, H, W, generator=g)).requires_grad_(True)
    w = bf(torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(27 * cin))
    b = torch.randn(cout, generator=g)
    dy = bf(torch.randn(n, cout, D, H, W, generator=g))
    y = F.conv3d(x, w, b.double(), padding=1)
    dx, = torch.autograd.grad(y, x, dy)
    M = n * D * H * W
    return dict(M=M, x=cl(x.detach()).reshape(M, cin).float(), w=w.float(), b=b, y=cl(y.detach()).reshape(M, cout),
                dy=cl(dy).reshape(M, cout).float(), dx=cl(dx).reshape(M, cin))


def pack_fwd(w, cols, G):
    """forward pack [16][27][16 G]: wp[co][tap][col(ci)] = w[co][ci][tap]"""
    cout, cin = w.shape[:2]
    p = torch.zeros(16, 27, 16 * G)
    p[:cout][:, :, cols] = w.reshape(cout, cin, 27).permute(0, 2, 1)
    return p


def pack_dgrad(w, rows, NT):
    """data-gradient pack [16 NT][27][16]: wp[row(ci)][26 - tap][co] = w[co][ci][tap]"""
    cout, cin = w.shape[:2]
    p = torch.zeros(16 * NT, 27, 16)
    p[rows, :, :cout] = w.reshape(cout, cin, 27).flip(2).permute(1, 2, 0)
    return p


def rows(m, width, cols=None):
    out = torch.zeros(m.shape[0], width)
    out[:, torch.arange(m.shape[1]) if cols is None else cols] = m
    return out


def planes(m48):    # [M][48] -> [4][M][12]
    return m48.view(m48.shape[0], 4, 12).permute(1, 0, 2).contiguous()


def case(path, grid, room=0, nan_tail=0, pack=None, **over):
    """One sv_stencil3_fwd call: operands in the kernel's memory layout (CPU), the arguments, and what must come back.  room: spare
    columns behind the table's row width; nan_tail: NaN columns appended to the input rows at and beyond cin_load; over: argument overrides."""
    cin, cout, inst = PATHS[path]
    r = reference(cin, cout, grid)
    M = r["M"]
    c = dict(path=path, grid=grid, M=M, groups=1, nt=1, x_plane=0, planar=False, col_off=0, bias=None, stats=False, res=None, ldr=0)
    if path.startswith("fwd"):
        c.update(bias=r["b"], stats=True, exp=r["y"], cout=cout, real=torch.arange(cout), ldc={"fwd_9x1_scalar": 1, "fwd_9x9_ld9": 9, "fwd_36x9_scalar": 9}.get(path, 12))
        if cin == 36:
            c.update(groups=3, pack=pack_fwd(r["w"], CAT, 3), cin_load=48, x=rows(r["x"], 48, CAT), ldx=48)
            if path == "fwd_36x9_planes":
                c.update(x=planes(c["x"]), ldx=12, x_plane=M * 12)
        else:
            c.update(pack=pack_fwd(r["w"], torch.arange(9), 1), cin_load=12, x=rows(r["x"], 12), ldx=12)
    else:
        c.update(exp=r["dx"], x=rows(r["dy"], 12), ldx=12, cin_load=12)
        if path == "dgrad_1x9_ld4":      # layer 6: one real channel and three zero columns
            c.update(x=rows(r["dy"], 4), ldx=4, cin_load=4)
        if cin == 36:
            c.update(nt=3, pack=pack_dgrad(r["w"], CAT, 3), cout=48, real=CAT, ldc=48)
            if path == "dgrad_9x36_planes":
                c.update(planar=True, ldc=12)
            elif path == "dgrad_9x36_rows48":
                c.update(res="inplace")
            elif path == "dgrad_9x36_scalar":   # rows = the 36 dense input channels
                c.update(pack=pack_dgrad(r["w"], torch.arange(36), 3), cout=36, real=torch.arange(36), ldc=37)
        else:
            c.update(pack=pack_dgrad(r["w"], torch.arange(9), 1), cout=9, real=torch.arange(9), ldc=12, res="inplace" if path == "dgrad_9x9_inplace" else None)
    if not c["planar"]:
        c["ldc"] += room
    if nan_tail:
        c.update(x=torch.cat([c["x"], torch.full((M, nan_tail), float("nan"))], 1), ldx=c["ldx"] + nan_tail)
    if pack is not None:
        c["pack"] = pack
    c.update(over)
    if c["res"] == "inplace":
        c["ldr"] = c["ldc"]
    cs4 = (c["cout"] + 3) & ~3
    # the `vec` expression of sv_stencil3_fwd
    c["vec"] = c["planar"] or (c["ldc"] % 4 == 0 and c["col_off"] % 4 == 0 and c["col_off"] + cs4 <= c["ldc"] and (c["res"] is None or (c["ldr"] % 4 == 0 and cs4 <= c["ldr"])))
    c["inst"] = (c["groups"], c["nt"], c["vec"])
    c["width"] = cs4 if c["vec"] else c["cout"]        # columns of a row the call may write
    if c["res"]:
        g = torch.Generator().manual_seed(5)
        c["base"] = torch.randn(M, c["width"], generator=g).bfloat16().float()
    return c


def launch(dev, store, c):
    """Runs the call into a sentinel-filled buffer with guard elements on both sides; returns (whole buffer, out view, statistics)."""
    dt, act = STORES[store]
    n, D, H, W = GRIDS[c["grid"]]
    M, ldc, col_off, width = c["M"], c["ldc"], c["col_off"], c["width"]
    xbuf = torch.full((2 * XGUARD + c["x"].numel(),), float("nan"), dtype=dt, device=dev)   # a read outside the input comes back as NaN
    xd = xbuf[XGUARD:XGUARD + c["x"].numel()].view(c["x"].shape)
    xd.copy_(c["x"])
    wd = c["pack"].to(dev).bfloat16().contiguous()
    bd = c["bias"].to(dev) if c["bias"] is not None else None
    nel = 4 * M * 12 if c["planar"] else M * ldc
    buf = torch.full((GUARD + nel + GUARD,), SENT, dtype=dt, device=dev)
    out = buf[GUARD:GUARD + nel].view(4, M, 12) if c["planar"] else buf[GUARD:GUARD + nel].view(M, ldc)
    resd, rptr = None, None
    if c["res"] == "inplace":          # residual[pos * ldr + n] is out's own window
        out[:, col_off:col_off + width] = c["base"].to(dev, dt)
        rptr = out.data_ptr() + col_off * out.element_size()
    elif c["res"] == "own":            # its own buffer; what lies beyond the window's columns must never be read
        resd = torch.full((M, c["ldr"]), float("nan"), dtype=dt, device=dev)
        resd[:, :width] = c["base"].to(dev, dt)
        rptr = ptr(resd)
    stats = torch.zeros(ops.BN_SLOTS, 2 * c["cout"], dtype=torch.float64, device=dev) if c["stats"] else None
    call("sv_stencil3_fwd", ptr(xd), c["ldx"], c["cin_load"], c["groups"], ptr(wd), c["nt"], ptr(bd), ptr(out), ldc, col_off, c["cout"], rptr, c["ldr"],
         ptr(stats), n, D, H, W, c["x_plane"], M * 12 if c["planar"] else 0, act=act)
    torch.cuda.synchronize()
    return buf, out, stats


def check(c, store, buf, out, stats):
    """Window / padding contract, values and statistics of one call; prints the measured errors."""
    M, col_off, width, real = c["M"], c["col_off"], c["width"], c["real"]
    assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), "wrote outside the output buffer"
    o = out.cpu()
    if c["planar"]:
        o = o.permute(1, 0, 2).reshape(M, 48)          # every plane is written whole
    outside = torch.cat([o[:, :col_off], o[:, col_off + width:]], 1)
    assert bool((outside == SENT).all()), "columns outside the window changed"
    win = o[:, col_off:col_off + width].float()
    pad = torch.ones(width, dtype=torch.bool)
    pad[real] = False
    if bool(pad.any()):                                # vectorised path only: exactly zero, or exactly the residual's pad value
        assert c["vec"]
        assert torch.equal(win[:, pad], c["base"][:, pad] if c["res"] else torch.zeros(M, int(pad.sum())))
    ref = c["exp"] + c["base"][:, real].double() if c["res"] else c["exp"]
    got = win[:, real].double()
    assert bool(torch.isfinite(got).all())
    e = rel(got, ref)
    if store == "f32":
        print(f"{c['path']} {c['grid']} f32: rel {e:.3e}")
        assert e < F32_BOUND
    else:
        tol = BF16_ULP * ref.abs() + F32_BOUND * ref.abs().max()
        worst = float(((got - ref).abs() / tol).max())
        print(f"{c['path']} {c['grid']} bf16: rel {e:.3e}  worst |out - ref| / (2^-8 |ref| + 2e-5 max|ref|) {worst:.3f}")
        assert worst <= 1.0
    if c["stats"]:                                     # sums of the values before storage rounding, without residual
        st, cout, v = stats.sum(0).cpu(), c["cout"], c["exp"]
        e1, e2 = rel(st[:cout], v.sum(0)), rel(st[cout:], (v * v).sum(0))
        print(f"{c['path']} {c['grid']} {store}: stats sum rel {e1:.3e}  sum of squares rel {e2:.3e}")
        assert e1 < STAT_BOUND and e2 < STAT_BOUND


def run_and_check(dev, store, c):
    buf, out, stats = launch(dev, store, c)
    check(c, store, buf, out, stats)
    if store == "bf16":                                # printed, not asserted: do the two storages contract identically?
        _, out32, _ = launch(dev, "f32", c)
        print(f"{c['path']} {c['grid']}: out_bf16 == out_f32.bfloat16() bitwise: {torch.equal(out, out32.bfloat16())}")
    return out


MATRIX = [(p, g, room) for g in GRIDS for p in PATHS for room in ((0,) if g == "multi" else (0, 4))
          if not (room and p == "dgrad_9x36_planes")]     # planar output has no spare columns


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("path,grid,room", MATRIX, ids=[f"{p}-{g}" + ("-room4" if r else "") for p, g, r in MATRIX])
def test_launch_path(dev, path, grid, room, store):
    c = case(path, grid, room)
    assert c["inst"] == PATHS[path][2], "the call does not select the instantiation this id stands for"
    run_and_check(dev, store, c)


def _bias_none():
    c = case("fwd_9x9", "faces", bias=None)
    c["exp"] = c["exp"] - reference(9, 9, "faces")["b"].double()
    return c


EXTRAS = {   # window, padding and input-side promises of the header that the matrix does not reach; all on `faces`
    "coloff12_rows48": lambda: case("fwd_9x9", "faces", ldc=48, col_off=12),
    "coloff12_rows48_inplace": lambda: case("dgrad_9x9_inplace", "faces", ldc=48, col_off=12),
    "coloff1_scalar": lambda: case("fwd_9x9", "faces", col_off=1),
    "nan_beyond_cin_load_fwd": lambda: case("fwd_9x9", "faces", nan_tail=4),               # ldx 16, cin_load 12
    "nan_beyond_cin_load_dgrad_1x9": lambda: case("dgrad_1x9_ld4", "faces", nan_tail=8),   # ldx 12, cin_load 4
    "residual_own_ldr16": lambda: case("dgrad_9x9", "faces", res="own", ldr=16),
    "residual_own_ldr16_scalar": lambda: case("dgrad_9x9", "faces", res="own", ldr=16, ldc=13),
    "bias_none_stats": _bias_none,
}
EXTRA_VEC = {"coloff1_scalar": False, "residual_own_ldr16_scalar": False}


@pytest.mark.parametrize("store", list(STORES))
@pytest.mark.parametrize("name", list(EXTRAS))
def test_window_and_padding_contract(dev, name, store):
    c = EXTRAS[name]()
    assert c["vec"] == EXTRA_VEC.get(name, True)
    run_and_check(dev, store, c)


# ------------------------------------------------------------------------------------------------------------------ sv_merger_pack
def kernel_pack(dev, w, dgrad, concat):
    wp = torch.full((16 * 27 * (48 if concat else 16),), SENT, dtype=torch.bfloat16, device=dev)
    call("sv_merger_pack", ptr(w.to(dev).contiguous()), ptr(wp), w.shape[0], w.shape[1], dgrad, concat)
    torch.cuda.synchronize()
    return wp


def hand_pack(w, dgrad, concat):
    cols = CAT if concat else torch.arange(w.shape[1])
    return (pack_dgrad(w, cols, 3 if concat else 1) if dgrad else pack_fwd(w, cols, 3 if concat else 1)).bfloat16()


@pytest.mark.parametrize("cout,cin,dgrad,concat", [(9, 9, 0, 0), (9, 9, 1, 0), (1, 9, 0, 0), (1, 9, 1, 0), (9, 36, 0, 1), (9, 36, 1, 1)])
def test_merger_pack_equals_hand_built_pack(dev, cout, cin, dgrad, concat):
    """One round-to-nearest of the same fp32 value on both sides: equal bit for bit, zeros (rows, columns, pad channels) included."""
    w = torch.randn(cout, cin, 3, 3, 3, generator=torch.Generator().manual_seed(100 * cout + cin)) / math.sqrt(27 * cin)
    got, want = kernel_pack(dev, w, dgrad, concat).cpu(), hand_pack(w, dgrad, concat).reshape(-1)
    nz = int((want != 0).sum())
    print(f"non-zero entries {nz} of {want.numel()}")
    assert nz == cout * cin * 27
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("path,dgrad", [("fwd_36x9_planes", 0), ("dgrad_9x36_planes", 1)])
@pytest.mark.parametrize("store", list(STORES))
def test_kernel_built_pack_gives_the_same_output(dev, path, dgrad, store):
    w = reference(36, 9, "faces")["w"]
    hand = case(path, "faces")
    assert torch.equal(hand["pack"].bfloat16(), hand_pack(w, dgrad, 1))
    built = case(path, "faces", pack=kernel_pack(dev, w, dgrad, 1).view(hand["pack"].shape).float().cpu())
    out_hand, out_built = run_and_check(dev, store, hand), run_and_check(dev, store, built)
    assert torch.equal(out_hand.view(torch.int16 if store == "bf16" else torch.int32), out_built.view(torch.int16 if store == "bf16" else torch.int32))


# ------------------------------------------------------------------------------------------------------------------ error convention
def _bad_calls():
    ok = dict(ldx=12, cin_load=12, groups=1, nt=1, ldc=12, col_off=0, cout=9, res=False, stats=False, grid=(1, 8, 8, 8), out_plane=0)
    return {
        "grid_D12": dict(ok, grid=(1, 12, 8, 8)),
        "stats_ntiles3": dict(ok, nt=3, ldc=48, cout=48, stats=True),
        "groups3_ntiles3": dict(ok, groups=3, nt=3, ldx=48, cin_load=48, ldc=48, cout=48),
        "cin_load6": dict(ok, cin_load=6),
        "ldc_below_window": dict(ok, col_off=4),
        "planar_out_residual": dict(ok, nt=3, cout=48, out_plane=512 * 12, res=True),
    }


@pytest.mark.parametrize("name", list(_bad_calls()))
def test_error_convention(dev, name):
    """Refused with a RuntimeError that names the entry point; nothing is launched: the sentinel-filled output comes back untouched."""
    a = _bad_calls()[name]
    n, D, H, W = a["grid"]
    M = 1024                                            # every buffer is larger than any of these calls could touch
    x = torch.zeros(M * 48, device=dev)
    w = torch.zeros(48 * 27 * 48, dtype=torch.bfloat16, device=dev)
    out = torch.full((M * 48,), SENT, device=dev)
    res = torch.zeros(M * 48, device=dev) if a["res"] else None
    stats = torch.full((ops.BN_SLOTS, 96), SENT, dtype=torch.float64, device=dev) if a["stats"] else None
    with pytest.raises(RuntimeError, match="sv_stencil3_fwd") as info:
        call("sv_stencil3_fwd", ptr(x), a["ldx"], a["cin_load"], a["groups"], ptr(w), a["nt"], None, ptr(out), a["ldc"], a["col_off"], a["cout"],
             ptr(res), a["ldc"] if a["res"] else 0, ptr(stats), n, D, H, W, 0, a["out_plane"], act=hip.F32)
    print(info.value)
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and (stats is None or bool((stats == SENT).all()))
