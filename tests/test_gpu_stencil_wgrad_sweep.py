"""The merger's stencil weight gradient as a sweep over halo slices (csrc/stencil.hip, stencil3_wgrad_sweep_kernel) against
torch conv3d autograd on bf16-rounded operands (fp32 accumulate): dw within rel < 2e-4 (the bound of
test_gpu_ops.py::test_stencil3_fwd_dgrad_wgrad), db within the same bound of the column sums of dy.

Grids: 8x8x8 x 1 image (one brick: every halo face is outside the volume), 16x8x24 x 2 (interior faces on every axis, unequal
extents), 32^3 x 9 (576 bricks > the resident grid: several bricks per workgroup through the prefetch path)."""
import functools
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from swinvox_amd import hip  # noqa: E402
from swinvox_amd.ops import call, ptr  # noqa: E402

BOUND = 2e-4
SWITCH = "SV_STENCIL_WGRAD_SWEEP"
GRIDS = {"brick": (1, 8, 8, 8), "faces": (2, 16, 8, 24), "multi": (9, 32, 32, 32)}
CHANNELS = [(9, 9, 1), (9, 1, 1), (36, 9, 3)]


def rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def cl(x):      # NC... -> N...C contiguous
    n = x.dim()
    return x.permute(0, *range(2, n), 1).contiguous()


@functools.lru_cache(maxsize=None)
def reference(cin, cout, groups, grid):
    """Operands in the kernels' memory layout and the conv3d autograd weight gradient; computed once per case and never modified."""
    n, D, H, W = GRIDS[grid]
    g = torch.Generator().manual_seed(1000 * cin + 10 * cout + len(grid))
    bf = lambda t: t.bfloat16().float()
    x = bf(torch.randn(n, cin, D, H, W, generator=g))
    w = bf(torch.randn(cout, cin, 3, 3, 3, generator=g) / math.sqrt(cin * 27)).requires_grad_(True)
    dy = bf(torch.randn(n, cout, D, H, W, generator=g))
    F.conv3d(x, w, None, padding=1).backward(dy)
    M = n * D * H * W
    ld = 12 if groups == 1 else 48
    cols = torch.arange(cin) if groups == 1 else torch.tensor([12 * k + j for k in range(4) for j in range(9)])
    xm = torch.zeros(M, ld); xm[:, cols] = cl(x).reshape(M, cin)
    dym = torch.zeros(M, 12); dym[:, :cout] = cl(dy).reshape(M, cout)
    return xm, dym, w.grad.detach(), dym[:, :cout].double().sum(0)


def run_wgrad(dev, cin, cout, groups, grid, store, planes=False, extras=True, dw0=None):
    """dw (and db, or None) from sv_stencil3_wgrad; extras = workspace + dbias, otherwise both null."""
    n, D, H, W = GRIDS[grid]
    xm, dym, _, _ = reference(cin, cout, groups, grid)
    M = xm.shape[0]
    dt, act = (torch.bfloat16, hip.BF16) if store == "bf16" else (torch.float32, hip.F32)
    dyd = dym.to(dev, dt)
    if planes:
        xd, ldx, cin_load, plane = xm.view(M, 4, 12).permute(1, 0, 2).contiguous().to(dev, dt), 12, 48, M * 12   # [4][M][12]
    else:
        xd, ldx, cin_load, plane = xm.to(dev, dt), xm.shape[1], xm.shape[1], 0
    dw = torch.zeros(cout, cin, 3, 3, 3, device=dev) if dw0 is None else dw0.to(dev).clone()
    db = torch.zeros(cout, device=dev) if extras else None
    ws = torch.zeros(16 * cout * cin * 27, device=dev) if extras else None
    call("sv_stencil3_wgrad", ptr(xd), ldx, cin_load, groups, ptr(dyd), 12, 12, ptr(dw), ptr(db) if extras else None, ptr(ws) if extras else None,
         cout, cin, 16 if groups == 1 else 12, 9, n, D, H, W, plane, act=act)
    torch.cuda.synchronize()
    return dw, db


@pytest.fixture(autouse=True)
def _default_switch():
    old = os.environ.pop(SWITCH, None)
    yield
    os.environ.pop(SWITCH, None)
    if old is not None:
        os.environ[SWITCH] = old


@pytest.mark.parametrize("extras", [True, False], ids=["ws_dbias", "null"])
@pytest.mark.parametrize("store", ["bf16", "f32"])
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("cin,cout,groups,planes", [(9, 9, 1, False), (9, 1, 1, False), (36, 9, 3, False), (36, 9, 3, True)],
                         ids=["9x9", "9x1", "36x9_rows48", "36x9_planes"])
def test_sweep_matches_conv3d(dev, cin, cout, groups, planes, grid, store, extras):
    _, _, dw_ref, db_ref = reference(cin, cout, groups, grid)
    dw, db = run_wgrad(dev, cin, cout, groups, grid, store, planes=planes, extras=extras)
    e = rel(dw, dw_ref)
    print(f"dw rel {e:.3e}")
    assert e < BOUND
    if extras:
        eb = rel(db, db_ref)
        print(f"db rel {eb:.3e}")
        assert eb < BOUND


@pytest.mark.parametrize("extras", [True, False], ids=["ws_dbias", "null"])
def test_sweep_accumulates_into_dw(dev, extras):
    """dw += : a non-zero initial dw comes back as initial + gradient."""
    cin, cout, groups, grid = 9, 9, 1, "faces"
    _, _, dw_ref, _ = reference(cin, cout, groups, grid)
    dw0 = torch.randn(cout, cin, 3, 3, 3, generator=torch.Generator().manual_seed(7)) * float(dw_ref.abs().max())
    dw, _ = run_wgrad(dev, cin, cout, groups, grid, "bf16", extras=extras, dw0=dw0)
    e = rel(dw, dw0 + dw_ref)
    print(f"dw0 + dw rel {e:.3e}")
    assert e < BOUND


@pytest.mark.parametrize("cin,cout,groups", [(9, 9, 1), (36, 9, 3)])
def test_switch_selects_tap_split_kernel_and_both_agree(dev, cin, cout, groups):
    """SV_STENCIL_WGRAD_SWEEP=0 runs the tap-split kernel: each kernel meets the bound, and they agree within it."""
    grid = "multi"
    _, _, dw_ref, db_ref = reference(cin, cout, groups, grid)
    os.environ[SWITCH] = "0"
    dw_old, db_old = run_wgrad(dev, cin, cout, groups, grid, "bf16")
    os.environ[SWITCH] = "1"
    dw_new, db_new = run_wgrad(dev, cin, cout, groups, grid, "bf16")
    figs = {"old dw": rel(dw_old, dw_ref), "new dw": rel(dw_new, dw_ref), "new vs old dw": rel(dw_new, dw_old),
            "old db": rel(db_old, db_ref), "new db": rel(db_new, db_ref), "new vs old db": rel(db_new, db_old)}
    print("  ".join(f"{k} {v:.3e}" for k, v in figs.items()))
    assert all(v < BOUND for v in figs.values())
