"""Window attention at SEVERAL WINDOWS PER WORKGROUP (per wave in the exact-fp32 kernels).

Every window kernel of csrc/attn.hip walks a run of consecutive windows of one head; host heuristics choose the run's length (the
"share").  The other op tests call the kernels with at most 128 windows, where every share is 1, so the window loop, its LDS reuse, the
next-window prefetch of the backward kernels, the bias-gradient sums carried across windows, the ragged last run and the padded grid
slots run against no reference there.  The cases below are the smallest that put each kernel at a share >= 2 with a ragged tail; every
test asks sv_window_attention_windows_per_group (the function the launches take their share from) for the share of every launch it makes
and fails if a case has fallen back to share 1.

Two oracles, for every math mode and both storages:
 (a) the same images again in slices of consecutive images, each small enough that the query answers 1: `out` and `dqkv` of a window are
     written by exactly one workgroup without atomics and must not depend on the loop iteration that computed them - bit for bit, no
     tolerance.  No kernel here computes a later window with other arithmetic than the first, so there is no exception to the equality.
 (b) the fp64 reference of the operation (_ref_window_attention of tests/test_gpu_ops.py + autograd) at the tolerances the suite applies
     to these kernels at share 1 (max |err| / max |ref|: fp32 2e-4; bf16 out 2e-2, dqkv / dtable 3e-2; fp8 forward: mean error 8e-2);
     the fp8 backward (SV_MATH_FP8_FULL) against the recipe emulation of tests/test_gpu_attn_fp8_bwd.py at that file's L1_BOUND.  dtable
     is the output that cannot be bit-equal (atomics); it is what checks the carried sums and dbias_flush, with the workspace NULL and
     given.

Inputs are N(0, 1) qkv and dout rounded to bf16-representable values (so that fp32 and bf16 storage read the same numbers and share one
reference) and a 0.5 N(0, 1) table.  The exact-fp32 kernels therefore see no operand with a full fp32 mantissa here: an fp32 path that
truncated its inputs would pass this file.  tests/test_gpu_ops.py feeds them unrounded N(0, 1) inputs at share 1, and oracle (a) ties
every share above 1 to share 1 bit for bit, so nothing is left uncovered by the rounding.

Tails: for the workgroup kernels a tail is windows % share != 0.  The exact-fp32 backward puts two waves in a workgroup, so its last
workgroup is ragged when windows % (2 share) != 0: in case C that leaves the second wave without a window (130 = 32 * 4 + 2), in cases A
and B the last wave has one window of two."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from swinvox_amd import hip  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402
from test_gpu_attn_fp8_bwd import L1_BOUND, _emulate, _l1  # noqa: E402
from test_gpu_ops import _ref_window_attention  # noqa: E402

F32, BF16, FP8, FP8_FULL = hip.MATH_F32, hip.MATH_BF16, hip.MATH_FP8, hip.MATH_FP8_FULL
MODES = [(F32, "f32"), (BF16, "f32"), (BF16, "bf16"), (FP8, "f32"), (FP8, "bf16"), (FP8_FULL, "f32"), (FP8_FULL, "bf16")]
# max |err| / max |ref| against the fp64 reference: (out, dqkv, dtable)
TOL_F32 = (2e-4, 2e-4, 2e-4)
TOL_BF16 = (2e-2, 3e-2, 3e-2)
FP8_FWD_MEAN = 8e-2

#         I, H, heads, shift, ragged forward
CASES = {"A-shift0": (153, 21, 3, 0, True), "A-shift3": (153, 21, 3, 3, True), "B": (57, 21, 8, 3, True), "C": (130, 7, 32, 0, False)}


def _share(I, H, heads, math, backward):
    s = hip.load().sv_window_attention_windows_per_group(I, H, H, heads, math, int(backward))
    assert s >= 1, (s, I, H, heads, math, backward)
    return s


def _slices(I, H, heads, math, backward):
    """consecutive image ranges (i0, n), each as long as the query still answers 1 for it"""
    n = next(n for n in range(I, 0, -1) if _share(n, H, heads, math, backward) == 1)
    sl = [(i0, min(n, I - i0)) for i0 in range(0, I, n)]
    assert all(_share(m, H, heads, math, backward) == 1 for _, m in sl), sl
    return sl


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class _Case:
    def __init__(self, I, H, heads, shift, dev, seed):
        self.I, self.H, self.heads, self.shift, self.C, self.dev = I, H, heads, shift, heads * 32, dev
        g = torch.Generator().manual_seed(seed)
        M, C = I * H * H, self.C
        self.qkv = torch.randn(M, 3 * C, generator=g).bfloat16().float()
        self.dout = torch.randn(M, C, generator=g).bfloat16().float()
        self.table = 0.5 * torch.randn(169, heads, generator=g)
        q64, t64 = self.qkv.double().requires_grad_(True), self.table.double().requires_grad_(True)
        ref = _ref_window_attention(q64, t64, I, H, C, heads, shift)
        ref.backward(self.dout.double())
        self.ref = tuple(t.detach().to(dev) for t in (ref, q64.grad, t64.grad))     # out, dqkv, dtable (fp64, read-only)
        self.td = self.table.to(dev)
        self.d = {"f32": (self.qkv.to(dev), self.dout.to(dev))}
        self.d["bf16"] = tuple(t.bfloat16() for t in self.d["f32"])
        self._recipe = None

    def recipe(self):
        """dqkv, dtable of the fp8 backward recipe (the stored values are the same under both storages)"""
        if self._recipe is None:
            self._recipe = _emulate(self.qkv, self.table, self.dout, self.I, self.H, self.C, self.heads, self.shift)
        return self._recipe

    def release(self):
        """drop every tensor of the case (whoever still holds the object holds nothing of size) and hand the device memory back"""
        self.ref = self.d = self.td = self.qkv = self.dout = self._recipe = None
        torch.cuda.empty_cache()

    def rows(self, t, i0, n):
        return t[i0 * self.H * self.H:(i0 + n) * self.H * self.H]

    def fwd(self, math, store, parts=None):
        """out of one call over all images, or of one call per (i0, n) of `parts`"""
        qd = self.d[store][0]
        out = torch.full((qd.shape[0], self.C), float("nan"), dtype=qd.dtype, device=self.dev)
        for i0, n in parts or [(0, self.I)]:
            call("sv_window_attention_fwd", ptr(self.rows(qd, i0, n)), ptr(self.td), ptr(self.rows(out, i0, n)), n, self.H, self.H, self.C,
                 self.heads, self.shift, math, act=hip.BF16 if store == "bf16" else hip.F32)
        torch.cuda.synchronize()
        return out

    def bwd(self, math, store, workspace=False, parts=None):
        """(dqkv, dtable); dtable accumulates over the calls of `parts`"""
        qd, dod = self.d[store]
        dqkv = torch.full(qd.shape, float("nan"), dtype=qd.dtype, device=self.dev)
        dt = torch.zeros(169, self.heads, device=self.dev)
        for i0, n in parts or [(0, self.I)]:
            ws = torch.zeros(int(hip.load().sv_window_attention_bwd_workspace_floats(self.heads)), device=self.dev) if workspace else None
            call("sv_window_attention_bwd", ptr(self.rows(qd, i0, n)), ptr(self.td), ptr(self.rows(dod, i0, n)), ptr(self.rows(dqkv, i0, n)),
                 ptr(dt), ptr(ws), n, self.H, self.H, self.C, self.heads, self.shift, math, act=hip.BF16 if store == "bf16" else hip.F32)
            torch.cuda.synchronize()
        return dqkv, dt


@pytest.fixture(scope="module", params=list(CASES))
def case(request, dev):
    """one case at a time (qkv of case A is 78 MB in fp32, its fp64 gradient twice that), its reference computed once and shared by the
    forward and the backward test, its device tensors freed before the next case"""
    I, H, heads, shift, _ = CASES[request.param]
    c = _Case(I, H, heads, shift, dev, seed=1000 * I + 10 * heads + shift)
    yield request.param, c
    c.release()


def _check_forward(c, math, out, tag):
    ref = c.ref[0]
    assert bool(torch.isfinite(out.float()).all()), tag
    if math in (FP8, FP8_FULL):
        e = float((out.double() - ref).abs().mean() / ref.abs().mean())
        print(f"{tag}: fp8 forward mean error {e:.3e}")
        assert e < FP8_FWD_MEAN, (tag, e)
    else:
        e = _rel(out, ref)
        print(f"{tag}: out max error {e:.3e}")
        assert e < (TOL_F32 if math == F32 else TOL_BF16)[0], (tag, e)


def _check_backward(c, math, store, dqkv, dt, tag):
    assert bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(dt).all()), tag
    if math == FP8_FULL:
        rq, rt = c.recipe()
        e_q, e_t = _l1(dqkv, rq), _l1(dt, rt)
        print(f"{tag}: fp8 backward vs recipe, L1: dqkv {e_q:.3e} dtable {e_t:.3e}")
        assert e_q < L1_BOUND[store] and e_t < L1_BOUND[store], (tag, e_q, e_t)
    else:   # SV_MATH_FP8 runs the bf16 backward
        tol = TOL_F32 if math == F32 else TOL_BF16
        e_q, e_t = _rel(dqkv, c.ref[1]), _rel(dt, c.ref[2])
        print(f"{tag}: dqkv max error {e_q:.3e} dtable max error {e_t:.3e}")
        assert e_q < tol[1] and e_t < tol[2], (tag, e_q, e_t)


def test_forward_at_several_windows_per_workgroup(case):
    name, c = case
    I, H, heads, shift, ragged = CASES[name]
    windows = I * (H // 7) ** 2
    assert _share(I, H, heads, F32, False) == 1            # wave per window, no loop
    for math, store in MODES:
        tag = f"{name} fwd math={math} {store}"
        share = _share(I, H, heads, math, False)
        if math != F32:
            assert share >= 2 and (not ragged or windows % share != 0), (tag, share, windows)
            parts = _slices(I, H, heads, math, False)
            assert len(parts) >= 2
        out = c.fwd(math, store)
        _check_forward(c, math, out, tag)
        if math == F32:
            continue
        assert torch.equal(_bits(out), _bits(c.fwd(math, store, parts))), tag      # oracle (a)


def test_backward_at_several_windows_per_workgroup(case):
    name, c = case
    I, H, heads, shift, _ = CASES[name]
    windows = I * (H // 7) ** 2
    for math, store in MODES:
        tag = f"{name} bwd math={math} {store}"
        share = _share(I, H, heads, math, True)
        # every case has a ragged last workgroup; the exact-fp32 kernel holds two waves (two runs of windows) per workgroup
        assert share >= 2 and windows % (2 * share if math == F32 else share) != 0, (tag, share, windows)
        if math == F32 and name != "C":
            assert windows % share != 0, (tag, share, windows)
        parts = _slices(I, H, heads, math, True)
        assert len(parts) >= 2
        dq1, dt1 = c.bwd(math, store, parts=parts)
        _check_backward(c, math, store, dq1, dt1, tag + " slices")
        for workspace in ((False,) if math == F32 else (False, True)):       # the exact-fp32 kernel has no slot images
            dq, dt = c.bwd(math, store, workspace)
            _check_backward(c, math, store, dq, dt, f"{tag} ws={workspace}")
            assert torch.equal(_bits(dq), _bits(dq1)), (tag, workspace)         # oracle (a)


@pytest.mark.parametrize("heads,shift", [(3, 0), (3, 3), (8, 3)])
def test_three_by_three_windows_at_one_window_per_workgroup(dev, heads, shift):
    """21 x 21 is the smallest map with an interior window without a seam, edge windows with one seam and a corner window with two.  Two
    images: every share is 1, so a failure of the cases above that this test does not share belongs to the window loop, not the geometry."""
    I, H = 2, 21
    c = _Case(I, H, heads, shift, dev, seed=77 + heads + shift)
    for math, store in MODES:
        assert _share(I, H, heads, math, False) == 1 and _share(I, H, heads, math, True) == 1
        tag = f"21x21 heads={heads} shift={shift} math={math} {store}"
        _check_forward(c, math, c.fwd(math, store), tag)
        for workspace in ((False,) if math == F32 else (False, True)):
            dq, dt = c.bwd(math, store, workspace)
            _check_backward(c, math, store, dq, dt, f"{tag} ws={workspace}")
    c.release()

