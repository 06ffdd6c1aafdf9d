"""fp64 reference, error model and case builder of the stand-alone BatchNorm passes (csrc/norm.hip: sv_bn_stats, sv_bn_finalize,
sv_scale_shift_act(_signs), sv_bn_bwd(_signs)), pinned here on the CPU; tests/test_gpu_batchnorm_paths.py imports this file and holds the
kernels to it on every launch path.

Error model (bn_check): |got - ref| <= K * 2^-24 * bound, elementwise, where `bound` is the sum of the magnitudes of the terms the output is
built from - an fp32 evaluation of a well-rounded formula errs by a few 2^-24 of THAT, not of the (possibly cancelled) result.  Outputs stored
as bf16 get 2^-8 |ref| on top: round-to-nearest costs 2^-9 relative, the doubling allows one last-place flip from the fp32 value underneath.
K is one constant for every output, measured on the kernels (see the table in tests/test_gpu_batchnorm_paths.py) and capped at 256: above
that a kernel with fp32 statistics would pass (test_checker_rejects_corruptions).

Bounds that the formulas of bn_reference do not already name, each the magnitudes of what fp32 combines:
  mean          sum|x| / M                       (double sums, one rounding)
  rstd          rstd                             (rsqrtf: a few last places)
  scale         |gamma| rstd
  shift         |beta| + |mean scale|
  running_mean  (1 - m)|rm| + m sum|x| / M
  running_var   (1 - m)|rv| + m var M/(M-1)      (the variance itself is formed in double)
  dres          |d|                              (one product)
"""
import functools
import math

import pytest
import torch

ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 3     # SV_ACT_* of include/swinvox_hip.h
EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.2
U24 = 2.0 ** -24
GUARD = 64 * U24         # no |p| below GUARD * Bz: the fma's rounding plus a few ulp each on scale and shift stay under it
K = 64                   # 4 x the largest ratio measured on the MI355X (15.5: dx, scalar family, LeakyReLU, mask from z), rounded up to a power of two
K_MAX = 256
assert K <= K_MAX

OUTPUTS = ("z", "dres", "dx", "dgamma", "dbeta", "mean", "rstd", "scale", "shift", "running_mean", "running_var")
BOUND_OF = dict(z="Bz", dres="Bdres", dx="Bdx", dgamma="Bdgamma", dbeta="Bdbeta", mean="Bmean", rstd="Brstd", scale="Bscale", shift="Bshift",
                running_mean="Brm", running_var="Brv")
STORED = ("z", "dres", "dx")     # activation tensors: bf16 in bf16 storage; everything else stays fp32


# ---- a. the reference -----------------------------------------------------------------------------------------------------------------
def bn_reference(x, gamma, beta, dz, res=None, act=ACT_NONE, slope=SLOPE, eps=EPS, training=True, running_mean=None, running_var=None,
                 momentum=MOMENTUM):
    """BatchNorm (+ residual) + activation, forward and backward, on channels-last [M, C] in float64 from the inputs as given.  Returns a dict:
    the quantities (mean, var, rstd, scale, shift, p, z, mask, d, dgamma, dbeta, dx, running_mean, running_var) and the bounds B* of bn_check."""
    f = lambda t: None if t is None else t.detach().to(torch.float64)
    x, gamma, beta, dz, res, rm, rv = f(x), f(gamma), f(beta), f(dz), f(res), f(running_mean), f(running_var)
    M, C = x.shape
    absmean = x.abs().sum(0) / M
    if training:
        mean = x.sum(0) / M
        var = ((x - mean) ** 2).sum(0) / M                     # biased, two-pass
    else:
        mean, var = rm, rv
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    p = x * scale + shift
    if res is not None:
        p = p + res
    mask = p > 0
    if act == ACT_NONE:
        z, dact = p, torch.ones_like(p)
    else:
        neg = slope if act == ACT_LRELU else 0.0
        dact = torch.where(mask, torch.ones_like(p), torch.full_like(p, neg))
        z = p * dact
    d = dz * dact
    xhat = (x - mean) * rstd
    dgamma, dbeta = (d * xhat).sum(0), d.sum(0)
    k1 = scale
    if training:
        a, b = dbeta / M, dgamma / M
        k3 = k1 * b * rstd
        dx = k1 * d - k1 * a + k3 * mean - k3 * x
        Bdx = (k1 * d).abs() + (k1 * a).abs() + (k3 * mean).abs() + (k3 * x).abs()
    else:
        dx = d * scale
        Bdx = (k1 * d).abs()
    out = dict(mean=mean, var=var, rstd=rstd, scale=scale, shift=shift, p=p, z=z, mask=mask, d=d, dres=d, dgamma=dgamma, dbeta=dbeta, dx=dx)
    out.update(Bz=(x * scale).abs() + beta.abs() + (mean * scale).abs() + (res.abs() if res is not None else 0.0), Bdx=Bdx,
               Bdgamma=(d.abs() * (x.abs() + mean.abs())).sum(0) * rstd, Bdbeta=d.abs().sum(0), Bdres=d.abs(),
               Bmean=absmean if training else mean.abs(), Brstd=rstd, Bscale=scale.abs(), Bshift=beta.abs() + (mean * scale).abs())
    if rm is not None:
        if training:
            unb = var * (M / (M - 1.0) if M > 1 else 1.0)      # bn_finalize_kernel: unbiased factor M / (M - 1), 1 when M == 1
            out.update(running_mean=(1 - momentum) * rm + momentum * mean, running_var=(1 - momentum) * rv + momentum * unb,
                       Brm=(1 - momentum) * rm.abs() + momentum * absmean, Brv=(1 - momentum) * rv.abs() + momentum * unb)
        else:
            out.update(running_mean=rm, running_var=rv, Brm=rm.abs(), Brv=rv.abs())
    return out


# ---- b. the checker -------------------------------------------------------------------------------------------------------------------
RATIOS = {}      # (output kind, stored_bf16) -> largest |got - ref| / (2^-24 bound) seen by bn_check (after the bf16 term), for the K table


def bn_ratio(got, ref, bound, stored_bf16):
    """max over the elements of (|got - ref| - [2^-8 |ref|]) / (2^-24 bound); inf when an element is not finite or errs where the bound is 0"""
    got, ref = got.detach().to(torch.float64).cpu(), ref.to(torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref).abs()
    if stored_bf16:
        err = (err - 2.0 ** -8 * ref.abs()).clamp_min(0.0)
    r = torch.where(err == 0, torch.zeros_like(err), err / (U24 * bound))      # 0 / 0 -> 0, e / 0 -> inf
    return float(r.max())


def bn_check(name, got, ref, bound, K, stored_bf16=False):
    """|got - ref| <= K 2^-24 bound (+ 2^-8 |ref| for an output stored as bf16) for every element, none of them non-finite"""
    r = bn_ratio(got, ref, bound, stored_bf16)
    kind = name.split(":")[-1]
    RATIOS[(kind, bool(stored_bf16))] = max(RATIOS.get((kind, bool(stored_bf16)), 0.0), r)
    assert r <= K, f"{name}: error {r:.3g} x 2^-24 x bound exceeds K = {K} (bf16 storage: {bool(stored_bf16)})"


# ---- c. cases -------------------------------------------------------------------------------------------------------------------------
def _q(t, bf16):
    """round to what the tensor is stored as; the case keeps the stored values in float64"""
    return (t.to(torch.bfloat16) if bf16 else t.to(torch.float32)).to(torch.float64)


def bn_make_case(M, C, act, with_res, offset=0.0, bf16=False, seed=0, training=True, const_channel=None):
    """Draws x (offset + 0.5 randn when offset != 0, else 2 randn + 0.5), res, dz, gamma, beta and running statistics, then removes mask
    ambiguity: elements with |p| < GUARD * Bz are nudged (in res when there is one - the statistics stay -, else in x; whole bf16 steps in a bf16
    case) and the reference recomputed, at most 8 rounds; a case that still has one is an error.  const_channel: that channel of x is constant."""
    g = torch.Generator().manual_seed(1000003 * seed + 8191 * M + C)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x = offset + 0.5 * rn(M, C) if offset else 2.0 * rn(M, C) + 0.5
    if const_channel is not None:
        x[:, const_channel] = 3.0 + offset
    res = rn(M, C) if with_res else None
    # dz is not centred: with a zero-mean dz both a = sum(d) / M and b = sum(d xhat) / M cancel to (almost) nothing in the odd channel out of a
    # thousand, and Bdx, built from |a| and |b| THEMSELVES, then no longer covers the rounding of the fp32 products behind b (Bdgamma does)
    dz = rn(M, C) + 0.5
    gamma = (1.0 + 0.3 * rn(C)).abs() * torch.where(torch.arange(C) % 5 == 4, -1.0, 1.0)      # some negative scales
    beta, rm, rv = 0.3 * rn(C), 0.5 * rn(C) + (offset if offset else 0.5), 0.5 + torch.rand(C, generator=g, dtype=torch.float64) * (4.0 if not offset else 0.5)
    x, dz, res = _q(x, bf16), _q(dz, bf16), (None if res is None else _q(res, bf16))
    gamma, beta, rm, rv = (_q(t, False) for t in (gamma, beta, rm, rv))
    kw = dict(act=act, slope=SLOPE, eps=EPS, training=training, running_mean=rm, running_var=rv, momentum=MOMENTUM)
    rounds = 0
    while True:
        ref = bn_reference(x, gamma, beta, dz, res, **kw)
        bad = ref["p"].abs() < GUARD * ref["Bz"]
        if not bool(bad.any()):
            break
        if rounds == 8:
            raise RuntimeError(f"bn_make_case({M}, {C}): {int(bad.sum())} elements still inside the mask guard after 8 rounds")
        rounds += 1
        away = torch.where(ref["p"] < 0, -1.0, 1.0).to(torch.float64)
        if res is not None:      # p moves by the step itself
            step = torch.maximum(4 * GUARD * ref["Bz"], 2.0 ** -7 * res.abs())        # >= one bf16 step of res, so the rounded value moves
            res = torch.where(bad, _q(res + away * step, bf16), res)
        else:                    # p moves by scale * step (and, slightly, with the statistics: hence the rounds)
            sc = ref["scale"].expand_as(x)
            step = torch.maximum(4 * GUARD * ref["Bz"] / sc.abs().clamp_min(1e-30), 2.0 ** -7 * x.abs())
            x = torch.where(bad, _q(x + away * torch.sign(sc) * step, bf16), x)
    return dict(M=M, C=C, act=act, slope=SLOPE, eps=EPS, momentum=MOMENTUM, training=training, bf16=bf16, x=x, res=res, dz=dz, gamma=gamma,
                beta=beta, running_mean=rm, running_var=rv, ref=ref, rounds=rounds)


@functools.lru_cache(maxsize=24)
def bn_case(M, C, act, with_res, offset=0.0, bf16=False, seed=0, training=True, const_channel=None):
    """bn_make_case, computed once per process and shared (nobody writes into a case)"""
    return bn_make_case(M, C, act, with_res, offset, bf16, seed, training, const_channel)


def sign_words(p):
    """The sign words of sv_scale_shift_act_signs for the pre-activation p [M, C], C % 256 == 0, as int64 [M, C/256, 4]:
    bit l of word[(r C/256 + b) 4 + j] = p[r, 256 b + 4 l + j] > 0."""
    M, C = p.shape
    bits = (p > 0).view(M, C // 256, 64, 4).to(torch.int64)
    w = torch.zeros(M, C // 256, 4, dtype=torch.int64)
    for l in range(64):
        w |= bits[:, :, l, :] << l
    return w


# the shapes of the forward / statistics matrix (family -> (C, M)); the GPU file adds the strides and alignments that select the family
FWD_SHAPES = {
    "scalar": [(C, M) for C in (1, 9, 18, 8) for M in (1, 2, 65, 1031)],
    "narrow": [(C, M) for C in (9, 1, 2, 13) for M in (63, 64, 65)] + [(9, 17000)],
    "vec": [(C, M) for C in (4, 12, 40, 64, 256, 320, 1024) for M in (3, 517, 1031)],
}
SIGN_SHAPES = [(C, M) for C in (256, 512) for M in (5, 1031)]


def fwd_recipe(C, M):
    """activation, residual and offset of a forward shape: every third shape has none / ReLU / LeakyReLU, every second a residual, and the
    offset (x = 10 + 0.5 randn, what fp32 statistics cannot carry) goes to every shape with M >= 63 whose C + M is even"""
    act = (ACT_RELU, ACT_LRELU, ACT_NONE)[(C + M) % 3]
    return dict(act=act, with_res=(C + M // 2) % 2 == 0, offset=10.0 if (M >= 63 and (C + M) % 2 == 0) else 0.0)


# backward: one representative shape per family (M, C), the two-rows-in-flight tail with more row blocks than reduce slots (vec256), more than
# 16 workgroups of the narrow reduce (narrow_wrap), the merger's two stride patterns and the shapes of the misaligned fwd_scale / fwd_shift
BWD_SHAPES = {"scalar": (65, 18), "narrow": (65, 9), "vec": (517, 40), "vec256": (1031, 256), "narrow_wrap": (17000, 9), "merger12": (1031, 9),
              "merger1": (1031, 1), "fsc8": (65, 8), "fsc24": (65, 24)}
MASK_RECIPES = {"z": True, "recompute": False, "none": False}     # mask source -> the forward had a residual


def bwd_recipe(shape, act, mask, training, bf16):
    """bn_case arguments of a backward case; LeakyReLU training cases carry the offset"""
    M, C = BWD_SHAPES[shape]
    return (M, C, act, MASK_RECIPES[mask], 10.0 if (training and act == ACT_LRELU) else 0.0, bf16, 2, training)


def sign_recipe(C, M, act, bf16, training=True):
    return (M, C, act, True, 0.0, bf16, 1, training)


CONST_CHANNEL = 1


def const_recipe(bf16):
    """one constant channel (variance 0); with a residual, so that the guard's nudges leave x alone"""
    return (65, 12, ACT_RELU, True, 0.0, bf16, 4, True, CONST_CHANNEL)


def fwd_has_eval(M):
    """the forward shapes that also run in eval mode: one row count per family"""
    return M in (65, 517)


def listed_cases():
    """bn_case arguments of every numeric case the GPU file draws, both storage modes"""
    out = []
    for bf16 in (False, True):
        for fam, shapes in FWD_SHAPES.items():
            for C, M in shapes:
                r = fwd_recipe(C, M)
                out.append((M, C, r["act"], r["with_res"], r["offset"], bf16, 0, True))
                if fwd_has_eval(M):
                    out.append((M, C, r["act"], r["with_res"], r["offset"], bf16, 0, False))
        for C, M in SIGN_SHAPES:
            for act in (ACT_RELU, ACT_LRELU):
                out.append(sign_recipe(C, M, act, bf16))
            out.append(sign_recipe(C, M, ACT_RELU, bf16, False))
        for shape in BWD_SHAPES:
            for act, mask in ((ACT_RELU, "z"), (ACT_LRELU, "z"), (ACT_RELU, "recompute"), (ACT_LRELU, "recompute"), (ACT_NONE, "none")):
                for training in (True, False):
                    out.append(bwd_recipe(shape, act, mask, training, bf16))
        out.append(const_recipe(bf16))
    return out


def _case_id(c):
    M, C, act, with_res, offset, bf16, seed, training = c[:8]
    return (f"M{M}-C{C}-{ {0: 'none', 1: 'relu', 3: 'lrelu'}[act]}{'-res' if with_res else ''}{'-off' if offset else ''}"
            f"-{'bf16' if bf16 else 'f32'}-{'train' if training else 'eval'}-s{seed}{'-const' if len(c) > 8 else ''}")


CASES = sorted(set(listed_cases()))


# ---- the documented arithmetic in fp32, and ways to get it wrong -----------------------------------------------------------------------
CORRUPTIONS = ("unbiased_var", "fwd_last_row", "bwd_last_row", "channel_scale", "mask_flip", "fp32_stats")


def bn_emulate(case, corrupt=None):
    """What the kernels document, in torch on the CPU: statistics in double from the stored values, fp32 rstd / scale / shift, p by one fma
    (+ res), fp32 products summed in double, dx in double from the fp32 per-channel constants; activations rounded to the storage type."""
    f32, f64 = torch.float32, torch.float64
    M, C, act, training = case["M"], case["C"], case["act"], case["training"]
    x, dz, res = case["x"], case["dz"], case["res"]
    gm, bt, rm, rv = (case[k].to(f32) for k in ("gamma", "beta", "running_mean", "running_var"))
    out = {}
    if training:
        xs = x[:-1] if corrupt == "fwd_last_row" else x
        if corrupt == "fp32_stats":
            s1, s2 = xs.to(f32).sum(0), (xs.to(f32) * xs.to(f32)).sum(0)
            m = s1 / M
            v = (s2 / M - m * m).clamp_min(0.0).to(f64)
            m = m.to(f64)
        else:
            m = xs.sum(0) / M
            v = ((xs * xs).sum(0) / M - m * m).clamp_min(0.0)
        mean, var = m.to(f32), v.to(f32)
        out["running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
        out["running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * (v * (M / (M - 1.0) if M > 1 else 1.0)).to(f32)
        if corrupt == "unbiased_var" and M > 1:
            var = (v * M / (M - 1.0)).to(f32)
    else:
        mean, var = rm, rv
        out["running_mean"], out["running_var"] = rm, rv
    rstd = torch.rsqrt(var + torch.tensor(case["eps"], dtype=f32))
    scale = gm * rstd
    shift = bt - mean * scale
    sc_apply = scale.clone()
    if corrupt == "channel_scale":
        sc_apply[0] = scale[-1]
    p = (x * sc_apply.to(f64) + shift.to(f64)).to(f32)           # the fma: exact product and sum, one rounding
    if res is not None:
        p = p + res.to(f32)
    mask = p > 0
    if corrupt == "mask_flip":
        mask = mask.clone()
        mask[M // 2, C // 2] = ~mask[M // 2, C // 2]
    neg = {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: case["slope"]}[act]
    dact = torch.where(mask, torch.ones_like(p), torch.full_like(p, neg)) if act != ACT_NONE else torch.ones_like(p)
    z = p * dact
    d = dz.to(f32) * dact
    xf = x.to(f32)
    prod = d * (xf - mean) * rstd                                # fp32 products ...
    rows = slice(0, M - 1) if corrupt == "bwd_last_row" else slice(0, M)
    s1, s2 = d[rows].to(f64).sum(0), prod[rows].to(f64).sum(0)   # ... summed in double
    k1 = gm.to(f64) * rstd.to(f64)
    if training:
        a, b = s1 / M, s2 / M
        k3 = k1 * b * rstd.to(f64)
        k2 = k1 * a - k3 * mean.to(f64)
        dx = (k1 * d.to(f64) - k2 - k3 * x).to(f32)
    else:
        dx = d * gm * rstd
    out.update(mean=mean, rstd=rstd, scale=scale, shift=shift, z=_q(z, case["bf16"]), dres=_q(d, case["bf16"]), dx=_q(dx, case["bf16"]),
               dgamma=s2.to(f32), dbeta=s1.to(f32))
    return out


def emulation_ratios(case, corrupt=None):
    ref, emu = case["ref"], bn_emulate(case, corrupt)
    return {k: bn_ratio(emu[k], ref[k], ref[BOUND_OF[k]], case["bf16"] and k in STORED) for k in OUTPUTS}


# ---- d. tests -------------------------------------------------------------------------------------------------------------------------
def _autograd(case):
    import torch.nn.functional as F
    x = case["x"].clone().requires_grad_(True)
    res = case["res"].clone().requires_grad_(True) if case["res"] is not None else None
    gm, bt = case["gamma"].clone().requires_grad_(True), case["beta"].clone().requires_grad_(True)
    rm, rv = case["running_mean"].clone(), case["running_var"].clone()
    y = F.batch_norm(x, rm, rv, gm, bt, training=case["training"], momentum=case["momentum"], eps=case["eps"])
    if res is not None:
        y = y + res
    z = {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_LRELU: lambda t: F.leaky_relu(t, case["slope"])}[case["act"]](y)
    z.backward(case["dz"])
    return dict(z=z.detach(), dx=x.grad, dgamma=gm.grad, dbeta=bt.grad, dres=None if res is None else res.grad, running_mean=rm, running_var=rv)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("M,C,act,with_res,offset", [(2, 3, ACT_RELU, True, 0.0), (65, 9, ACT_LRELU, False, 0.0), (517, 40, ACT_NONE, True, 10.0),
                                                     (1031, 256, ACT_RELU, False, 10.0), (63, 1, ACT_LRELU, True, 0.0)])
def test_reference_is_torch_batch_norm(M, C, act, with_res, offset, training):
    """the written-out formulas against torch.nn.functional.batch_norm + the activation's autograd, both in float64: 1e-12 of the largest term"""
    case = bn_make_case(M, C, act, with_res, offset, False, 3, training)
    ref, ag = case["ref"], _autograd(case)
    for k, v in ag.items():
        if v is not None:
            den = float(ref[BOUND_OF[k]].max())      # the magnitude of the terms: with M == 2 dx itself cancels to rounding
            assert float((ref[k] - v).abs().max()) <= 1e-12 * den, k


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_listed_cases_hold_the_guard(c):
    case = bn_case(*c)
    ref = case["ref"]
    assert bool((ref["p"].abs() >= GUARD * ref["Bz"]).all()) and case["rounds"] <= 8
    for t in (case["x"], case["dz"], case["res"]):
        if t is not None:
            assert torch.equal(_q(t, case["bf16"]), t)          # the case holds exactly what the GPU buffers will hold


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_fp32_emulation_passes(c):
    r = emulation_ratios(bn_case(*c))
    assert max(r.values()) <= K, r


def _applies(c, corrupt):
    """fp32 statistics are told apart on the offset cases only; no mask without an activation; eval mode takes its statistics as given"""
    M, C, act, with_res, offset, bf16, seed, training = c[:8]
    if C <= 1 or M <= 2 or (corrupt == "fp32_stats" and not offset) or (corrupt == "mask_flip" and act == ACT_NONE):
        return False
    return training or corrupt not in ("unbiased_var", "fwd_last_row", "fp32_stats")


@pytest.mark.parametrize("c,corrupt", [(c, k) for c in CASES for k in CORRUPTIONS if _applies(c, k)], ids=lambda v: v if isinstance(v, str) else _case_id(v))
def test_checker_rejects_corruptions(c, corrupt):
    """the power of bn_check at the K in force: every corruption must push at least one output of every case over K"""
    r = emulation_ratios(bn_case(*c), corrupt)
    assert max(r.values()) > K, (corrupt, r)


def test_sign_words_layout():
    g = torch.Generator().manual_seed(5)
    p = torch.randn(3, 512, generator=g, dtype=torch.float64)
    w = sign_words(p)
    assert w.shape == (3, 2, 4)
    for r, c in ((0, 0), (1, 255), (2, 256), (2, 511), (1, 300)):
        b, l, j = c // 256, (c % 256) // 4, c % 4
        assert bool((int(w[r, b, j]) >> l) & 1) == bool(p[r, c] > 0)
    assert int(sign_words(torch.ones(1, 256, dtype=torch.float64))[0, 0, 0]) == -1      # all 64 bits, two's complement


def test_k_is_capped():
    assert 0 < K <= K_MAX == 256
