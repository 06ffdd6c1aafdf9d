"""Swin-T / Swin-B backbone + per-stage LayerNorm([C,H,W]) heads on HIP kernels.

Mirrors reference models/swin_transformer.py:10-94 (class SwinTransformer, attributes `model`, `layer_norm`,
`dropout`, `out_channels`, `out_spatial`) and the timm 1.0.15 `swin_tiny_patch4_window7_224` FeatureListNet it
wraps (state-dict keys `model.patch_embed.{proj,norm}`, `model.layers_{i}.downsample.{norm,reduction}`,
`model.layers_{i}.blocks.{j}.{norm1,attn.{qkv,proj,relative_position_bias_table},norm2,mlp.{fc1,fc2}}`;
notebook cell 68).  No pretrained weights are fetched (there is no network); `pretrained` is accepted and ignored
with a log line, exactly the tensors the reference would overwrite with init_weights anyway.

The modules below only HOLD parameters; the arithmetic is the kernel chain in swin_forward / swin_backward.
"""
from __future__ import annotations

import logging
from typing import List

import torch
import torch.nn as nn

from .. import ops
from ..ops import ACT_GELU, ACT_NONE, ConvSpec, call, empty, fempty, fzeros, ptr, zeros

_VARIANTS = {
    "tiny": dict(embed_dim=96, depths=(2, 2, 6, 2), heads=(3, 6, 12, 24)),
    "base": dict(embed_dim=128, depths=(2, 2, 18, 2), heads=(4, 8, 16, 32)),
}


class _Holder(nn.Module):
    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: run the parent Encoder / SwinTransformer module instead")


class WindowAttention(_Holder):
    def __init__(self, dim, heads, ws=7):
        super().__init__()
        self.num_heads = heads
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * ws - 1) ** 2, heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)


class Mlp(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.fc1 = nn.Linear(dim, 4 * dim)
        self.fc2 = nn.Linear(4 * dim, dim)


class SwinBlock(_Holder):
    def __init__(self, dim, res, heads, shift, drop_path):
        super().__init__()
        self.dim, self.res, self.heads = dim, res, heads
        self.shift = 0 if res <= 7 else shift          # timm: window clipped to the map => no shift (stage 3)
        self.drop_path = float(drop_path)
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, heads)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim)
        self.s_qkv, self.s_proj = ConvSpec.linear(dim, 3 * dim), ConvSpec.linear(dim, dim)
        self.s_fc1, self.s_fc2 = ConvSpec.linear(dim, 4 * dim), ConvSpec.linear(4 * dim, dim)


class PatchMerging(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.norm = nn.LayerNorm(4 * dim)
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.spec = ConvSpec.linear(4 * dim, 2 * dim)


class SwinStage(_Holder):
    def __init__(self, dim_in, dim, res, depth, heads, dps, merge):
        super().__init__()
        self.dim, self.res = dim, res
        self.downsample = PatchMerging(dim_in) if merge else nn.Identity()
        self.blocks = nn.Sequential(*[SwinBlock(dim, res, heads, 0 if i % 2 == 0 else 3, dps[i]) for i in range(depth)])


class PatchEmbed(_Holder):
    def __init__(self, in_ch, dim):
        super().__init__()
        self.proj = nn.Conv2d(in_ch, dim, 4, 4)
        self.norm = nn.LayerNorm(dim)


class _FeatureInfo:
    def __init__(self, ch):
        self._ch = list(ch)

    def channels(self):
        return list(self._ch)


class SwinBackbone(_Holder):
    def __init__(self, out_indices, embed_dim, depths, heads, img_size=224, drop_path_rate=0.1, in_ch=3):
        super().__init__()
        self.out_indices = list(out_indices)
        self.patch_embed = PatchEmbed(in_ch, embed_dim)
        dps = torch.linspace(0, drop_path_rate, sum(depths)).tolist()
        res, dim_in, ofs, chans = img_size // 4, embed_dim, 0, []
        for i, d in enumerate(depths):
            dim = embed_dim * 2 ** i
            if i > 0:
                res //= 2
            if i <= max(self.out_indices):   # timm's FeatureListNet drops every module after the last requested stage
                setattr(self, f"layers_{i}", SwinStage(dim_in, dim, res, d, heads[i], dps[ofs:ofs + d], i > 0))
            ofs, dim_in = ofs + d, dim
            chans.append(dim)
        self.feature_info = _FeatureInfo([chans[i] for i in self.out_indices])
        self.embed_spec = ConvSpec.conv2d(in_ch, embed_dim, 4, 4, 0)
        self.embed_lin = ConvSpec.linear(in_ch * 16, embed_dim)     # the same layer on patch rows [(ky, kx, c)] (sv_encoder_prep)

    def stages(self) -> List[SwinStage]:
        return [getattr(self, f"layers_{i}") for i in range(max(self.out_indices) + 1)]


class SwinTransformer(_Holder):
    def __init__(self, cfg, in_channels=3, img_size=224, pretrained=True, variant="tiny"):
        super().__init__()
        self.cfg, self.img_size = cfg, img_size
        if pretrained:
            logging.info("swinvox_amd: pretrained Swin weights are not fetched (offline); load a state_dict instead")
        stages = list(cfg.NETWORK.SWIN_T_STAGES)
        self.model = SwinBackbone(stages, img_size=img_size, in_ch=in_channels, **_VARIANTS[variant])
        self.out_channels = [self.model.feature_info.channels()[i] for i in range(len(stages))]
        self.out_spatial = [img_size // (4 * 2 ** i) for i in stages]
        self.layer_norm = nn.ModuleList([
            nn.LayerNorm([self.out_channels[i], self.out_spatial[i], self.out_spatial[i]]) for i in range(len(stages))])
        self.dropout = nn.Dropout(0.05)


# ---------------------------------------------------------------------------------------------------
# kernel chains
# ---------------------------------------------------------------------------------------------------
def _drop_scale(I, p, seed, like):
    sc = fempty(I, like=like)
    call("sv_droppath_scale", ptr(sc), I, float(p), int(seed), ops.seed_epoch_ptr())
    return sc


# What block_forward keeps for block_backward.  ln1, att, ln2 and h are tensors or, under store "mx" (LinearPlan.keep), the MX rows (bytes,
# scales) the forward GEMM consumed; a fused branch leaves the entries it does not store None.  packs: the fused MLP's bf16 weight images, when
# its backward reads them; fused_mlp: the fused MLP took the block (block_backward runs _fused_mlp_backward).
BlockTape = ops.named_tape("BlockTape", "x m1 r1 ln1 qkv att sc1 sc2 x1 m2 r2 ln2 hpre h I packs fused_mlp")
# What stage_forward keeps of the patch merging: its input, the norm's output (or its MX rows, store "mx") and statistics, the rows, Hin.
MergeTape = ops.named_tape("MergeTape", "x ln mean rstd rows Hin")


def _norm_for_linear(x, norm, rows, Cd, plan, save, merge_hw=(0, 0)):
    """The LayerNorm in front of a Swin linear (norm1 -> qkv, norm2 -> fc1, patch-merge norm -> reduction; plan: that linear's
    ops.swin_linear_plan) -> (ln, mean, rstd, xq).  plan.ln_emits: the LayerNorm kernel emits the quantised rows xq = (bytes, scales) itself, and
    without `save` (no backward follows) stores nothing else (ln, mean, rstd are None); otherwise xq is None and this is ops.layernorm_fwd.
    plan.keep: the tape will keep xq in place of ln, so ln comes back as None and xq always - an emitting LayerNorm does not write ln at all,
    otherwise ln is quantised here by the stand-alone quantiser and dropped."""
    if plan.ln_emits and plan.kind == "mx":
        ln, m, r, q, sq = ops.layernorm_quant_mx_fwd(x, norm.weight, norm.bias, rows, Cd, merge_hw=merge_hw, store=save, store_y=not plan.keep)
        return ln, m, r, (q, sq)
    if plan.ln_emits:
        ln, m, r, q, sq = ops.layernorm_quant_fwd(x, norm.weight, norm.bias, rows, Cd, merge_hw=merge_hw, store=save)
        return ln, m, r, (q, sq)
    ln, m, r = ops.layernorm_fwd(x, norm.weight, norm.bias, rows, Cd, merge_hw=merge_hw)
    if plan.keep:
        return None, m, r, ops.quantize_rows_mx(ln, rows, Cd)
    return ln, m, r, None


def block_forward(blk: SwinBlock, x, I, training, stochastic, seeds, save=True):
    """x [I*res*res, C] -> same shape; returns (out, ctx).  save=False (no backward will follow): the fused attention branch
    skips the tensors it would store for the backward.  ctx is a BlockTape.  Every unfused linear runs under its ops.swin_linear_plan, made
    before its input is produced: who quantises the rows, and whether the tape keeps them in place of the tensor (store "mx")."""
    H = W = blk.res
    Cd, M = blk.dim, I * H * W
    a, mlp = blk.attn, blk.mlp
    dp = blk.drop_path if (training and stochastic) else 0.0
    esz = 2.0 if x.dtype == torch.bfloat16 else 4.0
    if ops.fused_attn_block_enabled(Cd, blk.heads):
        # norm1 -> qkv -> window attention -> proj -> drop-path -> +x in ONE kernel; with save it also stores what the unfused backward reads
        sc1 = _drop_scale(I, dp, seeds(), x) if dp > 0 else None
        sc2 = _drop_scale(I, dp, seeds(), x) if dp > 0 else None
        x1 = empty(M, Cd, like=x)
        ln1 = qkv = att = m1 = r1 = None
        if save:
            ln1, qkv, att = empty(M, Cd, like=x), empty(M, 3 * Cd, like=x), empty(M, Cd, like=x)
            m1, r1 = fempty(M, like=x), fempty(M, like=x)
        # LayerNorm-free products of the branch: qkv + QK^T + PV + proj per token; bytes: x in, x1 out (+ the 5 saved rows when training)
        flops, nbytes = 2.0 * M * Cd * 4 * Cd + 4.0 * 49 * 32 * M * blk.heads, esz * M * Cd * (7 if save else 2)
        if ops.fused_attn_block_mx_enabled(Cd, blk.heads):
            # opt-in MXFP8 forward (set_fused_attn_block_mx): qkv and proj on MX operands, quantised in registers; same side outputs, so the
            # backward and the tape do not change
            images = ops.swin_attn_block_mx_packs(a.qkv.weight, a.proj.weight, Cd)
            ops.traced_call("sv_swin_attn_block_fwd_mx", flops, nbytes, ptr(x), ptr(blk.norm1.weight), ptr(blk.norm1.bias),
                            ptr(images), ptr(a.qkv.bias), ptr(a.relative_position_bias_table),
                            ptr(a.proj.bias), ptr(sc1), ptr(x1), ptr(ln1), ptr(m1), ptr(r1), ptr(qkv), ptr(att),
                            I, H, W, Cd, blk.heads, blk.shift, float(blk.norm1.eps), tag=f"M={M} C={Cd}")
        else:
            ops.traced_call("sv_swin_attn_block_fwd", flops, nbytes,
                            ptr(x), ptr(blk.norm1.weight), ptr(blk.norm1.bias), ptr(a.qkv.weight), ptr(a.qkv.bias), ptr(a.relative_position_bias_table),
                            ptr(a.proj.weight), ptr(a.proj.bias), ptr(sc1), ptr(x1), ptr(ln1), ptr(m1), ptr(r1), ptr(qkv), ptr(att),
                            I, H, W, Cd, blk.heads, blk.shift, float(blk.norm1.eps), tag=f"M={M} C={Cd}")
    else:
        # the fused attention backward reads ln1 and att as tensors: the branch then keeps its bf16 tape
        store_a = save and ops.linear_fp8_store() == "mx" and not ops.fused_attn_block_bwd_enabled(Cd, blk.heads)
        p_qkv = ops.swin_linear_plan(blk.s_qkv, a.qkv.weight, store_a, bias=a.qkv.bias)
        ln1, m1, r1, q1 = _norm_for_linear(x, blk.norm1, M, Cd, p_qkv, save)
        qkv = empty(M, 3 * Cd, like=x)
        ops.swin_linear_fwd(ln1, M, blk.s_qkv, a.qkv.weight, qkv, xq=q1, plan=p_qkv)
        sc1 = _drop_scale(I, dp, seeds(), x) if dp > 0 else None
        sc2 = _drop_scale(I, dp, seeds(), x) if dp > 0 else None
        p_proj = ops.swin_linear_plan(blk.s_proj, a.proj.weight, store_a, producer=True,
                                      bias=a.proj.bias, residual=x, ldr=Cd, row_scale=sc1, rows_per_scale=H * W)
        # algorithmic work of the core (49-token windows, no padding): QK^T + PV = 4 * 49 * 32 flop per (token, head); bytes: qkv in, out
        if p_proj.prod_emits:
            # MX recipe: the core emits the operand rows of proj (one head of a token = one block); without `save` att itself is not stored
            att, qa = (empty(M, Cd, like=x) if (save and not p_proj.keep) else None), ops.operand_buffers(M, Cd, True, x.device)
            ops.traced_call("sv_window_attention_fwd_mxq", 4.0 * 49 * 32 * M * blk.heads, (esz * (4 if save else 3) + 1) * M * Cd, ptr(qkv),
                            ptr(a.relative_position_bias_table), ptr(att), I, H, W, Cd, blk.heads, blk.shift, ops.attention_math(),
                            ptr(qa[0]), qa[0].shape[1], ptr(qa[1]), tag=f"M={M} C={Cd}")
        else:
            att, qa = empty(M, Cd, like=x), None
            ops.traced_call("sv_window_attention_fwd", 4.0 * 49 * 32 * M * blk.heads, esz * 4 * M * Cd, ptr(qkv), ptr(a.relative_position_bias_table),
                            ptr(att), I, H, W, Cd, blk.heads, blk.shift, ops.attention_math(), tag=f"M={M} C={Cd}")
            if p_proj.keep:
                qa = ops.quantize_rows_mx(att, M, Cd)
        x1 = empty(M, Cd, like=x)
        ops.swin_linear_fwd(att, M, blk.s_proj, a.proj.weight, x1, xq=qa, plan=p_proj)
        if p_qkv.keep:
            ln1 = q1
        if p_proj.keep:
            att = qa                                       # the tensor, where one was written, is dropped here
    if ops.fused_mlp_enabled(Cd):
        # norm2 -> fc1 -> GELU -> fc2 -> drop-path -> +x1 in ONE kernel; the 4C-wide hidden activation never reaches HBM
        mx = ops.fused_mlp_mx_enabled(Cd)
        packs = None
        # the bf16 images: read by sv_swin_mlp_fwd and by the fused bf16 backward (the MX data gradient packs its own operands; the weight
        # gradient reads pack_fwd / pack_dgrad, or the MX rows of the weights)
        if not mx or (save and not ops.fused_mlp_mx_bwd_enabled(Cd)):
            packs = torch.empty(16 * Cd * Cd, dtype=torch.bfloat16, device=x.device)
            call("sv_swin_mlp_pack", ptr(mlp.fc1.weight), ptr(mlp.fc2.weight), ptr(packs), Cd)
        x2 = empty(M, Cd, like=x)
        # opt-in MXFP8 forward (set_fused_mlp_mx): both products on MX operands, quantised in registers; the backward recomputes in bf16, or on
        # MX operands as well with set_fused_mlp_mx(True, backward=True)
        name, images = ("sv_swin_mlp_fwd_mx", ops.swin_mlp_mx_packs(mlp.fc1.weight, mlp.fc2.weight, Cd)) if mx else ("sv_swin_mlp_fwd", packs)
        ops.traced_call(name, 4.0 * M * Cd * 4 * Cd, 4.0 * M * Cd, ptr(x1), ptr(x2), ptr(blk.norm2.weight), ptr(blk.norm2.bias), ptr(images),
                        ptr(mlp.fc1.bias), ptr(mlp.fc2.bias), ptr(sc2), H * W, M, Cd, float(blk.norm2.eps), tag=f"M={M} C={Cd}")
        return x2, BlockTape(x, m1, r1, ln1, qkv, att, sc1, sc2, x1, None, None, None, None, None, I, packs, True)
    p_fc1 = ops.swin_linear_plan(blk.s_fc1, mlp.fc1.weight, save, bias=mlp.fc1.bias, act=ACT_GELU)
    ln2, m2, r2, q2 = _norm_for_linear(x1, blk.norm2, M, Cd, p_fc1, save)
    p_fc2 = ops.swin_linear_plan(blk.s_fc2, mlp.fc2.weight, save, producer=p_fc1,
                                 bias=mlp.fc2.bias, residual=x1, ldr=Cd, row_scale=sc2, rows_per_scale=H * W)
    # MX recipe: fc1 emits the operand rows of fc2 from its epilogue; without `save` neither h nor hpre is allocated or written
    emit = p_fc2.prod_emits
    hpre = h = None
    if save or not emit:
        hpre = empty(M, 4 * Cd, like=x)
        h = empty(M, 4 * Cd, like=x) if not (emit and p_fc2.keep) else None   # store "mx": fc1 writes hpre and the MX rows of h, not h
    qh = ops.swin_linear_fwd(ln2, M, blk.s_fc1, mlp.fc1.weight, h, xq=q2, emit=emit, plan=p_fc1, pre_act=hpre)
    if p_fc2.keep and not emit:
        qh = ops.quantize_rows_mx(h, M, 4 * Cd)
    x2 = empty(M, Cd, like=x)
    ops.swin_linear_fwd(h, M, blk.s_fc2, mlp.fc2.weight, x2, xq=qh, plan=p_fc2)
    return x2, BlockTape(x, m1, r1, ln1, qkv, att, sc1, sc2, x1, m2, r2, q2 if p_fc1.keep else ln2, hpre, qh if p_fc2.keep else h, I, None, False)


def block_backward(blk: SwinBlock, t: BlockTape, dx2, grads):
    """dx2 is consumed (used as the accumulator of the residual path); returns dx.  t.ln1, t.att, t.ln2 and t.h are tensors or, under store
    "mx", the MX rows (bytes, scales) the forward kept: ops.swin_linear_wgrad takes either."""
    H = W = blk.res
    Cd, M, mlp = blk.dim, t.I * H * W, blk.mlp
    # ---- MLP branch: x2 = x1 + s2 * fc2(gelu(fc1(ln2)))
    if t.fused_mlp:
        return _attention_backward(blk, t, _fused_mlp_backward(blk, t, dx2, grads), grads)
    dbr = dx2
    if t.sc2 is not None:
        dbr = empty(M, Cd, like=t.x)
        call("sv_rowscale", ptr(dx2), ptr(t.sc2), ptr(dbr), M, Cd, H * W)
    # without a drop-path copy dbr IS dx2, which the LayerNorm backward below updates in place -> keep this one in order
    ops.swin_linear_wgrad(dbr, t.h, M, blk.s_fc2, mlp.fc2.weight, grads[mlp.fc2.weight], grads[mlp.fc2.bias], async_ok=t.sc2 is not None)
    dh = empty(M, 4 * Cd, like=t.x)
    ops.swin_linear_dgrad(dbr, M, blk.s_fc2, mlp.fc2.weight, dh, act_grad_src=t.hpre, act_grad_kind=ACT_GELU)
    ops.swin_linear_wgrad(dh, t.ln2, M, blk.s_fc1, mlp.fc1.weight, grads[mlp.fc1.weight], grads[mlp.fc1.bias])
    dln2 = empty(M, Cd, like=t.x)
    ops.swin_linear_dgrad(dh, M, blk.s_fc1, mlp.fc1.weight, dln2)
    ops.layernorm_bwd(dln2, t.x1, blk.norm2.weight, t.m2, t.r2, dx2, grads[blk.norm2.weight], grads[blk.norm2.bias], M, Cd, accumulate_dx=True)
    return _attention_backward(blk, t, dx2, grads)


def _fused_mlp_backward(blk, t: BlockTape, dx2, grads):
    """Data gradient (dx1 = dx2 + branch gradient, LayerNorm parameter gradients) and weight gradients of the fused MLP branch:
    both recompute norm2 and the pre-activation from x1; the weight gradients run on the weight-gradient stream."""
    x1, sc2, mlp, Cd, HW = t.x1, t.sc2, blk.mlp, blk.dim, blk.res * blk.res
    M = t.I * HW
    unit = 2.0 * M * Cd * 4 * Cd
    eps = float(blk.norm2.eps)
    dx1 = empty(M, Cd, like=x1)
    # opt-in MXFP8 data gradient (set_fused_mlp_mx(True, backward=True)): the unfused MX backward chain of the branch in one kernel
    name, images = (("sv_swin_mlp_bwd_mx", ops.swin_mlp_mx_bwd_packs(mlp.fc1.weight, mlp.fc2.weight, Cd)) if ops.fused_mlp_mx_bwd_enabled(Cd)
                    else ("sv_swin_mlp_bwd", t.packs))
    ops.traced_call(name, 3 * unit, 6.0 * M * Cd, ptr(x1), ptr(dx2), ptr(dx1), ptr(blk.norm2.weight), ptr(blk.norm2.bias), ptr(images),
                    ptr(mlp.fc1.bias), ptr(sc2), HW, ptr(grads[blk.norm2.weight]), ptr(grads[blk.norm2.bias]), M, Cd, eps, tag=f"M={M} C={Cd}")
    # opt-in MXFP8 weight gradients (set_fused_mlp_mx(True, wgrad=True)): the unfused MX weight-gradient chain of the branch in one kernel, on the
    # MX rows of fc1.weight and of fc2.weight^T (the bytes of the unfused sites and of the other two MX kernels); the bf16 rows are not built
    if ops.fused_mlp_mx_wgrad_enabled(Cd):
        name = "sv_swin_mlp_wgrad_mx"
        operands = (*ops.quantize_weight_mx(mlp.fc1.weight), *ops.quantize_weight_t_mx(mlp.fc2.weight))
    else:
        name = "sv_swin_mlp_wgrad"
        operands = (blk.s_fc1.pack_fwd(mlp.fc1.weight), blk.s_fc2.pack_dgrad(mlp.fc2.weight))     # bf16 [4C][C] rows both

    def launch():
        ops.traced_call(name, 4 * unit, 4.0 * M * Cd, ptr(x1), ptr(dx2), ptr(blk.norm2.weight), ptr(blk.norm2.bias), *(ptr(o) for o in operands),
                        ptr(mlp.fc1.bias), ptr(sc2), HW, ptr(grads[mlp.fc1.weight]), ptr(grads[mlp.fc1.bias]),
                        ptr(grads[mlp.fc2.weight]), ptr(grads[mlp.fc2.bias]), M, Cd, eps, tag=f"M={M} C={Cd}")

    ops.run_on_wgrad_stream((x1, dx2, *operands), launch)
    return dx1


def _attention_backward(blk, t: BlockTape, dx1, grads):
    """x1 = x + s1 * proj(attn(qkv(ln1))): dx1 is consumed (accumulator of the residual path); returns dx."""
    x, qkv, sc1, m1, r1, I, a = t.x, t.qkv, t.sc1, t.m1, t.r1, t.I, blk.attn
    H = W = blk.res
    Cd, M = blk.dim, I * H * W
    esz = 2.0 if x.dtype == torch.bfloat16 else 4.0
    if ops.fused_attn_block_bwd_enabled(Cd, blk.heads):
        # data path in ONE kernel: dx1 -> projection data gradient -> attention backward (P recomputed) -> qkv data gradient -> LayerNorm
        # backward + residual; dqkv goes to HBM for the weight gradients, which stay on the engine (weight-gradient stream)
        dqkv, dx = empty(M, 3 * Cd, like=x), empty(M, Cd, like=x)
        dbr = empty(M, Cd, like=x) if sc1 is not None else None
        ws = ops.attn_bwd_workspace(blk.heads, x.device)
        ops.traced_call("sv_swin_attn_block_bwd", 2.0 * M * Cd * 4 * Cd + 10.0 * 49 * 32 * M * blk.heads, esz * M * Cd * (10 if sc1 is not None else 9),
                        ptr(dx1), ptr(qkv), ptr(x), ptr(m1), ptr(r1), ptr(blk.norm1.weight), ptr(a.qkv.weight), ptr(a.proj.weight),
                        ptr(a.relative_position_bias_table), ptr(sc1), ptr(dqkv), ptr(dx), ptr(dbr), ptr(grads[blk.norm1.weight]),
                        ptr(grads[blk.norm1.bias]), ptr(grads[a.relative_position_bias_table]), ptr(ws), I, H, W, Cd, blk.heads, blk.shift,
                        tag=f"M={M} C={Cd}")
        ops.linear_wgrad(dbr if dbr is not None else dx1, t.att, M, blk.s_proj, grads[a.proj.weight], grads[a.proj.bias])
        ops.linear_wgrad(dqkv, t.ln1, M, blk.s_qkv, grads[a.qkv.weight], grads[a.qkv.bias])
        return dx
    # ---- attention branch: x1 = x + s1 * proj(attn(qkv(ln1)))
    dbr = dx1
    if sc1 is not None:
        dbr = empty(M, Cd, like=x)
        call("sv_rowscale", ptr(dx1), ptr(sc1), ptr(dbr), M, Cd, H * W)
    ops.swin_linear_wgrad(dbr, t.att, M, blk.s_proj, a.proj.weight, grads[a.proj.weight], grads[a.proj.bias], async_ok=sc1 is not None)
    datt = empty(M, Cd, like=x)
    ops.swin_linear_dgrad(dbr, M, blk.s_proj, a.proj.weight, datt)
    dqkv = empty(M, 3 * Cd, like=x)
    ws = ops.attn_bwd_workspace(blk.heads, x.device)
    # backward = 2.5 x the forward products (recomputed P, dP, dQ, dK, dV); bytes: qkv + dout in, dqkv out
    ops.traced_call("sv_window_attention_bwd", 10.0 * 49 * 32 * M * blk.heads, esz * 7 * M * Cd, ptr(qkv), ptr(a.relative_position_bias_table),
                    ptr(datt), ptr(dqkv), ptr(grads[a.relative_position_bias_table]), ptr(ws), I, H, W, Cd, blk.heads, blk.shift,
                    ops.attention_bwd_math(), tag=f"M={M} C={Cd}")
    ops.swin_linear_wgrad(dqkv, t.ln1, M, blk.s_qkv, a.qkv.weight, grads[a.qkv.weight], grads[a.qkv.bias])
    dln1 = empty(M, Cd, like=x)
    ops.swin_linear_dgrad(dqkv, M, blk.s_qkv, a.qkv.weight, dln1)
    ops.layernorm_bwd(dln1, x, blk.norm1.weight, m1, r1, dx1, grads[blk.norm1.weight], grads[blk.norm1.bias], M, Cd, accumulate_dx=True)
    return dx1


def stage_forward(stage: SwinStage, x, I, training, stochastic, seeds, save=True):
    """One backbone stage (timm SwinTransformerStage: PatchMerging at the START of stages 1-3, then the blocks): x [I*Hin*Hin, Cin]
    -> ([I*res*res, dim], stage tape)."""
    sctx = {"merge": None, "blocks": []}
    if not isinstance(stage.downsample, nn.Identity):
        ds = stage.downsample
        Hin = stage.res * 2
        Mo = I * stage.res * stage.res
        plan = ops.swin_linear_plan(ds.spec, ds.reduction.weight, save)
        lnm, mm, rm, qm = _norm_for_linear(x, ds.norm, Mo, 2 * stage.dim, plan, save, merge_hw=(Hin, Hin))
        y = empty(Mo, stage.dim, like=x)
        ops.swin_linear_fwd(lnm, Mo, ds.spec, ds.reduction.weight, y, xq=qm, plan=plan)
        sctx["merge"] = MergeTape(x, qm if plan.keep else lnm, mm, rm, Mo, Hin)   # store "mx": the MX rows of the norm's output, not the tensor
        x = y
    for blk in stage.blocks:
        x, bctx = block_forward(blk, x, I, training, stochastic, seeds, save)
        sctx["blocks"].append(bctx)
    return x, sctx


def stage_backward(stage: SwinStage, sctx, dx, grads, I):
    """dx [I*res*res, dim] (consumed) -> gradient wrt the stage input [I*Hin*Hin, Cin]; parameter gradients accumulate into `grads`."""
    for blk, bctx in zip(reversed(list(stage.blocks)), reversed(sctx["blocks"])):
        dx = block_backward(blk, bctx, dx, grads)
    if sctx["merge"] is not None:
        ds = stage.downsample
        mt = sctx["merge"]
        ops.swin_linear_wgrad(dx, mt.ln, mt.rows, ds.spec, ds.reduction.weight, grads[ds.reduction.weight], None)
        dln = empty(mt.rows, 2 * stage.dim, like=dx)
        ops.swin_linear_dgrad(dx, mt.rows, ds.spec, ds.reduction.weight, dln)
        dxin = empty(I * mt.Hin * mt.Hin, stage.dim // 2, like=dx)
        ops.layernorm_bwd(dln, mt.x, ds.norm.weight, mt.mean, mt.rstd, dxin, grads[ds.norm.weight], grads[ds.norm.bias], mt.rows, 2 * stage.dim,
                          merge_hw=(mt.Hin, mt.Hin))
        dx = dxin
    return dx


def swin_forward(st: SwinTransformer, img_nhwc, I, training, stochastic, seeds, ready=None, save=True, *, patches=None):
    """img_nhwc [I,224,224,3] - or `patches` [I*56*56, 48], the 4 x 4 x 3 pixel blocks as rows [(ky, kx, c)] (sv_encoder_prep) - -> list of
    stage-head outputs [I*HW, C] (NHWC rows) + tape.  `ready` (optional list) receives one event per head output, recorded on the current
    stream as soon as that output is complete, so that another stream can consume the early stages while the later ones are still being
    computed."""
    bb = st.model
    pe = bb.patch_embed
    S = st.img_size
    Ce = pe.proj.out_channels
    M = I * (S // 4) ** 2
    src = patches if patches is not None else img_nhwc
    emb = empty(M, Ce, like=src)
    if patches is not None:
        # PatchEmbed's Conv2d(3, C, 4, 4) as a Linear(48, C) on the patch rows: weight [co][c][(ky, kx)] -> [co][(ky, kx)][c].  On the image the
        # layer gathers 3-channel (6-byte) taps on the engine's scalar path: 0.31 ms forward + 0.28 ms weight gradient at 512 images
        w48 = torch.empty(Ce, 48, dtype=torch.float32, device=src.device)
        ops.transpose(pe.proj.weight, w48, Ce, 3, 16)
        bb.embed_lin.forward(patches, M, (1, 1, 1), ops.pack_one(bb.embed_lin, w48, "f"), emb, bias=pe.proj.bias)
    else:
        wpe = bb.embed_spec.pack_fwd(pe.proj.weight)
        bb.embed_spec.forward(img_nhwc, I, (1, S, S), wpe, emb, bias=pe.proj.bias)
    x, pm, pr = ops.layernorm_fwd(emb, pe.norm.weight, pe.norm.bias, M, Ce)
    tape = {"embed": (src, emb, pm, pr, patches is not None), "stages": [], "heads": []}
    feats = []
    head_i = 0
    for si, stage in enumerate(bb.stages()):
        x, sctx = stage_forward(stage, x, I, training, stochastic, seeds, save)
        tape["stages"].append(sctx)
        if si in bb.out_indices:
            ln = st.layer_norm[head_i]
            Cs, Hs = stage.dim, stage.res
            L = Cs * Hs * Hs
            wt, bt = fempty(L, like=x), fempty(L, like=x)
            ops.transpose(ln.weight, wt, 1, Cs, Hs * Hs)       # [C,HW] -> [HW,C]
            ops.transpose(ln.bias, bt, 1, Cs, Hs * Hs)
            y = empty(I * Hs * Hs, Cs, like=x)
            mr = fempty(2 * I, like=x)
            ws = fempty(int(ops.hip.load().sv_ln_image_workspace_floats(I, L)), like=x)
            p = st.dropout.p if (training and stochastic) else 0.0
            seed = seeds() if p > 0 else 0
            call("sv_ln_image_fwd", ptr(x), ptr(wt), ptr(bt), ptr(y), ptr(mr), ptr(ws), I, L, float(ln.eps), float(p), seed, ops.seed_epoch_ptr())
            tape["heads"].append((si, head_i, x, wt, mr, p, seed, L))
            feats.append(y)
            if ready is not None:
                ev = torch.cuda.Event()
                ev.record()
                ready.append(ev)
            head_i += 1
    return feats, tape


def swin_backward(st: SwinTransformer, tape, dfeats, I, grads, ready=None, need_dx=False):
    """dfeats: list of gradients wrt the stage-head outputs ([I*HW, C]).
    `ready` (optional): one event per entry of dfeats, awaited right before that gradient is first read (the producer may
    still be working on the earlier stages' gradients on another stream).
    need_dx: also return the gradient wrt the patch rows, [I*(S/4)^2, 48] with columns (ky, kx, c) (sv_encoder_prep's xp layout; the
    same in both forward paths); else None."""
    bb = st.model
    stages = bb.stages()
    head_of = {si: (hi, xs, wt, mr, p, seed, L) for (si, hi, xs, wt, mr, p, seed, L) in tape["heads"]}
    dx = None
    for si in reversed(range(len(stages))):
        stage = stages[si]
        if si in head_of:
            hi, xs, wt, mr, p, seed, L = head_of[si]
            if ready is not None and ready[hi] is not None:
                torch.cuda.current_stream().wait_event(ready[hi])
            ln = st.layer_norm[hi]
            Cs, Hs = stage.dim, stage.res
            dxe = empty(I * Hs * Hs, Cs, like=xs)
            dwt, dbt = fzeros(L, like=xs), fzeros(L, like=xs)
            sums = torch.empty(2 * I, dtype=torch.float64, device=xs.device)
            call("sv_ln_image_bwd", ptr(dfeats[hi]), ptr(xs), ptr(wt), ptr(mr), ptr(dxe), ptr(dwt), ptr(dbt), ptr(sums), I, L, float(p), seed, ops.seed_epoch_ptr())
            ops.transpose(dwt, grads[ln.weight], 1, Hs * Hs, Cs)   # [HW,C] -> [C,HW]
            ops.transpose(dbt, grads[ln.bias], 1, Hs * Hs, Cs)
            if dx is None:
                dx = dxe
            else:
                call("sv_axpby", ptr(dx), ptr(dxe), ptr(dx), 1.0, 1.0, dx.numel())
        dx = stage_backward(stage, tape["stages"][si], dx, grads, I)
    # patch embed: LN backward, then conv weight/bias gradient (+ the data gradient on the patch rows when asked)
    img, emb, pm, pr, as_patches = tape["embed"]
    pe = bb.patch_embed
    M, Ce = emb.shape
    demb = empty(M, Ce, like=dx)
    ops.layernorm_bwd(dx, emb, pe.norm.weight, pm, pr, demb, grads[pe.norm.weight], grads[pe.norm.bias], M, Ce)
    S = st.img_size
    if as_patches:
        dw48 = torch.zeros(Ce, 48, dtype=torch.float32, device=dx.device)
        bb.embed_lin.wgrad(demb, img, M, (1, 1, 1), dw48, db=grads[pe.proj.bias])
        # the weight gradient went out on the weight-gradient stream: its way back to [co][c][(ky, kx)] follows it there (no wait: stream order)
        ops.run_on_wgrad_stream((dw48,), lambda: ops.transpose(dw48, grads[pe.proj.weight], Ce, 16, 3), wait=False)
    else:
        bb.embed_spec.wgrad(demb, img, I, (1, S, S), grads[pe.proj.weight], db=grads[pe.proj.bias])
    if not need_dx:
        return None
    # PatchEmbed's Conv2d(3, C, 4, 4) has stride = kernel: its data gradient is the Linear(48, C)'s on the patch rows, dxp = demb . w48
    w48 = torch.empty(Ce, 48, dtype=torch.float32, device=dx.device)
    ops.transpose(pe.proj.weight, w48, Ce, 3, 16)                         # [co][c][(ky, kx)] -> [co][(ky, kx)][c]
    dxp = empty(M, 48, like=dx)
    bb.embed_lin.dgrad(demb, M, (1, 1, 1), ops.pack_one(bb.embed_lin, w48, "d"), dxp)
    return dxp
