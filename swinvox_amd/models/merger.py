"""Merger on HIP kernels; mirrors reference models/merger.py:9-107.

forward(raw_features [B,V,9,32,32,32], coarse_volumes [B,V,32,32,32]) -> [B,32,32,32].
The six 3x3x3 convolutions work on channels-last data padded 9 -> 12 channels (16-byte channel vectors); layers 1-4
write straight into the 4x12-wide concat buffer that layer 5 reads.  Two kernel back-ends:
  * set_math("bf16"): the LDS-halo MFMA stencils of csrc/stencil.hip (brick + halo staged once in LDS);
  * set_math("f32") : the generic implicit-GEMM engine in exact fp32 (parity runs).
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from .. import ops
from ..ops import ACT_LRELU, BatchNormState, ConvSpec, call, empty, fzeros, ptr, zeros
from ._base import HipModule
from .decoder import VOX, as_channels_last12, raw_view

G = (32, 32, 32)


class _Layer(NamedTuple):
    """One of the six Conv3d(3x3x3) + BatchNorm + LeakyReLU layers as the kernels see it.  Layer 5 (concat) reads the 4 x 12-column concat."""
    conv: nn.Module
    bn: nn.Module
    spec: ConvSpec
    concat: bool       # layer 5: the input is the concat of the four 9-channel maps
    ldy: int           # row width of the conv output and of its activation outside the concat: 12 (9 channels + 3 pads); 1 for layer 6

    # what csrc/stencil.hip is told: channels loaded per voxel, 16-channel groups, output tile of the weight gradient, distance between the
    # concat's dense planes
    cin_load = property(lambda self: 48 if self.concat else 12)
    groups = property(lambda self: 3 if self.concat else 1)
    wgrad_tile = property(lambda self: 12 if self.concat else 16)

    def plane(self, I):
        return I * VOX * 12 if self.concat else 0


# one layer's forward: input and its row stride, conv output, BatchNormState
_LayerTape = ops.named_tape("_LayerTape", "x ldx y st")
MergerTape = ops.named_tape("MergerTape", "B V vol cat layers w5p wl out raw_dtype vol_dtype")


class Merger(HipModule):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        lk = cfg.NETWORK.LEAKY_VALUE
        self._slope = float(lk)

        def c3(cin, cout):
            return nn.Sequential(nn.Conv3d(cin, cout, kernel_size=3, padding=1), nn.BatchNorm3d(cout), nn.LeakyReLU(lk))

        self.layer1, self.layer2, self.layer3, self.layer4 = c3(9, 9), c3(9, 9), c3(9, 9), c3(9, 9)
        self.layer5 = c3(36, 9)
        self.layer6 = c3(9, 1)
        self._s14 = ConvSpec.conv3d(9, 9, 3, 1, 1, cin_mem=12, cout_mem=12)
        self._s5 = ConvSpec.conv3d(48, 9, 3, 1, 1, cin_mem=48, cout_mem=12)   # 36 real inputs spread over 4 x 12 columns
        self._s6 = ConvSpec.conv3d(9, 1, 3, 1, 1, cin_mem=12, cout_mem=4)
        self._layers = [_Layer(m[0], m[1], self._s14, False, 12) for m in (self.layer1, self.layer2, self.layer3, self.layer4)]
        self._layers += [_Layer(self.layer5[0], self.layer5[1], self._s5, True, 12), _Layer(self.layer6[0], self.layer6[1], self._s6, False, 1)]
        idx = torch.tensor([12 * g + j for g in range(4) for j in range(9)], dtype=torch.long)
        self.register_buffer("_cat_cols", idx, persistent=False)

    def forward(self, raw_features, coarse_volumes):
        assert raw_features.dim() == 6 and tuple(raw_features.shape[2:]) == (9, 32, 32, 32), "raw_features must be [B,V,9,32,32,32]"
        assert tuple(coarse_volumes.shape) == (raw_features.shape[0], raw_features.shape[1], 32, 32, 32)
        return self._run(raw_features, coarse_volumes)

    # ---- per-layer contraction dispatch ---------------------------------------------------------------
    def _w5_padded(self):
        w5 = self.layer5[0].weight                       # [9,36,3,3,3] -> [9,48,27] with the concat column map
        wp = fzeros(9, 48, 27, like=w5)
        wp[:, self._cat_cols] = w5.detach().reshape(9, 36, 27)
        return wp

    def _stencil_pack(self, L, dgrad):
        """bf16 weights for csrc/stencil.hip: forward [16][27][16G] (memory input channels), data-gradient
        [16*NT][27][16] (rows = memory channels of the conv input, taps flipped)."""
        w = L.conv.weight
        wp = torch.empty(16 * 27 * 16 * L.groups, dtype=torch.bfloat16, device=w.device)
        call("sv_merger_pack", ptr(w), ptr(wp), w.shape[0], w.shape[1], 1 if dgrad else 0, 1 if L.concat else 0)
        return wp

    def _conv_fwd(self, L, x, ldi, y, ldc, stats, w5p):
        conv, I = L.conv, y.shape[0] // VOX
        if ops.get_math() == "bf16":   # layer 5 reads the four dense 12-wide planes of the concat
            call("sv_stencil3_fwd", ptr(x), ldi, L.cin_load, L.groups, ptr(self._stencil_pack(L, False)), 1,
                 ptr(conv.bias), ptr(y), ldc, 0, conv.out_channels, None, 0, ptr(stats), I, 32, 32, 32, L.plane(I), 0)
        else:
            L.spec.forward(x, I, G, L.spec.pack_fwd(w5p if L.concat else conv.weight), y, ldi=ldi, ldc=ldc, bias=conv.bias, stats=stats)

    def _conv_dgrad(self, L, dy, lddy, dx, lddx, accumulate, w5p=None):
        conv, I = L.conv, dy.shape[0] // VOX
        if ops.get_math() == "bf16":
            call("sv_stencil3_fwd", ptr(dy), lddy, min(lddy, 12), 1, ptr(self._stencil_pack(L, True)), L.groups,
                 None, ptr(dx), lddx, 0, 48 if L.concat else 9, ptr(dx) if accumulate else None, lddx, None, I, 32, 32, 32, 0, L.plane(I))
        else:
            epi = dict(residual=dx, ldr=lddx) if accumulate else {}
            L.spec.dgrad(dy, I, G, L.spec.pack_dgrad(w5p if L.concat else conv.weight), dx, lddy=lddy, lddx=lddx, **epi)

    def _conv_wgrad(self, L, dy, lddy, x, ldx, grads):
        """weight gradient, and in bf16 math the conv bias gradient (column sums of dy) in the same stencil kernel; next to the generic engine
        the bias takes a column-sum kernel of its own, first"""
        conv, I = L.conv, dy.shape[0] // VOX
        if ops.get_math() == "bf16":
            ws = ops.zeros_f64(8 * conv.out_channels * conv.in_channels * 27, dy.device)   # 16 slot images of floats, zero on entry
            call("sv_stencil3_wgrad", ptr(x), ldx, L.cin_load, L.groups, ptr(dy), lddy, min(lddy, 12), ptr(grads[conv.weight]),
                 ptr(grads[conv.bias]), ptr(ws), conv.out_channels, conv.in_channels, L.wgrad_tile, 9, I, 32, 32, 32, L.plane(I))
            return
        ops.colsum(dy, dy.shape[0], conv.out_channels, lddy, grads[conv.bias])
        if L.concat:
            dw5p = fzeros(9, 48, 27, like=dy)
            L.spec.wgrad(dy, x, I, G, dw5p, lddy=lddy, ldx=ldx, async_ok=False)   # dw5p is read back right below
            grads[conv.weight].view(9, 36, 27).copy_(dw5p[:, self._cat_cols])
        else:
            L.spec.wgrad(dy, x, I, G, grads[conv.weight], lddy=lddy, ldx=ldx)

    # ---- forward / backward chains -------------------------------------------------------------------------
    def _fwd(self, raw, vol, save):
        B, V = raw.shape[:2]
        M, tr, sl = B * V * VOX, self.training, self._slope
        raw_dtype, vol_dtype = raw.dtype, vol.dtype
        x12 = ops.to_store(as_channels_last12(raw))
        vol = ops.to_store(vol)
        # the reference's torch.cat of the four 9-channel maps (merger.py:84) is never materialised: layers 1-4 write their
        # activations where layer 5 reads them.  Stencil back-end: four DENSE planes [4][M][12] (every per-layer pass streams
        # whole cache lines); generic fp32 engine: 12-column windows of 48-wide rows (one 48-channel input).
        planar = ops.get_math() == "bf16"
        # stencil back-end: every 12-wide row is written whole by its producer (9 channels + 3 zero pads: sv_stencil3_fwd and the
        # narrow BatchNorm kernels store complete 4-channel groups), so these buffers need no zero fill; the generic engine of the
        # fp32 mode writes the 9 real columns only
        cat = empty(4, M, 12, like=vol) if planar else zeros(M, 48, like=vol)
        ldcat = 12 if planar else 48
        w5p = self._w5_padded() if not planar else None
        layers, x, ldx = [], x12, 12
        for k, L in enumerate(self._layers):
            y = empty(M, L.ldy, like=vol)              # 9 channels + 3 pad columns: whole-row vector stores / loads
            st = BatchNormState(L.bn, M, tr)
            self._conv_fwd(L, x, ldx, y, L.ldy, st.sums, w5p)
            st.finalize()
            if k < 4:                                  # layers 1-4: into their slot of the concat
                z, ldz = (cat[k] if planar else cat[:, 12 * k:]), ldcat
            else:
                z, ldz = (empty if planar or k == 5 else zeros)(M, L.ldy, like=vol), L.ldy
            st.apply(y, L.ldy, z, ldz, ACT_LRELU, sl)
            layers.append(_LayerTape(x, ldx, y, st))
            x, ldx = (cat, ldcat) if k == 3 else (z, ldz)
        wl = x                                         # [M, 1]: the view weights
        out = empty(B, 32, 32, 32, like=vol)
        call("sv_merge_views_fwd", ptr(wl), ptr(vol), ptr(out), B, V, VOX)
        tape = MergerTape(B, V, vol, cat, layers, w5p, wl, out, raw_dtype, vol_dtype) if save else None
        return ops.to_f32(out), tape

    def _bwd(self, tape, grads, in_needs, dout):
        B, V, vol = tape.B, tape.V, tape.vol
        M, sl = B * V * VOX, self._slope
        dout = ops.to_store(dout)
        dwl = empty(M, 1, like=vol)
        dvol = empty(B, V, 32, 32, 32, like=vol)
        call("sv_merge_views_bwd", ptr(tape.wl), ptr(vol), ptr(tape.out), ptr(dout), ptr(dwl), ptr(dvol), B, V, VOX)
        planar = tape.cat.dim() == 3
        ldcat = 12 if planar else 48
        buf = empty if planar else zeros   # see _fwd: whole rows are written by the stencil / narrow kernels
        dz, lddz, dcat = dwl, 1, None
        for k in (5, 4, 3, 2, 1, 0):
            L, t = self._layers[k], tape.layers[k]
            lddy = L.spec.cout_mem          # 12; 4 for layer 6 (1 real column, padded for 16-byte gathers)
            dy = (zeros if k == 5 else buf)(M, lddy, like=vol)
            # z = None: the LeakyReLU mask is recomputed from the conv output (scale * y + shift > 0), one tensor read less in each of the two
            # BatchNorm backward passes
            t.st.backward(dz, lddz, None, 0, t.y, L.ldy, dy, lddy, grads[L.bn.weight], grads[L.bn.bias], ACT_LRELU, sl)
            self._conv_wgrad(L, dy, lddy, t.x, t.ldx, grads)
            if k == 4:      # data-gradient wrt the concat buffer, same storage scheme as `cat` (pad columns receive zero weights)
                dcat = empty(4, M, 12, like=vol) if planar else zeros(M, 48, like=vol)
            if k in (5, 0):
                dz, lddz = buf(M, 12, like=vol), 12
            else:           # the gradient of z_(k-1) lives in its slot of dcat; z_k feeds layer k+1 AND the concat: layers 4..2 add to the slot
                dz, lddz = (dcat[k - 1] if planar else dcat[:, 12 * (k - 1):]), ldcat
            self._conv_dgrad(L, dy, lddy, dcat if k == 4 else dz, lddz, 1 <= k <= 3, tape.w5p)
        dx = dz
        # gradients in the dtypes the inputs came in (raw_features arrives in the storage dtype from Decoder, fp32 from anyone else)
        draw = raw_view(dx if tape.raw_dtype == dx.dtype else ops.to_f32(dx), B, V) if in_needs[0] else None
        return (draw, (dvol if tape.vol_dtype == dvol.dtype else ops.to_f32(dvol)) if in_needs[1] else None)
