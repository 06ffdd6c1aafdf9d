"""The binvox writer on the GPU (data.encode_binvox_batch -> sv_binvox_encode, harness.reconstruct): byte for byte the files the
reference's utils/binvox_rw.py writes (tests/golden/binvox_encode_cases.npz and binvox_cases.npz), zero-count pairs included, and
for generated volumes the closed form of that writer restated in test_cpu_binvox_encode.py (rle_pairs)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_binvox_encode import file_order, golden, payload_of, rle_pairs  # noqa: E402

import oracle as O  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import harness  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402

G_DEC = np.load(os.path.join(os.path.dirname(__file__), "golden", "binvox_cases.npz"))
CUBE32 = ("full32_holes", "long_exact", "half32", "sparse32")
SMALL = ("runs255_16", "tail255_8", "alt8", "noncubic")
DECODER_32 = ("empty32", "full32", "sparse32", "dense32", "slab32", "asym32")


def decoder_golden(name):
    dims = [int(d) for d in G_DEC[name + "_dims"]]
    return G_DEC[name + "_file"].tobytes(), np.unpackbits(G_DEC[name + "_xyz"])[:int(np.prod(dims))].astype(bool).reshape(dims)


def expected_files(xyz, translate=(0.0, 0.0, 0.0), scale=1.0):
    """xyz [B, a, b, c] (numpy bool) -> the files of the closed form, header dims (a, c, b)"""
    B, a, b, c = xyz.shape
    flat = file_order(xyz)
    return [D.binvox_header((a, c, b), translate, scale) + rle_pairs(flat[i]) for i in range(B)]


def test_reference_written_fixtures_byte_exact(dev):
    cases = [golden(n) for n in CUBE32]           # pair counts from 131 to 16 k in ONE call: the per-volume slicing of the payload
    got = D.encode_binvox_batch(torch.from_numpy(np.stack([c[1] for c in cases])).to(dev))
    for n, g, c in zip(CUBE32, got, cases):
        assert g == c[0], n
    for n in SMALL:
        raw, xyz, _ = golden(n)
        kw = dict(translate=(-0.5, 0.25, 0.0), scale=0.75) if n == "noncubic" else {}
        assert D.encode_binvox_batch(torch.from_numpy(xyz[None]).to(dev), **kw) == [raw], n
    dec = [decoder_golden(n) for n in DECODER_32]
    got = D.encode_binvox_batch(torch.from_numpy(np.stack([c[1] for c in dec])).to(dev))
    assert got == [c[0] for c in dec]
    raw, xyz = decoder_golden("cube16")
    assert D.encode_binvox_batch(torch.from_numpy(xyz[None]).to(dev)) == [raw]


def test_input_types_views_and_raw_order_give_the_same_bytes(dev):
    names = ("sparse32", "long_exact", "half32")
    want = [golden(n)[0] for n in names]
    xyz = torch.from_numpy(np.stack([golden(n)[1] for n in names])).to(dev)
    assert xyz.dtype == torch.bool and D.encode_binvox_batch(xyz) == want
    assert D.encode_binvox_batch(xyz.to(torch.uint8) * 7) == want              # any non-zero byte is a set voxel
    assert D.encode_binvox_batch(xyz.float() * -0.5) == want                   # any non-zero float too
    xzy = xyz.transpose(2, 3).contiguous()                                      # the file's own order
    view = xzy.transpose(2, 3)
    assert not view.is_contiguous() and D.encode_binvox_batch(view) == want
    wide = torch.zeros(3, 32, 32, 64, dtype=torch.float32, device=dev)
    wide[..., ::2] = xyz.float()
    assert D.encode_binvox_batch(wide[..., ::2]) == want
    assert D.encode_binvox_batch(xzy, fix_coords=False) == want                 # cubic: same header, same payload
    raw, nxyz, dims = golden("noncubic")
    nxzy = torch.from_numpy(np.ascontiguousarray(np.swapaxes(nxyz, 1, 2))[None]).to(dev)
    got = D.encode_binvox_batch(nxzy, fix_coords=False, translate=[(-0.5, 0.25, 0.0)], scale=[0.75])
    assert got == [raw] and list(nxzy.shape[1:]) == dims
    per = D.encode_binvox_batch(xyz, translate=[(0.0, 0.0, 0.0), (1.5, 2.0, -3.0), (0.0, 0.0, 0.0)], scale=[1.0, 0.25, 1.0])
    assert per[0] == want[0] and per[2] == want[2]
    assert per[1] == D.binvox_header((32, 32, 32), (1.5, 2.0, -3.0), 0.25) + payload_of(want[1])


def test_boundary_sweep(dev):
    """Volume p (16^3) has ones at file positions [p, p + 255) and [p + 256, p + 256 + 510): every run boundary and every 255-block
    boundary falls on every lane, wave and pass position of the 256-thread workgroup.  The kernel stages the volume in chunks of 1024
    voxels (four 256-voxel passes each), so the sweep runs to p = 1099 instead of 599: each of the boundaries p, p + 255, p + 256,
    p + 511 and p + 766 then also crosses the chunk edge at 1024, where the staged bit mask is replaced and the last value is carried."""
    P = 1100
    flat = np.zeros((P, 4096), bool)
    pos = np.arange(4096)[None, :] - np.arange(P)[:, None]
    flat[(pos >= 0) & (pos < 255)] = True
    flat[(pos >= 256) & (pos < 256 + 510)] = True
    xzy = flat.reshape(P, 16, 16, 16)
    want = [D.binvox_header((16, 16, 16)) + rle_pairs(f) for f in flat]
    xyz = torch.from_numpy(np.ascontiguousarray(np.swapaxes(xzy, 2, 3))).to(dev)
    got = D.encode_binvox_batch(xyz)                                           # one launch for the whole sweep
    bad = [p for p in range(P) if got[p] != want[p]]
    assert not bad, bad[:20]
    got = D.encode_binvox_batch(torch.from_numpy(xzy).to(dev), fix_coords=False)   # the untransposed staging path, same sweep
    bad = [p for p in range(P) if got[p] != want[p]]
    assert not bad, bad[:20]


@pytest.mark.parametrize("shape", [(32, 32, 32), (8, 24, 40)])
def test_round_trip_and_closed_form(dev, shape):
    rng = np.random.default_rng(5)
    xyz = np.stack([rng.random(shape) < p for p in (0.0, 0.02, 0.5, 0.98, 1.0)])
    v = torch.from_numpy(xyz).to(dev)
    files = D.encode_binvox_batch(v)
    assert files == expected_files(xyz)
    back = D.decode_binvox_batch(files, dev)
    assert back.shape == v.shape and torch.equal(back, v.float())
    raw = D.encode_binvox_batch(v, fix_coords=False)                           # the same array taken as file order
    assert [payload_of(f) for f in raw] == [rle_pairs(x) for x in xyz]
    assert torch.equal(D.decode_binvox_batch(raw, dev, fix_coords=False), v.float())


def test_threshold_mode_agrees_with_the_iou_kernel(dev):
    """logits = logit(th) +- (0.05 + |N(0, 1)|): no voxel lies within 0.05 logits of the decision boundary and none is excluded - a
    condition on the inputs that keeps a one-ulp expf difference between host and device from deciding a voxel, not a tolerance."""
    cfg = S.default_cfg()
    rng = np.random.default_rng(9)
    B = 2
    for th in cfg.TEST.VOXEL_THRESH:
        sign = np.where(rng.random((B, 32, 32, 32)) < 0.3, 1.0, -1.0)
        x = (math.log(th / (1.0 - th)) + sign * (0.05 + np.abs(rng.standard_normal((B, 32, 32, 32))))).astype(np.float32)
        occ = 1.0 / (1.0 + np.exp(-x.astype(np.float64))) >= th
        assert 0 < occ.sum() < occ.size
        xd = torch.from_numpy(x).to(dev)
        files = D.encode_binvox_batch(xd, threshold=th)
        assert files == expected_files(occ), th
        assert files == D.encode_binvox_batch(torch.from_numpy(occ).to(dev)), th
        counts = torch.empty(B, 1, 4, device=dev)
        ths = torch.tensor([th], dtype=torch.float32, device=dev)
        call("sv_iou_counts", ptr(xd), ptr(torch.zeros_like(xd)), ptr(ths), 1, B, 32768, ptr(counts))
        tp_fp = (counts[:, 0, 0] + counts[:, 0, 2]).tolist()
        assert D.decode_binvox_batch(files, dev).sum(dim=(1, 2, 3)).tolist() == tp_fp == occ.sum(axis=(1, 2, 3)).tolist(), th


def test_argument_errors(dev):
    v = torch.zeros(1, 4, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.encode_binvox_batch(v.cpu())
    with pytest.raises(RuntimeError, match="encode_binvox_batch expects"):
        D.encode_binvox_batch(v[0])                                            # rank 3
    with pytest.raises(RuntimeError, match="encode_binvox_batch expects"):
        D.encode_binvox_batch(v.double())
    with pytest.raises(RuntimeError, match="encode_binvox_batch expects"):
        D.encode_binvox_batch(v.to(torch.int32))
    for th in (0.0, 1.0, -0.2, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            D.encode_binvox_batch(v, threshold=th)
    for t in (v.bool(), v.to(torch.uint8)):
        with pytest.raises(ValueError, match="threshold"):
            D.encode_binvox_batch(t, threshold=0.5)
    with pytest.raises(ValueError, match="one per volume"):
        D.encode_binvox_batch(v, scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="one per volume"):
        D.encode_binvox_batch(v, translate=[(0.0, 0.0, 0.0)] * 3)


@pytest.mark.parametrize("use_refiner", [True, False])
def test_reconstruct(dev, use_refiner):
    """harness.reconstruct against forward_losses with the nets in eval(): bit-equal when two successive eval forwards are bit-equal
    to each other, within twice their difference otherwise.  On the MI355X the eval forward repeated bit for bit in both
    configurations, so the bit-equal branch is the one that held."""
    cfg = S.default_cfg()
    cfg.NETWORK.USE_REFINER = use_refiner
    nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
    for i, n in enumerate(nets):
        O.seeded_weights_(n, seed=3 + i)
        n.to(dev).train()
    nets[1].eval()                                                             # a mixed state: every mode has to come back as it was
    g = torch.Generator().manual_seed(2)
    x = (0.5 * torch.randn(1, 2, 3, 224, 224, generator=g)).to(dev)
    gt = (torch.rand(1, 32, 32, 32, generator=g) < 0.1).float().to(dev)
    before = {k: v.clone() for n in nets for k, v in n.state_dict().items() if "running" in k or "num_batches" in k}
    th = 0.3
    volume, files = harness.reconstruct(nets, cfg, x, binvox_threshold=th)
    assert [n.training for n in nets] == [True, False, True, True]
    after = {k: v for n in nets for k, v in n.state_dict().items() if "running" in k or "num_batches" in k}
    assert before and all(torch.equal(before[k], after[k]) for k in before)
    assert volume.shape == (1, 32, 32, 32) and volume.dtype == torch.float32 and not volume.requires_grad
    assert files == D.encode_binvox_batch(volume, threshold=th)
    assert D.decode_binvox_batch(files, dev).shape == (1, 32, 32, 32)
    plain = harness.reconstruct(nets, cfg, x)
    assert torch.is_tensor(plain) and plain.shape == volume.shape
    modes = [n.training for n in nets]
    for n in nets:
        n.eval()
    with torch.no_grad():
        v1, v2 = (harness.forward_losses(nets, cfg, x, gt)[3] for _ in range(2))
    for n, t in zip(nets, modes):
        n.train(t)
    spread = float((v1 - v2).abs().max())
    print(f"reconstruct (refiner {use_refiner}): eval forwards differ by {spread:.3e}, reconstruct vs forward_losses "
          f"{float((volume - v1).abs().max()):.3e}, repeat {float((plain - volume).abs().max()):.3e}")
    if spread == 0.0:
        assert torch.equal(volume, v1) and torch.equal(plain, v1)
    else:
        assert float((volume - v1).abs().max()) <= 2 * spread and float((plain - v1).abs().max()) <= 2 * spread
