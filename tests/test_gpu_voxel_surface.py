"""The exposed-voxel-face mesh on the GPU (data.extract_surface_batch / encode_mesh_batch -> sv_voxel_surface, harness.reconstruct):
vertices and faces element for element what the numpy restatement (tests/voxel_surface_ref.py) gives - the order is specified, so
nothing is sorted and there is no tolerance - and, for the fixtures, the face sets matplotlib's Axes3D.voxels built
(tests/golden/voxel_surface_cases.npz), which is what the reference draws (utils/helpers.py:50-88)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_cpu_voxel_surface import CASES, ONE_FACES, ONE_VERTS, PARSERS, golden  # noqa: E402
from voxel_surface_ref import canonical_faces, revoxelise, surface  # noqa: E402

import oracle as O  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import harness  # noqa: E402
from swinvox_amd.hip import call, ptr  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402


def check(vols, dev, what=""):
    """bool [B, a, b, c] through ONE call; every volume's verts and faces equal the restatement's.  Returns the meshes."""
    vols = np.asarray(vols)
    got = D.extract_surface_batch(torch.from_numpy(vols).to(dev))
    assert len(got) == len(vols)
    bad = []
    for i, ((v, f), vol) in enumerate(zip(got, vols)):
        wv, wf = surface(vol)
        assert v.dtype == np.int32 and f.dtype == np.int32 and v.ndim == 2 and f.ndim == 2
        if v.shape != wv.shape or f.shape != wf.shape or not np.array_equal(v, wv) or not np.array_equal(f, wf):
            bad.append((i, v.shape, wv.shape, f.shape, wf.shape))
    assert not bad, (what, bad[:10])
    return got


def test_fixtures_match_matplotlib(dev):
    for name in CASES:
        vol, faces = golden(name)
        (v, f), = check(vol[None], dev, name)
        assert np.array_equal(canonical_faces(v[f]), faces), name
    (v, f), = check(np.ones((1, 1, 1, 1), bool), dev)
    assert v.tolist() == ONE_VERTS and f.tolist() == ONE_FACES


def test_named_shapes_32(dev):
    x, y, z = np.indices((32, 32, 32))
    board = (x + y + z) % 2 == 0
    corners = np.zeros((8, 32, 32, 32), bool)
    for n in range(8):
        corners[n, 31 * (n >> 2), 31 * ((n >> 1) & 1), 31 * (n & 1)] = True
    vols = np.concatenate([np.zeros((1, 32, 32, 32), bool), np.ones((1, 32, 32, 32), bool), corners, board[None], ~board[None]])
    got = check(vols, dev, "32^3")
    sizes = [(len(v), len(f)) for v, f in got]
    assert sizes[0] == (0, 0) and sizes[1] == (6146, 6144) and sizes[2:10] == [(8, 6)] * 8
    assert sizes[10] == (35933, 98304) and sizes[11] == (35933, 98304)                 # capacities: 35 937 vertices, 101 376 faces


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 64), (64, 1, 1), (4, 6, 10), (31, 33, 32)])
def test_named_shapes_odd(dev, shape):
    rng = np.random.default_rng(sum(shape))
    check(np.stack([np.ones(shape, bool), rng.random(shape) < 0.5, rng.random(shape) < 0.1]), dev, shape)


def test_named_shapes_64(dev):
    rng = np.random.default_rng(64)
    (v, f), = check((rng.random((1, 64, 64, 64)) < 0.02), dev, "64^3 at 2 %")
    assert len(f) > 6 * 4000
    (v, f), = check(np.ones((1, 64, 64, 64), bool), dev, "64^3 full")
    assert (len(v), len(f)) == (6 * 64 * 64 + 2, 6 * 64 * 64)


def test_sweep(dev):
    """One launch of 1 024 volumes of 8^3: a single filled voxel at every position, and its complement - every boundary, lane and
    mask-word position occurs (lattice rows are 9 points long, so the vertex runs straddle the 32-bit words at every offset).  Then
    64 volumes of 16^3 at densities 0 ... 1."""
    eye = np.eye(512, dtype=bool).reshape(512, 8, 8, 8)
    got = check(np.concatenate([eye, ~eye]), dev, "8^3 sweep")
    assert all((len(v), len(f)) == (8, 6) for v, f in got[:512])
    rng = np.random.default_rng(16)
    check(np.stack([rng.random((16, 16, 16)) < n / 63.0 for n in range(64)]), dev, "16^3 densities")


def test_input_types_give_the_same_mesh(dev):
    rng = np.random.default_rng(7)
    occ = rng.random((3, 12, 20, 9)) < 0.4
    want = check(occ, dev)
    t = torch.from_numpy(occ).to(dev)
    assert t.dtype == torch.bool
    for other in (t.to(torch.uint8) * 7, t.float() * -0.5, t.float().transpose(1, 3).contiguous().transpose(1, 3)):
        got = D.extract_surface_batch(other)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got, want))


def test_threshold_mode_agrees_with_binvox_export_and_iou(dev):
    """logits = logit(th) +- (0.05 + |N(0, 1)|): no voxel lies within 0.05 logits of the decision boundary and none is excluded - a
    condition on the inputs that keeps a one-ulp expf difference between host and device from deciding a voxel, not a tolerance."""
    cfg = S.default_cfg()
    rng = np.random.default_rng(9)
    B = 2
    for th in cfg.TEST.VOXEL_THRESH:
        sign = np.where(rng.random((B, 32, 32, 32)) < 0.3, 1.0, -1.0)
        x = (math.log(th / (1.0 - th)) + sign * (0.05 + np.abs(rng.standard_normal((B, 32, 32, 32))))).astype(np.float32)
        occ = 1.0 / (1.0 + np.exp(-x.astype(np.float64))) >= th
        xd = torch.from_numpy(x).to(dev)
        meshes = D.extract_surface_batch(xd, threshold=th)
        back = D.decode_binvox_batch(D.encode_binvox_batch(xd, threshold=th), dev).cpu().numpy() != 0
        counts = torch.empty(B, 1, 4, device=dev)
        ths = torch.tensor([th], dtype=torch.float32, device=dev)
        call("sv_iou_counts", ptr(xd), ptr(torch.zeros_like(xd)), ptr(ths), 1, B, 32768, ptr(counts))
        tp_fp = (counts[:, 0, 0] + counts[:, 0, 2]).tolist()
        for b, (v, f) in enumerate(meshes):
            inside = revoxelise(v, f, (32, 32, 32))                                    # from the +-z faces, by column parity
            assert np.array_equal(inside, back[b]), th
            assert int(inside.sum()) == tp_fp[b], th
            wv, wf = surface(occ[b])
            assert np.array_equal(v, wv) and np.array_equal(f, wf), th


def test_batched_equals_one_by_one(dev):
    x, y, z = np.indices((24, 24, 24))
    rng = np.random.default_rng(3)
    vols = np.stack([np.zeros((24, 24, 24), bool), rng.random((24, 24, 24)) < 0.03, (x + y + z) % 2 == 0, rng.random((24, 24, 24)) < 0.5])
    t = torch.from_numpy(vols).to(dev)
    batched = check(vols, dev)
    assert len({len(f) for _, f in batched}) == 4                                      # four payload lengths, trimmed to the longest
    for b in range(4):
        (v, f), = D.extract_surface_batch(t[b:b + 1])
        assert v.tobytes() == batched[b][0].tobytes() and f.tobytes() == batched[b][1].tobytes()
    for fmt in ("ply", "off", "obj"):
        files = D.encode_mesh_batch(t, fmt=fmt)
        assert files == [D.mesh_file(v, f, fmt) for v, f in batched]
        assert files == [D.encode_mesh_batch(t[b:b + 1], fmt=fmt)[0] for b in range(4)]
    xyz, quads = PARSERS["ply"](D.encode_mesh_batch(t, translate=[(0.0, 0.0, 0.0), (1.5, 2.0, -3.0)] * 2, scale=[1.0, 0.25] * 2)[1])
    assert np.array_equal(quads, batched[1][1])
    assert np.array_equal(xyz, (np.asarray((1.5, 2.0, -3.0))[None] + 0.25 * batched[1][0].astype(np.float64) / 24.0).astype(np.float32))


def test_argument_errors(dev):
    v = torch.zeros(1, 4, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.extract_surface_batch(v.cpu())
    for bad in (v[0], v.double(), v.to(torch.int32)):
        with pytest.raises(RuntimeError, match="extract_surface_batch expects"):
            D.extract_surface_batch(bad)
    for th in (0.0, 1.0, -0.2, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            D.extract_surface_batch(v, threshold=th)
    for t in (v.bool(), v.to(torch.uint8)):
        with pytest.raises(ValueError, match="threshold"):
            D.extract_surface_batch(t, threshold=0.5)
    with pytest.raises(ValueError, match="no volumes"):
        D.extract_surface_batch(v[:0])
    with pytest.raises(ValueError, match="1 .. 64"):
        D.extract_surface_batch(torch.zeros(1, 2, 65, 2, device=dev))
    with pytest.raises(ValueError, match="one per volume"):
        D.encode_mesh_batch(v, scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="format"):
        D.encode_mesh_batch(v, fmt="stl")


def test_reconstruct_with_meshes(dev):
    cfg = S.default_cfg()
    nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
    for i, n in enumerate(nets):
        O.seeded_weights_(n, seed=3 + i)
        n.to(dev).eval()
    g = torch.Generator().manual_seed(2)
    x = (0.5 * torch.randn(1, 2, 3, 224, 224, generator=g)).to(dev)
    plain = harness.reconstruct(nets, cfg, x)
    assert torch.is_tensor(plain)
    volume, meshes = harness.reconstruct(nets, cfg, x, mesh_threshold=0.5)
    assert torch.equal(volume, plain)
    assert meshes == D.encode_mesh_batch(volume, 0.5) and len(meshes) == 1 and meshes[0].startswith(b"ply\n")
    xyz, quads = PARSERS["ply"](meshes[0])
    wv, wf = D.extract_surface_batch(volume, 0.5)[0]
    assert np.array_equal(xyz, wv.astype(np.float32)) and np.array_equal(quads, wf)
    back = D.decode_binvox_batch(D.encode_binvox_batch(volume, threshold=0.5), dev)[0].cpu().numpy() != 0
    assert np.array_equal(revoxelise(wv, wf, (32, 32, 32)), back)                      # the faces of the voxels the binvox export holds
    rv, rf = surface(back)
    assert np.array_equal(wv, rv) and np.array_equal(wf, rf)
    three = harness.reconstruct(nets, cfg, x, binvox_threshold=0.4, mesh_threshold=0.5, mesh_format="off")
    assert len(three) == 3 and torch.equal(three[0], plain)
    assert three[1] == D.encode_binvox_batch(volume, threshold=0.4) and three[2] == D.encode_mesh_batch(volume, 0.5, fmt="off")
    two = harness.reconstruct(nets, cfg, x, binvox_threshold=0.4)
    assert len(two) == 2 and two[1] == three[1]
