"""Volume views on the GPU (data.render_views_batch -> sv_render_volumes, harness.reconstruct): the id buffer against the float32 numpy
restatement (tests/volume_view_ref.py) - equal is the target; at most max(2, 1e-4 H W) pixels of an image may differ, each carrying an id
the restatement has in its 3 x 3 neighbourhood of that pixel, the cap test_cpu_volume_view.py shows to hold between the restatement's
own float32 and float64 variants - and the colours against the shading rule applied to the kernel's own ids, exactly.

Measured on the MI355X when this was written: 0 differing pixels in every case below, the fixture cases at 640 x 480 included."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_view_ref as R  # noqa: E402
from test_cpu_volume_view import CASES, SIZE, cap, golden, golden_ids, silhouette_exceptions, small_cases, small_ids  # noqa: E402

import oracle as O  # noqa: E402
import swinvox_amd as S  # noqa: E402
from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import harness  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402


def compare_ids(got, want, size, what):
    """got, want int32 [..., H, W]: per image at most cap(size) pixels differ and each of those holds an id of want's 3 x 3 neighbourhood;
    prints and returns the number of differing pixels"""
    assert got.shape == want.shape and got.dtype == np.int32, (what, got.shape, want.shape)
    g, w = got.reshape((-1,) + tuple(size)), want.reshape((-1,) + tuple(size))
    worst, total = 0, 0
    for n in range(len(g)):
        diff = g[n] != w[n]
        k = int(diff.sum())
        worst, total = max(worst, k), total + k
        if k:
            assert k <= cap(size), (what, n, k)
            assert R.in_neighbourhood(g[n], w[n])[diff].all(), (what, n)
    print(f"{what}: ids differ from the float32 restatement in {total} pixels ({worst} at most in one of {len(g)} images of {size[0]} x {size[1]})")
    return total


def render(vols, cams, size, dev, **kw):
    rgb, ids = D.render_views_batch(torch.from_numpy(np.asarray(vols)).to(dev), cameras=cams, size=size, return_ids=True, **kw)
    assert rgb.dtype == torch.uint8 and ids.dtype == torch.int32 and rgb.is_cuda and ids.is_cuda
    assert tuple(rgb.shape) == (len(vols), len(cams), 3) + tuple(size) and tuple(ids.shape) == (len(vols), len(cams)) + tuple(size)
    return rgb.cpu().numpy(), ids.cpu().numpy()


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_ids_equal_the_restatement(dev, name):
    vols, cams, size = small_cases()[name]
    rgb, ids = render(vols, cams, size, dev)
    compare_ids(ids, small_ids(name), size, name)
    assert np.array_equal(rgb, R.shade(ids, D.VIEW_FACE_RGB))
    if name == "rand8_not_reached":
        assert (ids == -1).all() and (rgb == 255).all()


def test_default_camera_is_the_reference_view(dev):
    vols, cams, size = small_cases()["rand8"]
    t = torch.from_numpy(vols).to(dev)
    rgb, ids = D.render_views_batch(t, size=size, return_ids=True)
    assert tuple(rgb.shape) == (3, 1, 3) + size
    compare_ids(ids.cpu().numpy(), small_ids("rand8"), size, "cameras=None")
    assert torch.equal(D.render_views_batch(t, size=size), rgb)
    assert torch.equal(D.render_views_batch(t, cameras=[D.view_camera((8, 8, 8), size=size).reshape(18).tolist()], size=size), rgb)


def test_colours_follow_the_shading_rule(dev):
    vols, cams, size = small_cases()["rand5x7x3"]
    rng = np.random.default_rng(5)
    table = rng.integers(0, 256, size=(6, 3)).tolist()
    plate = rng.integers(0, 256, size=(3,) + size, dtype=np.uint8)
    rgb, ids = render(vols, cams, size, dev)
    assert (ids >= 0).any() and (ids < 0).any() and R.edge_mask(ids).any()
    assert np.array_equal(rgb, R.shade(ids, D.VIEW_FACE_RGB, (0, 0, 0), (255, 255, 255)))
    rgb2, ids2 = render(vols, cams, size, dev, face_colors=table, edge_color=(200, 10, 30), background=(7, 8, 9))
    assert np.array_equal(ids2, ids) and np.array_equal(rgb2, R.shade(ids, table, (200, 10, 30), (7, 8, 9)))
    rgb3, ids3 = render(vols, cams, size, dev, face_colors=table, background=torch.from_numpy(plate).to(dev))
    assert np.array_equal(ids3, ids) and np.array_equal(rgb3, R.shade(ids, table, (0, 0, 0), plate))


def test_batched_equals_one_by_one_and_input_types_agree(dev):
    vols, cams, size = small_cases()["rand8_three_cameras"]
    t = torch.from_numpy(vols).to(dev)
    rgb, ids = D.render_views_batch(t, cameras=cams, size=size, return_ids=True)
    for b in range(len(vols)):
        r1, i1 = D.render_views_batch(t[b:b + 1], cameras=cams, size=size, return_ids=True)
        assert torch.equal(r1[0], rgb[b]) and torch.equal(i1[0], ids[b])
    for c in range(len(cams)):
        r1, i1 = D.render_views_batch(t, cameras=cams[c:c + 1], size=size, return_ids=True)
        assert torch.equal(r1[:, 0], rgb[:, c]) and torch.equal(i1[:, 0], ids[:, c])
    assert t.dtype == torch.bool
    for other in (t.to(torch.uint8) * 7, t.float() * -0.5, t.float().transpose(1, 3).contiguous().transpose(1, 3)):
        r1, i1 = D.render_views_batch(other, cameras=cams, size=size, return_ids=True)
        assert torch.equal(r1, rgb) and torch.equal(i1, ids)


def test_threshold_mode_agrees_with_the_binvox_export(dev):
    """logits = logit(th) +- (0.05 + |N(0, 1)|), as in test_gpu_voxel_surface.py: no voxel lies within 0.05 logits of the decision boundary.
    Looking down -z orthographically with one pixel per voxel column, a column is hit iff the exported file has a voxel in it, and the
    hit voxel is the column's topmost, seen through its +z face."""
    cfg = S.default_cfg()
    rng = np.random.default_rng(9)
    B = 2
    cam = R.top_down_camera((32, 32, 32))
    for th in cfg.TEST.VOXEL_THRESH:
        sign = np.where(rng.random((B, 32, 32, 32)) < 0.02, 1.0, -1.0)
        x = (math.log(th / (1.0 - th)) + sign * (0.05 + np.abs(rng.standard_normal((B, 32, 32, 32))))).astype(np.float32)
        xd = torch.from_numpy(x).to(dev)
        _, ids = D.render_views_batch(xd, threshold=th, cameras=[cam], size=(32, 32), return_ids=True)
        ids = ids.cpu().numpy()[:, 0]
        back = D.decode_binvox_batch(D.encode_binvox_batch(xd, threshold=th), dev).cpu().numpy() != 0
        assert back.any(axis=3).any() and not back.any(axis=3).all()
        assert np.array_equal(ids >= 0, back.any(axis=3)), th
        top = 31 - np.argmax(back[..., ::-1], axis=3)
        i, j = np.indices((32, 32))
        want = np.where(back.any(axis=3), ((i * 32 + j)[None] * 32 + top) * 6 + 5, -1)
        assert np.array_equal(ids, want), th
        want32 = np.stack([R.render_ids(back[b], cam, (32, 32)) for b in range(B)])
        assert np.array_equal(ids, want32), th


def test_fixture_cases_at_full_size(dev):
    """the cases of equal dims in one launch each, at the reference's 640 x 480; the kernel's silhouettes against the recorded pictures"""
    for names in (("boxes", "sphere"), ("rand31x33x32",)):
        vols = np.stack([golden(n)[0] for n in names])
        assert names[0] in CASES
        rgb, ids = render(vols, [D.view_camera(vols.shape[1:])], SIZE, dev)
        compare_ids(ids[:, 0], np.stack([golden_ids(n) for n in names]), SIZE, " + ".join(names))
        for b, n in enumerate(names):
            _, img, plate, _, _ = golden(n)
            assert silhouette_exceptions(img, plate, ids[b, 0] >= 0) == (0, 0), n
        assert np.array_equal(rgb, R.shade(ids, D.VIEW_FACE_RGB))


def test_argument_errors(dev):
    v = torch.zeros(1, 4, 4, 4, device=dev)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.render_views_batch(v.cpu())
    for bad in (v[0], v.double(), v.to(torch.int32)):
        with pytest.raises(RuntimeError, match="render_views_batch expects"):
            D.render_views_batch(bad)
    for th in (0.0, 1.0, -0.2, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            D.render_views_batch(v, threshold=th)
    for t in (v.bool(), v.to(torch.uint8)):
        with pytest.raises(ValueError, match="threshold"):
            D.render_views_batch(t, threshold=0.5)
    with pytest.raises(ValueError, match="no volumes"):
        D.render_views_batch(v[:0])
    with pytest.raises(ValueError, match="1 .. 64"):
        D.render_views_batch(torch.zeros(1, 2, 65, 2, device=dev))
    for size in ((0, 8), (8, -1), (4097, 4096)):
        with pytest.raises(ValueError, match="size"):
            D.render_views_batch(v, size=size)
    for cams in ([], [np.zeros(17)], [np.zeros((6, 4))]):
        with pytest.raises(ValueError, match="cameras"):
            D.render_views_batch(v, cameras=cams, size=(8, 8))
    cam = D.view_camera((4, 4, 4), size=(8, 8))
    nan, inside = cam.copy(), cam.copy()
    nan[3, 1], inside[0] = float("nan"), (2.0, 2.0, 4.0)
    with pytest.raises(ValueError, match="not finite"):
        D.render_views_batch(v, cameras=[cam, nan], size=(8, 8))
    with pytest.raises(ValueError, match="inside or on"):
        D.render_views_batch(v, cameras=[inside], size=(8, 8))
    with pytest.raises(ValueError, match="face_colors"):
        D.render_views_batch(v, face_colors=[(0, 0, 0)] * 5, size=(8, 8))
    with pytest.raises(ValueError, match="edge_color"):
        D.render_views_batch(v, edge_color=(0, 0, 256), size=(8, 8))
    with pytest.raises(ValueError, match="plate"):
        D.render_views_batch(v, background=torch.zeros(3, 8, 9, dtype=torch.uint8, device=dev), size=(8, 8))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.render_views_batch(v, background=torch.zeros(3, 8, 8, dtype=torch.uint8), size=(8, 8))


def test_reconstruct_with_views(dev):
    cfg = S.default_cfg()
    nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
    for i, n in enumerate(nets):
        O.seeded_weights_(n, seed=3 + i)
        n.to(dev).eval()
    g = torch.Generator().manual_seed(2)
    x = (0.5 * torch.randn(1, 2, 3, 224, 224, generator=g)).to(dev)
    plain = harness.reconstruct(nets, cfg, x)
    assert torch.is_tensor(plain)
    size = (90, 120)
    volume, views = harness.reconstruct(nets, cfg, x, view_threshold=0.5, view_size=size)
    assert torch.equal(volume, plain)
    assert views.dtype == torch.uint8 and tuple(views.shape) == (1, 1, 3) + size and views.is_cuda
    rgb, ids = D.render_views_batch(volume, 0.5, size=size, return_ids=True)
    assert torch.equal(views, rgb)
    back = D.decode_binvox_batch(D.encode_binvox_batch(volume, threshold=0.5), dev)[0].cpu().numpy() != 0
    compare_ids(ids.cpu().numpy()[0, 0], R.render_ids(back, R.view_camera((32, 32, 32), size=size), size), size, "reconstruct")
    cams = [D.view_camera((32, 32, 32), 30, a, size) for a in (45, 135)]
    three = harness.reconstruct(nets, cfg, x, binvox_threshold=0.4, view_threshold=0.5, view_size=size, view_cameras=cams)
    assert len(three) == 3 and torch.equal(three[0], plain) and three[1] == D.encode_binvox_batch(volume, threshold=0.4)
    assert tuple(three[2].shape) == (1, 2, 3) + size and torch.equal(three[2][:, 0], views[:, 0])
    assert D.image_file(views[0, 0]).startswith(b"\x89PNG")
