"""Bounding-box crops of ragged image batches on the device (swinvox_amd/data.py: augment_images -> sv_augment_images) against
tests/golden/bbox_crop_cases.npz: outputs of the reference's own transform lists at 40 x 48 and the padded crops it handed to its resize
(tests/golden/make_bbox_crop_golden.py).  Bounds are those of tests/test_gpu_data.py - the arithmetic after the geometry is the same
code: 5e-6 for the training list, 2e-6 for the validation list."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import swinvox_amd as S  # noqa: E402
from oracle import data as OD  # noqa: E402
from swinvox_amd import data as D  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "bbox_crop_cases.npz"))
NAMES = [str(n) for n in G["names"]]
OUT_H, OUT_W = (int(v) for v in G["out_hw"])


def cfg_at(h, w):
    cfg = S.default_cfg()
    cfg.CONST.IMG_H, cfg.CONST.IMG_W = h, w
    return cfg


def load_case(name, cfg):
    """(image, box, training list?, AugParams drawn as the loader would draw them after re-seeding)"""
    img = G["img_" + str(G[name + "_image"])]
    if img.ndim == 2:
        img = np.stack((img, ) * 3, -1)
    box = G[name + "_box"]
    box = None if box.size == 0 else [float(v) for v in box]
    train = bool(G[name + "_train"])
    np.random.seed(int(G[name + "_seeds"][0]))
    random.seed(int(G[name + "_seeds"][1]))
    p = D.draw_train_params(1, cfg, n_channels=img.shape[2], bounding_box=box) if train else D.val_params(1, cfg, n_channels=img.shape[2])
    return img, box, train, p


def by_channels(c):
    """the cases with c channels (a call shares C), a 37 x 53 image first so that every later image starts at an odd byte for C = 3"""
    names = [n for n in NAMES if G[n + "_crop"].shape[2] == c]
    return sorted(names, key=lambda n: G["img_" + str(G[n + "_image"])].size)


def check(got, name, train):
    want = G[name + "_out"]
    err = float(np.abs(got - want).max())
    assert got.shape == want.shape and err < (5e-6 if train else 2e-6), (name, err)


@pytest.mark.parametrize("channels", [3, 4])
def test_ragged_batch_matches_the_reference_outputs(dev, channels):
    cfg = cfg_at(OUT_H, OUT_W)
    names = by_channels(channels)
    cases = [load_case(n, cfg) for n in names]
    imgs, boxes, trains, params = (list(t) for t in zip(*cases))
    assert len({im.shape for im in imgs}) > 1 and any(b is None for b in boxes) and any(b is not None for b in boxes)
    starts = np.cumsum([0] + [im.size for im in imgs[:-1]])
    assert channels == 4 or (starts % 2 == 1).any()                # image starts that no wide load could use
    got = D.augment_images(imgs, boxes, params, cfg, device=dev)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(names), 1, 3, OUT_H, OUT_W)
    got = got.cpu().numpy()
    for i, n in enumerate(names):
        check(got[i, 0], n, trains[i])
    for i, n in enumerate(names):                                  # the same, one image per call
        one = D.augment_images([imgs[i]], [boxes[i]], [params[i]], cfg, device=dev).cpu().numpy()
        check(one[0, 0], n, trains[i])
        assert np.array_equal(one[0, 0], got[i, 0])                # an image's result does not depend on its neighbours or its offset


def test_greyscale_and_an_already_packed_device_buffer(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    names = by_channels(3)
    cases = [load_case(n, cfg) for n in names]
    imgs, boxes, trains, params = (list(t) for t in zip(*cases))
    want = D.augment_images(imgs, boxes, params, cfg, device=dev)
    packed = torch.from_numpy(np.concatenate([im.reshape(-1) for im in imgs])).to(dev)
    got = D.augment_images(packed, boxes, params, cfg, sizes=[im.shape for im in imgs])
    assert torch.equal(got, want)
    # a 2-D image is stacked to three channels, as the loader does (utils/data_loaders.py:194-196)
    _, box, train, p = load_case("grey_box", cfg)
    one = D.augment_images([G["img_grey"]], [box], [p], cfg, device=dev).cpu().numpy()
    check(one[0, 0], "grey_box", train)


def test_full_size_output_matches_the_restatement_on_the_recorded_crops(dev):
    """224 x 224, where no reference output is recorded: oracle.data.transform_views (pinned to the reference at 40 x 48 by
    tests/test_cpu_bbox_crop.py) on the crops the reference cut."""
    cfg = cfg_at(224, 224)
    for channels in (3, 4):
        names = by_channels(channels)
        cases = [load_case(n, cfg) for n in names]
        imgs, boxes, trains, params = (list(t) for t in zip(*cases))
        got = D.augment_images(imgs, boxes, params, cfg, device=dev).cpu().numpy()
        for i, (n, p) in enumerate(zip(names, params)):
            crop = G[n + "_crop"]
            ref = OD.transform_views(crop[None], dict(bg=np.asarray(p.bg), jitter_value=list(p.jitter_value), jitter_order=list(p.jitter_order),
                                                      noise_alpha=np.asarray(p.noise_alpha), flips=list(p.flips), perm=list(p.perm)),
                                     img_size=(224, 224), crop_size=(max(crop.shape[0], 224) + 1, max(crop.shape[1], 224) + 1))
            err = float(np.abs(got[i] - ref).max())
            assert err < (5e-6 if trains[i] else 2e-6), (n, err)


@pytest.mark.parametrize("shape", [(3, 137, 137, 4), (2, 150, 131, 3), (2, 100, 90, 4)])
def test_unboxed_equal_sizes_equal_augment_views_bit_for_bit(dev, shape):
    B, H, W, C = shape
    cfg = S.default_cfg()
    rng = np.random.default_rng(H + C)
    imgs = rng.integers(0, 256, size=(B, 1, H, W, C), dtype=np.uint8)
    if C == 4:
        imgs[..., 3] = np.where(rng.random((B, 1, H, W)) < 0.4, 0, 255)
    np.random.seed(5)
    random.seed(6)
    params = [D.draw_train_params(1, cfg, n_channels=C) for _ in range(B)]
    params[0].flips, params[0].perm = [True], [1, 2, 0]
    params[-1].flips = [False]
    dense = D.augment_views(torch.from_numpy(imgs).to(dev), params, cfg)
    ragged = D.augment_images([imgs[b, 0] for b in range(B)], None, params, cfg, device=dev)
    assert ragged.shape == dense.shape and torch.equal(ragged, dense)


def test_augment_images_argument_errors(dev):
    cfg = S.default_cfg()
    img = np.zeros((20, 30, 3), np.uint8)
    p = D.val_params(1, cfg, n_channels=3)
    with pytest.raises(ValueError, match="one AugParams"):
        D.augment_images([img], None, [p, p], cfg, device=dev)
    with pytest.raises(ValueError, match="one bounding box"):
        D.augment_images([img, img], [None], [p, p], cfg, device=dev)
    with pytest.raises(ValueError, match="empty"):
        D.augment_images([img], [(1.5, 0.2, 1.9, 0.6)], [p], cfg, device=dev)
    bad = D.val_params(1, cfg, n_channels=3)
    bad.perm = [0, 0, 1]
    with pytest.raises(ValueError, match="malformed"):
        D.augment_images([img], None, [bad], cfg, device=dev)
    two_views = D.val_params(2, cfg, n_channels=3)
    with pytest.raises(ValueError, match="malformed"):
        D.augment_images([img], None, [two_views], cfg, device=dev)
    with pytest.raises(RuntimeError, match="uint8"):
        D.augment_images([img.astype(np.float32)], None, [p], cfg, device=dev)
    with pytest.raises(RuntimeError, match="uint8"):
        D.augment_images([np.zeros((2, 3, 4, 3), np.uint8)], None, [p], cfg, device=dev)
    with pytest.raises(RuntimeError, match="same C"):
        D.augment_images([img, np.zeros((20, 30, 4), np.uint8)], None, [p, p], cfg, device=dev)
    with pytest.raises(RuntimeError, match="same C"):
        D.augment_images([np.zeros((20, 30, 2), np.uint8)], None, [p], cfg, device=dev)
    with pytest.raises(RuntimeError, match="GPU"):
        D.augment_images([img], None, [p], cfg, device="cpu")
    packed = torch.zeros(20 * 30 * 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="GPU"):
        D.augment_images(packed.cpu(), None, [p], cfg, sizes=[(20, 30, 3)])
    with pytest.raises(RuntimeError, match="1-D uint8"):
        D.augment_images(packed.view(20, 30, 3), None, [p], cfg, sizes=[(20, 30, 3)])
    with pytest.raises(RuntimeError, match="holds 1800 bytes"):
        D.augment_images(packed, None, [p], cfg, sizes=[(20, 31, 3)])
    with pytest.raises(RuntimeError, match=r"\(Hs, Ws, C\)"):
        D.augment_images(packed, None, [p], cfg, sizes=[(20, 30)])
    out = D.augment_images(packed, None, [p], cfg, sizes=[(20, 30, 3)])         # and the well-formed call goes through
    assert tuple(out.shape) == (1, 1, 3, 224, 224) and bool(torch.isfinite(out).all())
