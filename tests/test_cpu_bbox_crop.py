"""Host side of the bounding-box crop (swinvox_amd/data.py: bbox_crop_rect, draw_train_params(bounding_box=...), sv_augment_images'
descriptor checks) against tests/golden/bbox_crop_cases.npz, which the reference's own utils/data_transforms.py produced
(tests/golden/make_bbox_crop_golden.py).  The same fixture pins oracle.data.transform_views: applied to the crop the reference handed
to its resize, it must reproduce the reference's output element for element."""
import ctypes
import os
import random

import numpy as np
import pytest

import swinvox_amd as S
from oracle import data as OD
from swinvox_amd import data as D
from swinvox_amd import hip

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "bbox_crop_cases.npz"))
NAMES = [str(n) for n in G["names"]]
OUT_H, OUT_W = (int(v) for v in G["out_hw"])


def cfg_small():
    cfg = S.default_cfg()
    cfg.CONST.IMG_H, cfg.CONST.IMG_W = OUT_H, OUT_W
    return cfg


def load_case(name):
    img = G["img_" + str(G[name + "_image"])]
    if img.ndim == 2:
        img = np.stack((img, ) * 3, -1)
    box = G[name + "_box"]
    return img, (None if box.size == 0 else [float(v) for v in box]), bool(G[name + "_train"]), [int(s) for s in G[name + "_seeds"]]


def draw(name, cfg):
    """the case's AugParams, drawn as the loader would: re-seed, then the training draws or the validation parameters"""
    img, box, train, seeds = load_case(name)
    np.random.seed(seeds[0])
    random.seed(seeds[1])
    if train:
        return D.draw_train_params(1, cfg, n_channels=img.shape[2], bounding_box=box)
    return D.val_params(1, cfg, n_channels=img.shape[2])


def oracle_prm(p):
    return dict(bg=np.asarray(p.bg), jitter_value=list(p.jitter_value), jitter_order=list(p.jitter_order), noise_alpha=np.asarray(p.noise_alpha),
                flips=list(p.flips), perm=list(p.perm))


def test_the_fixture_holds_the_cases_that_matter():
    shapes = {n: G[n + "_crop"].shape[:2] for n in NAMES}
    assert shapes["inside"] == (27, 28) and shapes["tiny"] == (3, 4) and shapes["zero_area"] == (1, 1) and shapes["big_full"] == (201, 201)
    assert {G[n + "_crop"].shape[2] for n in NAMES} == {3, 4}
    assert any(G[n + "_box"].size == 0 for n in NAMES) and any(bool(G[n + "_train"]) for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_crop_integers_and_edge_padding_are_the_references(name):
    cfg = cfg_small()
    img, box, train, _ = load_case(name)
    p = draw(name, cfg)
    assert (p.crop_draws is not None) == (train and box is not None)
    xl, xr, yt, yb, pl, pr, pt, pb = D.bbox_crop_rect(img.shape[0], img.shape[1], box, p.crop_draws, (cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W))
    want = G[name + "_crop"]
    assert (pt + (yb - yt + 1) + pb, pl + (xr - xl + 1) + pr) == want.shape[:2]
    assert 0 <= xl <= xr < img.shape[1] and 0 <= yt <= yb < img.shape[0] and min(pl, pr, pt, pb) >= 0
    got = np.pad(img[yt:yb + 1, xl:xr + 1], ((pt, pb), (pl, pr), (0, 0)), mode="edge")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", NAMES)
def test_transform_restatement_equals_the_reference_on_the_recorded_crop(name):
    cfg = cfg_small()
    p = draw(name, cfg)
    crop = G[name + "_crop"]
    big = (max(crop.shape[0], OUT_H) + 1, max(crop.shape[1], OUT_W) + 1)          # crop_size above the crop: it is not cropped again
    got = OD.transform_views(crop[None], oracle_prm(p), img_size=(OUT_H, OUT_W), crop_size=big, mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD)
    assert got.shape == (1, 3, OUT_H, OUT_W)
    assert np.array_equal(got[0], G[name + "_out"]), float(np.abs(got[0] - G[name + "_out"]).max())


def test_truncation_is_toward_zero_and_a_touching_edge_pads_one():
    # raw x_left = -0.5 -> int() gives 0 and no pad (a floor would give -1 and one padded column)
    xl, xr, yt, yb, pl, pr, pt, pb = D.bbox_crop_rect(37, 53, (-0.5 / 53, 0.3, 0.6, 0.7))
    assert (xl, pl) == (0, 0) and xr == 31
    # x_right = 53.0 == img_width -> clamped to 52, pad_r = 1
    xl, xr, yt, yb, pl, pr, pt, pb = D.bbox_crop_rect(37, 53, (0.5, 0.4, 1.0, 0.6))
    assert (xl, xr, pl, pr) == (26, 52, 0, 1)
    # without a box: centre crop only when the image is larger than the crop size in BOTH directions (the rule of sv_augment_views)
    assert D.bbox_crop_rect(150, 200, None, None, (128, 128)) == (36, 163, 11, 138, 0, 0, 0, 0)
    assert D.bbox_crop_rect(150, 128, None, None, (128, 128)) == (0, 127, 0, 149, 0, 0, 0, 0)
    assert D.bbox_crop_rect(37, 53) == (0, 52, 0, 36, 0, 0, 0, 0)
    # the jitter: scale 1 and four 0.5 are the validation crop
    assert D.bbox_crop_rect(37, 53, (0.2, 0.3, 0.7, 0.8), [1.0, .5, .5, .5, .5]) == D.bbox_crop_rect(37, 53, (0.2, 0.3, 0.7, 0.8))


def test_draws_without_a_box_are_the_draws_of_today():
    cfg = S.default_cfg()
    for n_channels in (3, 4):
        for n_views in (1, 3):
            np.random.seed(7)
            random.seed(8)
            p = D.draw_train_params(n_views, cfg, n_channels=n_channels)
            state_np, state_py = np.random.get_state(), random.getstate()
            assert p.crop_draws is None
            # the same draws spelled out (data.draw_train_params before it knew about boxes)
            np.random.seed(7)
            random.seed(8)
            o = OD.draw_train_params(n_views, dict(RANDOM_BG_COLOR_RANGE=cfg.TRAIN.RANDOM_BG_COLOR_RANGE, BRIGHTNESS=cfg.TRAIN.BRIGHTNESS,
                                                   CONTRAST=cfg.TRAIN.CONTRAST, SATURATION=cfg.TRAIN.SATURATION, NOISE_STD=cfg.TRAIN.NOISE_STD),
                                     n_channels=n_channels)
            assert np.array_equal(np.random.get_state()[1], state_np[1]) and np.random.get_state()[2:] == state_np[2:]
            assert random.getstate() == state_py
            assert list(p.jitter_value) == list(o["jitter_value"]) and list(p.flips) == o["flips"] and list(p.perm) == o["perm"]
    # with a box: five random.uniform first, nothing else moves in np.random
    np.random.seed(7)
    random.seed(8)
    p = D.draw_train_params(1, cfg, n_channels=3, bounding_box=(0.1, 0.1, 0.9, 0.9))
    random.seed(8)
    want = [random.uniform(0.8, 1.2)] + [random.uniform(.4, .6) for _ in range(4)]
    assert list(p.crop_draws) == want and bool(random.randint(0, 1)) == p.flips[0]
    np.random.seed(7)
    q = D.draw_train_params(1, cfg, n_channels=3)
    assert list(q.jitter_value) == list(p.jitter_value) and list(q.perm) == list(p.perm)


def test_refusals_of_the_host_layer():
    cfg = S.default_cfg()
    with pytest.raises(ValueError, match="empty"):
        D.bbox_crop_rect(37, 53, (1.5, 0.2, 1.9, 0.6))                              # entirely to the right of the image
    with pytest.raises(ValueError, match="empty"):
        D.bbox_crop_rect(37, 53, (0.2, -0.9, 0.6, -0.5))                            # entirely above it
    with pytest.raises(ValueError, match="empty"):
        D.bbox_crop_rect(37, 53, (0.8, 0.8, 0.2, 0.2))                              # negative extent
    with pytest.raises(ValueError, match="x0, y0, x1, y1"):
        D.bbox_crop_rect(37, 53, (0.2, 0.2, 0.8))
    with pytest.raises(ValueError, match="five"):
        D.bbox_crop_rect(37, 53, (0.2, 0.2, 0.8, 0.8), [1.0, .5])
    with pytest.raises(ValueError, match="not finite"):
        D.bbox_crop_rect(37, 53, (0.2, float("nan"), 0.8, 0.8))
    with pytest.raises(ValueError, match="not finite"):
        D.bbox_crop_rect(37, 53, (0.2, 0.2, float("inf"), 0.8))
    with pytest.raises(ValueError, match="one view per sample"):
        D.draw_train_params(2, cfg, bounding_box=(0.2, 0.2, 0.8, 0.8))
    p = D.val_params(1, cfg, n_channels=3)
    img = np.zeros((8, 9, 3), np.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        D.augment_images([img], None, [p], cfg, device="cpu")
    with pytest.raises(ValueError, match="one AugParams"):
        D.augment_images([img], None, [p, p], cfg)
    with pytest.raises(ValueError, match="one bounding box"):
        D.augment_images([img], [None, None], [p], cfg)
    with pytest.raises(ValueError, match="at most 2\\^24"):                         # would wrap round in the descriptor's int fields
        D.augment_images([img], [(0.0, 0.0, 1e12, 1.0)], [p], cfg)
    with pytest.raises(ValueError, match="no images"):
        D.augment_images([], None, [], cfg)


def _entry_args(desc, src_bytes=4096, I=1, C=3, out_h=8, out_w=8, null=()):
    """arguments of sv_augment_images with dummy, never dereferenced device addresses: a refused table returns before any GPU call"""
    a = dict(src=0x1000, src_bytes=src_bytes, I=I, C=C, images_host=ctypes.addressof(desc), images_dev_ws=0x2000, out_h=out_h, out_w=out_w,
             params_dev=0x3000, flip_dev=None, grey_sum_ws=0x4000, out=0x5000, stream=None)
    for k in null:
        a[k] = None
    return list(a.values())


def test_the_entry_refuses_a_malformed_descriptor_table_on_the_host():
    """Every refusal returns SV_ERR_INVALID with a message from the host-side checks; nothing is launched (no GPU is needed here)."""
    lib = hip.load()

    def desc(**kw):
        d = (hip.AugImage * 1)()
        base = dict(offset=0, Hs=10, Ws=12, x_left=2, x_right=7, y_top=1, y_bottom=8, pad_l=0, pad_r=3, pad_t=2, pad_b=0)
        base.update(kw)
        for k, v in base.items():
            setattr(d[0], k, v)
        return d

    def refused(d, match, **kw):
        rc = lib.sv_augment_images(*_entry_args(d, **kw))
        msg = lib.sv_last_error().decode()
        assert rc != 0 and match in msg, (rc, msg)

    assert ctypes.sizeof(hip.AugImage) == 48
    refused(desc(x_left=8), "empty or outside")                  # x_left > x_right
    refused(desc(y_top=9), "empty or outside")
    refused(desc(x_right=12), "empty or outside")                # one past the last column
    refused(desc(y_bottom=10), "empty or outside")
    refused(desc(x_left=-1), "empty or outside")
    refused(desc(pad_l=-1), "negative pad")
    refused(desc(pad_b=-2), "negative pad")
    refused(desc(pad_r=1 << 25), "padded crop")
    refused(desc(Hs=0), "has size")
    refused(desc(offset=-1), "does not lie inside")
    refused(desc(offset=4096 - 10 * 12 * 3 + 1), "does not lie inside")          # the last byte would be one past the buffer
    refused(desc(), "does not lie inside", src_bytes=10 * 12 * 3 - 1)
    refused(desc(), "channels", C=2)
    refused(desc(), "bad output size", out_h=0)
    refused(desc(), "bad output size", out_w=-4)
    refused(desc(), "images", I=0)
    refused(desc(), "images", I=70000)
    refused(desc(), "bad arguments", null=("images_dev_ws", ))
    refused(desc(), "bad arguments", null=("src", ))
