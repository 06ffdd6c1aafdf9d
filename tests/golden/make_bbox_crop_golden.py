#!/usr/bin/env python3
"""Golden vectors for the bounding-box branch of CenterCrop / RandomCrop (utils/data_transforms.py:93-136, :187-232), produced by
the REFERENCE's own utils/data_transforms.py.  That module imports cv2, which is not installed; it runs as written once a stand-in
`cv2` whose only member `resize` is oracle.data.resize_linear sits in sys.modules.  The stand-in also records what it is handed: the
cut and edge-padded crop.  So everything but the cv2.resize arithmetic - crop integers, np.pad, the order of the random draws,
background, jitter, noise, normalise, flip, permutation - is the reference's program text at work.

Per case the fixture holds the name of its uint8 image (the images are stored once), the box, the two seeds (np.random, random),
whether the list is the training one (RandomCrop ...) or the validation one (CenterCrop ...) of core/train.py:44-59, the padded
crop as uint8 (rint(x * 255) / 255 reproduces the float32 crop exactly; asserted) and the output of the whole Compose at 40 x 48.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bbox_crop_golden.py      (never runs on the GPU box)"""
import importlib.util
import io
import os
import random
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from oracle import data as OD  # noqa: E402
from swinvox_amd.config import default_cfg  # noqa: E402

handed = []                                                     # what the reference hands to cv2.resize


def _resize(img, dsize):
    handed.append(np.array(img, copy=True))
    return OD.resize_linear(img, dsize[1], dsize[0])            # cv2 takes (width, height)


cv2 = types.ModuleType("cv2")
cv2.resize = _resize
sys.modules["cv2"] = cv2
spec = importlib.util.spec_from_file_location("ref_data_transforms", os.path.join(os.environ.get("SWINVOX_REFERENCE", "/root/reference"),
                                                                                  "utils", "data_transforms.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

cfg = default_cfg()
OUT_HW, CROP_HW = (40, 48), (cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W)


def transforms(train):
    if train:                                                   # core/train.py:44-53
        return ref.Compose([ref.RandomCrop(OUT_HW, CROP_HW), ref.RandomBackground(cfg.TRAIN.RANDOM_BG_COLOR_RANGE),
                            ref.ColorJitter(cfg.TRAIN.BRIGHTNESS, cfg.TRAIN.CONTRAST, cfg.TRAIN.SATURATION),
                            ref.RandomNoise(cfg.TRAIN.NOISE_STD), ref.Normalize(mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD),
                            ref.RandomFlip(), ref.RandomPermuteRGB(), ref.ToTensor()])
    return ref.Compose([ref.CenterCrop(OUT_HW, CROP_HW), ref.RandomBackground(cfg.TEST.RANDOM_BG_COLOR_RANGE),     # :54-59
                        ref.Normalize(mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD), ref.ToTensor()])


def run(img_u8, box, train, seeds):
    """the reference's get_datum + transforms for one photograph (utils/data_loaders.py:176-203); also reports the flip and the
    channel permutation it drew, seen through wrappers round random.randint and np.random.permutation"""
    np.random.seed(seeds[0])
    random.seed(seeds[1])
    del handed[:]
    seen = {"randint": [], "perm": []}
    randint, permutation = random.randint, np.random.permutation
    random.randint = lambda a, b: seen["randint"].append(randint(a, b)) or seen["randint"][-1]
    np.random.permutation = lambda n: seen["perm"].append(permutation(n)) or seen["perm"][-1]
    try:
        img = img_u8.astype(np.float32) / 255.
        out = transforms(train)(np.asarray([img]), None if box is None else list(box))
    finally:
        random.randint, np.random.permutation = randint, permutation
    assert len(handed) == 1 and handed[0].dtype == np.float32
    crop_u8 = np.rint(handed[0] * 255).astype(np.uint8)
    assert np.array_equal(crop_u8.astype(np.float32) / 255., handed[0])
    out = out.numpy()
    assert out.shape == (1, 3) + OUT_HW and out.dtype == np.float32
    flip = bool(seen["randint"][-1]) if train else False        # RandomFlip's is the last random.randint of the list
    perm = [int(i) for i in seen["perm"][-1]] if train else [0, 1, 2]
    return crop_u8, out[0], flip, perm


rng = np.random.default_rng(20)
H, W = 37, 53
small3 = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
small4 = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
small4[..., 3] = np.where(rng.random((H, W)) < 0.2, 0, np.where(rng.random((H, W)) < 0.3, 120, 255))
small4[:3, :, 3] = 0                                            # transparent along the top and left borders: replicated into the padding
small4[:, :4, 3] = 0
yy, xx = np.mgrid[:150, :200]                                   # periodic, so it compresses, yet no two neighbours are equal
big3 = np.stack([(xx * 7 + yy * 13 + c * 50) % 256 for c in range(3)], -1).astype(np.uint8)
grey = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
low4 = rng.integers(0, 256, size=(22, 31, 4), dtype=np.uint8)     # a second size with alpha, so that a C = 4 batch is ragged too
low4[..., 3] = np.where(rng.random((22, 31)) < 0.3, 0, 255)
images = {"small3": small3, "small4": small4, "big3": big3, "grey": grey, "low4": low4}

# name: (image, box, training list?)
cases = {
    "inside": ("small3", (0.2, 0.3, 0.7, 0.8), False),                      # 27 x 28 after truncation: not square
    "two_sides": ("small3", (-0.1, 0.5, 0.4, 1.2), False),                  # hangs over the left and the bottom border
    "four_sides": ("small3", (-0.2, -0.3, 1.1, 1.25), False),               # larger than the image
    "right_edge": ("small3", (0.5, 0.4, 1.0, 0.6), False),                  # x_right == img_width exactly: pad_r = 1
    "trunc_left": ("small3", (-0.5 / W, 0.3, 0.6, 0.7), False),             # raw x_left = -0.5: int() gives 0, a floor would give -1
    "tiny": ("small3", (0.45, 0.45, 0.5, 0.5), False),                      # 3 x 4 crop, upsampled
    "zero_area": ("small3", (0.5, 0.5, 0.5, 0.5), False),                   # 1 x 1 crop: ssize = 1 in both directions
    "big_full": ("big3", (0.0, 0.0, 1.0, 1.0), False),                      # 201 x 201 -> 40 x 48: the taps skip source pixels
    "alpha_border": ("small4", (-0.1, -0.1, 0.8, 0.9), True),               # alpha 0 replicated into the padding, training list
    "alpha_inside": ("small4", (0.1, 0.2, 0.9, 0.7), False),
    "jitter_flip_perm": ("small3", (0.1, 0.2, 0.8, 0.9), True),             # seeds searched below: flip set, permutation not the identity
    "jitter_noflip": ("small3", (0.3, -0.2, 1.3, 0.6), True),
    "grey_box": ("grey", (0.25, 0.1, 0.75, 0.95), True),                    # stacked to three channels by the loader (:194-196)
    "nobox": ("small3", None, True),                                        # smaller than CROP_IMG: the whole image
    "nobox_alpha": ("small4", None, False),
    "low_alpha": ("low4", (0.3, -0.1, 1.05, 0.8), True),
    "nobox_large": ("big3", None, False),                                   # larger than CROP_IMG: its centre 128 x 128
}

out = {"names": np.array(list(cases)), "out_hw": np.array(OUT_HW)}
for key, im in images.items():
    out["img_" + key] = im
report = {}
for k, (name, (key, box, train)) in enumerate(cases.items()):
    img = images[key]
    if img.ndim == 2:
        img = np.stack((img, ) * 3, -1)                         # data_loaders.py:194-196
    seeds = [100 + k, 200 + k]
    crop, res, flip, perm = run(img, box, train, seeds)
    while name == "jitter_flip_perm" and not (flip and perm != [0, 1, 2]):
        seeds = [seeds[0] + 1000, seeds[1] + 1000]
        crop, res, flip, perm = run(img, box, train, seeds)
    while name == "jitter_noflip" and flip:
        seeds = [seeds[0] + 1000, seeds[1] + 1000]
        crop, res, flip, perm = run(img, box, train, seeds)
    out[name + "_image"] = np.array(key)
    out[name + "_box"] = np.zeros(0) if box is None else np.array(box, dtype=np.float64)
    out[name + "_seeds"] = np.array(seeds)
    out[name + "_train"] = np.array(train)
    out[name + "_crop"] = crop
    out[name + "_out"] = res
    report[name] = (crop.shape, flip, perm, seeds)

shape = {n: r[0][:2] for n, r in report.items()}
assert shape["inside"] == (27, 28) and shape["tiny"] == (3, 4) and shape["zero_area"] == (1, 1), shape
assert shape["big_full"] == (201, 201) and shape["nobox"] == (H, W) and shape["nobox_large"] == CROP_HW, shape
# right_edge: x_left = int(26.5), x_right = int(53.0) -> clamped to 52 with pad_r = 1: 52 - 26 + 1 + 1 columns
assert shape["right_edge"][1] == 28 and np.array_equal(out["right_edge_crop"][:, -1], out["right_edge_crop"][:, -2])
# trunc_left: raw x_left in (-1, 0) truncates to 0 (no pad): columns 0 .. int(31.8); a floor would have padded one more column
b = cases["trunc_left"][1]
raw_left = (b[2] * W + b[0] * W) * .5 - max(b[2] * W - b[0] * W, b[3] * H - b[1] * H) * .5
assert -1 < raw_left < 0 and int(raw_left) == 0 and shape["trunc_left"][1] == 32, (raw_left, shape["trunc_left"])
assert shape["four_sides"][0] > H and shape["four_sides"][1] > W
assert report["jitter_flip_perm"][1] and report["jitter_flip_perm"][2] != [0, 1, 2] and not report["jitter_noflip"][1]
assert (out["alpha_border_crop"][0, :, 3] == 0).all() and (out["alpha_border_crop"][:, 0, 3] == 0).all()

# np.savez stamps every member with the current time; fixed stamps make two runs write the same bytes
with zipfile.ZipFile(os.path.join(HERE, "bbox_crop_cases.npz"), "w") as zf:
    for key in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
        info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        zf.writestr(info, buf.getvalue())
for name, (shp, flip, perm, seeds) in report.items():
    print(f"{name:18s} crop {shp[0]:3d} x {shp[1]:3d} x {shp[2]}  flip {int(flip)}  perm {perm}  seeds {seeds}")
print("wrote", len(cases), "cases run through the reference's own transforms")
