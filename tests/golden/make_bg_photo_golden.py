#!/usr/bin/env python3
"""Golden vectors for RandomBackground with a folder of photographs (utils/data_transforms.py:415-452), produced by the REFERENCE's own
utils/data_transforms.py, run as tests/golden/make_bbox_crop_golden.py runs it: that module imports cv2, which is not installed, so a
stand-in `cv2` sits in sys.modules whose `resize` is oracle.data.resize_linear and whose `imread` hands out arrays from a dict, and
os.listdir is patched while RandomBackground lists its folder.  Everything but the cv2.resize arithmetic - which photograph, which view
takes it, the blend, the order of the random draws, jitter, noise, normalise, flip, permutation - is the reference's program text at work.

Per case the fixture holds the name of its uint8 renderings (V = 3 views of 37 x 53, stored once), the two seeds (np.random, random),
what the reference drew - photograph index, the per-view coins, flips, jitter order, channel permutation - as seen through wrappers round
random.choice, random.randint, np.random.shuffle and np.random.permutation, and the output of the whole training Compose at 40 x 48.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_bg_photo_golden.py      (never runs on the GPU box)"""
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

FOLDER, FILES = "backgrounds", ["p0.jpg", "p1.jpg", "p2.jpg"]
on_disk = {}                                                    # path -> uint8 [40, 48, 3]: what the stand-in imread returns

cv2 = types.ModuleType("cv2")
cv2.resize = lambda img, dsize: OD.resize_linear(img, dsize[1], dsize[0])       # cv2 takes (width, height)
cv2.imread = lambda path: np.array(on_disk[path], copy=True)
sys.modules["cv2"] = cv2
spec = importlib.util.spec_from_file_location("ref_data_transforms", os.path.join(os.environ.get("SWINVOX_REFERENCE", "/root/reference"),
                                                                                  "utils", "data_transforms.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

cfg = default_cfg()
V, OUT_HW, CROP_HW = 3, (40, 48), (cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W)


def transforms():
    """core/train.py:44-53 with the folder argument of RandomBackground filled in"""
    listdir = os.listdir
    os.listdir = lambda path: list(FILES) if path == FOLDER else listdir(path)
    try:
        background = ref.RandomBackground(cfg.TRAIN.RANDOM_BG_COLOR_RANGE, FOLDER)
    finally:
        os.listdir = listdir
    assert background.random_bg_files == [os.path.join(FOLDER, f) for f in FILES]
    return ref.Compose([ref.RandomCrop(OUT_HW, CROP_HW), background,
                        ref.ColorJitter(cfg.TRAIN.BRIGHTNESS, cfg.TRAIN.CONTRAST, cfg.TRAIN.SATURATION),
                        ref.RandomNoise(cfg.TRAIN.NOISE_STD), ref.Normalize(mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD),
                        ref.RandomFlip(), ref.RandomPermuteRGB(), ref.ToTensor()])


def run(imgs_u8, seeds):
    """the reference's get_datum + training transforms for one sample (utils/data_loaders.py:52-88) and what it drew on the way"""
    np.random.seed(seeds[0])
    random.seed(seeds[1])
    seen = {"choice": [], "randint": [], "shuffle": [], "perm": []}
    choice, randint, shuffle, permutation = random.choice, random.randint, np.random.shuffle, np.random.permutation

    def shuffle_seen(x):
        shuffle(x)
        seen["shuffle"].append([int(i) for i in x])

    random.choice = lambda seq: seen["choice"].append(choice(seq)) or seen["choice"][-1]
    random.randint = lambda a, b: seen["randint"].append(randint(a, b)) or seen["randint"][-1]
    np.random.shuffle = shuffle_seen
    np.random.permutation = lambda n: seen["perm"].append(permutation(n)) or seen["perm"][-1]
    try:
        out = transforms()(np.asarray([im.astype(np.float32) / 255. for im in imgs_u8]), None)
    finally:
        random.choice, random.randint, np.random.shuffle, np.random.permutation = choice, randint, shuffle, permutation
    out = out.numpy()
    assert out.shape == (V, 3) + OUT_HW and out.dtype == np.float32
    alpha = imgs_u8.shape[-1] == 4
    assert len(seen["choice"]) == (1 if alpha else 0) and len(seen["randint"]) == (2 * V if alpha else V)
    assert len(seen["shuffle"]) == 1 and len(seen["perm"]) == 1
    index = [os.path.join(FOLDER, f) for f in FILES].index(seen["choice"][0]) if alpha else -1
    coins = [bool(c) for c in seen["randint"][:V]] if alpha else []
    flips = [bool(c) for c in seen["randint"][-V:]]             # RandomFlip's are the last V random.randint of the list
    return out, index, coins, flips, seen["shuffle"][0], [int(i) for i in seen["perm"][0]]


rng = np.random.default_rng(31)
H, W = 37, 53
yy, xx = np.mgrid[:OUT_HW[0], :OUT_HW[1]]                       # photographs: periodic, so they compress; no row is left-right symmetric
for k, f in enumerate(FILES):
    on_disk[os.path.join(FOLDER, f)] = np.stack([(xx * (5 + 2 * k) + yy * (11 + 4 * k) + c * 70 + 30 * k) % 256 for c in range(3)], -1).astype(np.uint8)
bank = np.stack([on_disk[os.path.join(FOLDER, f)] for f in FILES])
assert all((p != p[:, ::-1]).any(axis=(1, 2)).all() for p in bank)


def rendering(transparent, soft):
    im = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    # alpha in 4 x 4 patches, so that resized pixels whose taps are all transparent are common
    u = np.repeat(np.repeat(rng.random((H // 4 + 1, W // 4 + 1)), 4, axis=0), 4, axis=1)[:H, :W]
    im[..., 3] = np.where(u < transparent, 0, np.where(u < transparent + soft, 120, 255))
    return im


mix4 = np.stack([rendering(0.3, 0.25) for _ in range(V)])        # alpha in {0, 120, 255} in every view
edge4 = np.stack([rendering(1.0, 0.0), rendering(0.0, 0.4), rendering(0.3, 0.25)])
edge4[0, ..., :3] = 77                                          # view 0 fully transparent (its colours never show), view 1 without a transparent pixel
assert (edge4[0, ..., 3] == 0).all() and (edge4[1, ..., 3] != 0).all() and set(np.unique(mix4[..., 3])) == {0, 120, 255}
images = {"mix4": mix4, "edge4": edge4}

# name: (renderings, channels kept, what the seeds are searched for)
cases = {
    # mixed coins, a flipped view that takes the photograph, a permutation that is not the identity
    "mixed": ("mix4", 4, lambda i, c, f, o, p: 0 < sum(c) < V and any(a and b for a, b in zip(c, f)) and not all(f) and p != [0, 1, 2]),
    # every view takes the photograph - the fully transparent one is the photograph - and contrast comes first in the jitter order
    "all_photo": ("edge4", 4, lambda i, c, f, o, p: all(c) and o[0] == 1 and i != 0),
    "all_colour": ("edge4", 4, lambda i, c, f, o, p: not any(c) and any(f)),
    # three channels with a folder set: RandomBackground returns before it draws anything (:428-430)
    "rgb3": ("mix4", 3, lambda i, c, f, o, p: i == -1 and c == []),
}

out = {"names": np.array(list(cases)), "out_hw": np.array(OUT_HW), "bank": bank}
for key, im in images.items():
    out["img_" + key] = im
report = {}
for k, (name, (key, channels, wanted)) in enumerate(cases.items()):
    imgs = np.ascontiguousarray(images[key][..., :channels])
    seeds = [300 + k, 400 + k]
    res, index, coins, flips, order, perm = run(imgs, seeds)
    while not wanted(index, coins, flips, order, perm):
        seeds = [seeds[0] + 1000, seeds[1] + 1000]
        res, index, coins, flips, order, perm = run(imgs, seeds)
    out[name + "_image"] = np.array(key)
    out[name + "_channels"] = np.array(channels)
    out[name + "_seeds"] = np.array(seeds)
    out[name + "_index"] = np.array(index)
    out[name + "_coins"] = np.array(coins, dtype=bool)
    out[name + "_flips"] = np.array(flips, dtype=bool)
    out[name + "_order"] = np.array(order)
    out[name + "_perm"] = np.array(perm)
    out[name + "_out"] = res
    report[name] = (index, coins, flips, order, perm, seeds)

# np.savez stamps every member with the current time; fixed stamps make two runs write the same bytes
path = os.path.join(HERE, "bg_photo_cases.npz")
with zipfile.ZipFile(path, "w") as zf:
    for key in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[key]), allow_pickle=False)
        info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        zf.writestr(info, buf.getvalue())
for name, (index, coins, flips, order, perm, seeds) in report.items():
    print(f"{name:10s} photograph {index:2d}  coins {[int(c) for c in coins]}  flips {[int(c) for c in flips]}  order {order}  perm {perm}  seeds {seeds}")
print("wrote", len(cases), "cases run through the reference's own transforms:", os.path.getsize(path), "bytes")
