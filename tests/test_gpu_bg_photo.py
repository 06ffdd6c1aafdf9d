"""Photograph backgrounds on the device (swinvox_amd/data.py: augment_views(..., backgrounds=...) -> sv_augment_views_bg) against
tests/golden/bg_photo_cases.npz - outputs of the reference's own training Compose with RandomBackground given a folder
(tests/golden/make_bg_photo_golden.py) - and, where no reference output is recorded, against the restatement tests/bg_photo_ref.py,
which tests/test_cpu_bg_photo.py pins to those outputs element for element.  The bound is the training-list bound of
tests/test_gpu_data.py, 5e-6: the reference computes in float64 after the float32 resize, the kernel in float32 throughout, and the
photograph only replaces the value that enters that arithmetic."""
import ctypes
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bg_photo_ref as R  # noqa: E402

import swinvox_amd as S  # noqa: E402
from oracle import data as OD  # noqa: E402
from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import hip  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "bg_photo_cases.npz"))
NAMES = [str(n) for n in G["names"]]
OUT_H, OUT_W = (int(v) for v in G["out_hw"])
BANK = G["bank"]
V = 3
BOUND = 5e-6


def cfg_at(h, w):
    cfg = S.default_cfg()
    cfg.CONST.IMG_H, cfg.CONST.IMG_W = h, w
    return cfg


def load_case(name, cfg):
    imgs = np.ascontiguousarray(G["img_" + str(G[name + "_image"])][..., :int(G[name + "_channels"])])
    np.random.seed(int(G[name + "_seeds"][0]))
    random.seed(int(G[name + "_seeds"][1]))
    return imgs, D.draw_train_params(V, cfg, n_channels=imgs.shape[-1], n_backgrounds=len(BANK))


@functools.lru_cache(maxsize=None)
def alpha_cases():
    """the four-channel cases of the fixture as one batch: (names, uint8 [B, V, 37, 53, 4], [AugParams])"""
    cfg = cfg_at(OUT_H, OUT_W)
    names = [n for n in NAMES if int(G[n + "_channels"]) == 4]
    imgs, params = zip(*(load_case(n, cfg) for n in names))
    return names, np.stack(imgs), list(params)


def restate(imgs, params, bank, cfg):
    return np.stack([R.sample_reference(im, p, bank, img_size=(cfg.CONST.IMG_H, cfg.CONST.IMG_W), crop_size=(cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W),
                                        mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD) for im, p in zip(imgs, params)])


def run(imgs, params, cfg, dev, bank=BANK):
    bank_dev = None if bank is None else D.background_bank(bank, cfg, device=dev)
    return D.augment_views(torch.from_numpy(imgs).to(dev), params, cfg, backgrounds=bank_dev).cpu().numpy()


def close(got, want, what):
    err = float(np.abs(got - want).max())
    print(f"{what}: max abs difference {err:.3e}")
    assert got.shape == want.shape and err < BOUND, (what, err)


def plain(V_, bg=(0.9, 0.95, 1.0), **kw):
    """identity jitter, zero noise, no flips, identity permutation"""
    p = D.AugParams(bg=list(bg), flips=[False] * V_)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_fixture_cases_match_the_reference_outputs(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    names, imgs, params = alpha_cases()
    assert len(names) == 3
    got = run(imgs, params, cfg, dev)
    assert got.dtype == np.float32 and got.shape == (len(names), V, 3, OUT_H, OUT_W)
    for i, n in enumerate(names):
        close(got[i], G[n + "_out"], n)
    # three channels with a bank: nothing is drawn and nothing is composited
    im3, p3 = load_case("rgb3", cfg)
    assert p3.bg_index is None and im3.shape[-1] == 3
    got3 = run(im3[None], [p3], cfg, dev)
    close(got3[0], G["rgb3_out"], "rgb3")
    assert np.array_equal(got3, run(im3[None], [p3], cfg, dev, bank=None))
    # a batched call gives every sample the bits of a call of its own
    for i in range(len(names)):
        assert np.array_equal(run(imgs[i:i + 1], params[i:i + 1], cfg, dev), got[i:i + 1]), names[i]


def test_transparent_pixels_are_the_photograph_bit_for_bit(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    cfg.DATASET.MEAN, cfg.DATASET.STD = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    imgs = G["img_edge4"][None]                                     # view 0 fully transparent, view 1 without a transparent pixel, view 2 mixed
    p = plain(V, bg_index=2, bg_photo=[True, True, True])
    got = run(imgs, [p], cfg, dev)[0]
    flat = run(imgs, [p], cfg, dev, bank=None)[0]
    photo = np.transpose(BANK[2].astype(np.float32) / np.float32(255.), (2, 0, 1))
    colour = np.asarray(p.bg, np.float32).reshape(3, 1, 1)
    for v in range(V):
        a = OD.resize_linear(imgs[0, v].astype(np.float32) / 255.0, OUT_H, OUT_W)[..., 3]
        clear = np.broadcast_to(a == 0, (3, OUT_H, OUT_W))
        assert np.array_equal(got[v][clear], photo[clear])          # (float)byte / 255.f, untouched by the identity jitter and normalise
        assert np.array_equal(flat[v][clear], np.broadcast_to(colour, clear.shape)[clear])
        assert np.array_equal(got[v][~clear], flat[v][~clear])      # everything else does not know about the bank
    assert np.array_equal(got[0], photo) and np.array_equal(got[1], flat[1])


def test_a_photograph_per_sample_and_a_sample_without_one(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    _, imgs, params = alpha_cases()
    imgs, params = imgs[:2], [D.AugParams(**vars(p)) for p in params[:2]]
    params[0].bg_index, params[0].bg_photo = 1, [True, False, True]
    params[1].bg_index, params[1].bg_photo = 2, [True, True, False]
    got = run(imgs, params, cfg, dev)
    close(got, restate(imgs, params, BANK, cfg), "a different photograph per sample")
    # one sample without a photograph in the same call: the flat colour throughout, whatever its coins say
    params[0].bg_index = None
    mixed = run(imgs, params, cfg, dev)
    close(mixed, restate(imgs, params, BANK, cfg), "one sample with bg_index None")
    assert np.array_equal(mixed[1], got[1])
    assert np.array_equal(mixed[0], run(imgs[:1], params[:1], cfg, dev, bank=None)[0])


def test_flip_and_coin_in_all_four_combinations(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    assert (BANK[1] != BANK[1][:, ::-1]).any(axis=2).all()          # not left-right symmetric, anywhere
    _, imgs, params = alpha_cases()
    four = np.stack([imgs[0, 0]] * 4)[None]                         # one rendering four times
    p = D.AugParams(**vars(params[0]))
    p.flips, p.bg_index, p.bg_photo = [False, True, False, True], 1, [False, False, True, True]
    got = run(four, [p], cfg, dev)
    close(got, restate(four, [p], BANK, cfg), "flip x coin")
    # the flip mirrors the finished image, photograph included; the grey mean does not depend on it
    assert np.array_equal(got[0, 1], got[0, 0][..., ::-1]) and np.array_equal(got[0, 3], got[0, 2][..., ::-1])
    assert not np.array_equal(got[0, 2], got[0, 0])


def test_contrast_first_blends_with_the_mean_of_the_composited_image(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    imgs = G["img_mix4"][None]
    p = plain(V, jitter_value=[1.2, 0.6, 0.8], jitter_order=[1, 0, 2], bg_index=0, bg_photo=[True, False, True], flips=[False, True, True],
              noise_alpha=[0.05, -0.02, 0.01], perm=[1, 2, 0])
    got = run(imgs, [p], cfg, dev)
    want = restate(imgs, [p], BANK, cfg)
    close(got, want, "contrast first")
    # the case can tell: an opaque pixel of view 0 knows about the photograph only through that mean, and in the restatement it moves by
    # over a hundred bounds when the mean is taken over the colour composite instead
    colour_only = restate(imgs, [plain(V, **{**vars(p), "bg_index": None})], BANK, cfg)
    solid = np.broadcast_to(OD.resize_linear(imgs[0, 0].astype(np.float32) / 255.0, OUT_H, OUT_W)[..., 3] != 0, (3, OUT_H, OUT_W))
    assert np.abs(colour_only[0, 0] - want[0, 0])[solid].min() > 100 * BOUND


def test_every_index_minus_one_equals_augment_views_bit_for_bit(dev):
    cfg = cfg_at(OUT_H, OUT_W)
    _, imgs, params = alpha_cases()
    params = [D.AugParams(**{**vars(p), "bg_photo": [False] * V}) for p in params]
    assert np.array_equal(run(imgs, params, cfg, dev), run(imgs, params, cfg, dev, bank=None))
    # at the full size, with the centre crop of the 137 x 137 renderings, and for three channels
    cfg = S.default_cfg()
    rng = np.random.default_rng(11)
    big = rng.integers(0, 256, size=(2, 2, 137, 137, 4), dtype=np.uint8)
    big[..., 3] = np.where(rng.random(big.shape[:-1]) < 0.4, 0, 255)
    np.random.seed(5)
    random.seed(6)
    prm = [D.draw_train_params(2, cfg) for _ in range(2)]
    bank = rng.integers(0, 256, size=(1, 224, 224, 3), dtype=np.uint8)
    assert np.array_equal(run(big, prm, cfg, dev, bank=bank), run(big, prm, cfg, dev, bank=None))
    prm3 = [D.draw_train_params(2, cfg, n_channels=3, n_backgrounds=1) for _ in range(2)]
    rgb = np.ascontiguousarray(big[..., :3])
    assert np.array_equal(run(rgb, prm3, cfg, dev, bank=bank), run(rgb, prm3, cfg, dev, bank=None))


def test_full_size_output_matches_the_restatement(dev):
    """224 x 224 from 137 x 137 sources (centre crop 128 x 128), where no reference output is recorded"""
    cfg = S.default_cfg()
    rng = np.random.default_rng(12)
    imgs = rng.integers(0, 256, size=(1, 2, 137, 137, 4), dtype=np.uint8)
    yy, xx = np.mgrid[:137, :137]
    for v in range(2):                                              # an opaque disc on a transparent ground, soft alpha at its rim
        d = np.sqrt((yy - 60 - 9 * v) ** 2 + (xx - 72) ** 2)
        imgs[0, v, :, :, 3] = np.where(d < 38, 255, np.where(d < 40, 120, 0))
    bank = rng.integers(0, 256, size=(2, 224, 224, 3), dtype=np.uint8)
    np.random.seed(13)
    random.seed(14)
    p = D.draw_train_params(2, cfg, n_backgrounds=2)
    p.bg_photo, p.flips = [True, True], [True, False]
    got = run(imgs, [p], cfg, dev, bank=bank)
    assert got.shape == (1, 2, 3, 224, 224)
    close(got, restate(imgs, [p], bank, cfg), "224 x 224")


@pytest.mark.parametrize("what,table,with_bank", [("index = n_bank", [0, 3, -1], True), ("index = -2", [-1, -2, 1], True),
                                                  ("NULL bank with an index >= 0", [-1, 0, -1], False)])
def test_the_entry_returns_an_error_code_and_leaves_the_output_untouched(dev, what, table, with_bank):
    cfg = cfg_at(OUT_H, OUT_W)
    lib = hip.load()
    imgs = torch.from_numpy(G["img_mix4"].copy()).to(dev)          # I = 3 images, V = 3
    arr, flips = D._pack_aug_samples([plain(V)], V, cfg, "test")
    prm = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    fl = torch.from_numpy(flips).to(dev)
    bank = torch.from_numpy(BANK.copy()).to(dev)
    ws = torch.zeros(V, dtype=torch.float64, device=dev)
    tab_dev = torch.full((V, ), 77, dtype=torch.int32, device=dev)
    out = torch.full((V, 3, OUT_H, OUT_W), -123.0, dtype=torch.float32, device=dev)
    tab = (ctypes.c_int * V)(*table)
    torch.cuda.synchronize()
    rc = lib.sv_augment_views_bg(imgs.data_ptr(), V, V, 37, 53, 4, cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W, OUT_H, OUT_W, prm.data_ptr(), fl.data_ptr(),
                                 bank.data_ptr() if with_bank else None, len(BANK), ctypes.addressof(tab), tab_dev.data_ptr(), ws.data_ptr(),
                                 out.data_ptr(), hip._stream())
    msg = lib.sv_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and "augment_views_bg" in msg, (what, rc, msg)
    assert bool((out == -123.0).all()) and bool((tab_dev == 77).all())
