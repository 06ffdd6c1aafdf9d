"""Host side of photograph backgrounds (swinvox_amd/data.py: draw_train_params(n_backgrounds=...), background_bank, augment_views(...,
backgrounds=...), the table checks of sv_augment_views_bg) against tests/golden/bg_photo_cases.npz, which the reference's own
utils/data_transforms.py produced with RandomBackground given a folder (tests/golden/make_bg_photo_golden.py).  The same fixture pins
the restatement tests/bg_photo_ref.py - the expected value of tests/test_gpu_bg_photo.py: it must reproduce the reference's outputs
element for element."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bg_photo_ref as R  # noqa: E402

import swinvox_amd as S  # noqa: E402
from oracle import data as OD  # noqa: E402
from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "bg_photo_cases.npz"))
NAMES = [str(n) for n in G["names"]]
OUT_H, OUT_W = (int(v) for v in G["out_hw"])
BANK = G["bank"]
V = 3
ENTRY = "sv_augment_views_bg"


def cfg_small():
    cfg = S.default_cfg()
    cfg.CONST.IMG_H, cfg.CONST.IMG_W = OUT_H, OUT_W
    return cfg


def load_case(name, cfg):
    """(uint8 renderings [V, 37, 53, C], AugParams drawn as the loader would draw them after re-seeding)"""
    imgs = np.ascontiguousarray(G["img_" + str(G[name + "_image"])][..., :int(G[name + "_channels"])])
    np.random.seed(int(G[name + "_seeds"][0]))
    random.seed(int(G[name + "_seeds"][1]))
    return imgs, D.draw_train_params(V, cfg, n_channels=imgs.shape[-1], n_backgrounds=len(BANK))


def test_the_fixture_holds_the_cases_that_matter():
    assert BANK.shape == (3, OUT_H, OUT_W, 3) and BANK.dtype == np.uint8
    assert all((p != p[:, ::-1]).any() for p in BANK)                                   # no photograph is left-right symmetric
    coins = {n: [bool(c) for c in G[n + "_coins"]] for n in NAMES}
    flips = {n: [bool(c) for c in G[n + "_flips"]] for n in NAMES}
    assert any(0 < sum(c) < V for c in coins.values())                                  # mixed coins within a sample
    assert any(len(c) == V and all(c) for c in coins.values()) and any(len(c) == V and not any(c) for c in coins.values())
    assert any(a and b for n in NAMES for a, b in zip(coins[n], flips[n]))              # a flipped view that takes the photograph
    assert any(list(G[n + "_perm"]) != [0, 1, 2] for n in NAMES)
    assert any(int(G[n + "_order"][0]) == 1 and any(coins[n]) for n in NAMES)           # contrast first, over a composited photograph
    edge = G["img_edge4"]
    assert (edge[0, ..., 3] == 0).all() and (edge[1, ..., 3] != 0).all()                # a fully transparent view, one without a transparent pixel
    assert set(np.unique(G["img_mix4"][..., 3])) == {0, 120, 255}
    for v in range(V):                                                                  # resized pixels that take the background are common
        clear = OD.resize_linear(G["img_mix4"][v].astype(np.float32) / 255.0, OUT_H, OUT_W)[..., 3] == 0
        assert 0.1 < clear.mean() < 0.6, (v, clear.mean())
    assert any(int(G[n + "_channels"]) == 3 and int(G[n + "_index"]) == -1 and G[n + "_coins"].size == 0 for n in NAMES)
    assert all(G[n + "_out"].shape == (V, 3, OUT_H, OUT_W) for n in NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_draws_with_a_folder_are_the_references(name):
    _, p = load_case(name, cfg_small())
    index = int(G[name + "_index"])
    assert p.bg_index == (None if index < 0 else index)
    assert [bool(c) for c in p.bg_photo] == [bool(c) for c in G[name + "_coins"]]
    assert [bool(f) for f in p.flips] == [bool(f) for f in G[name + "_flips"]]
    assert list(p.jitter_order) == [int(i) for i in G[name + "_order"]] and list(p.perm) == [int(i) for i in G[name + "_perm"]]


def test_draws_without_a_folder_are_the_draws_of_today():
    cfg = S.default_cfg()
    for n_channels in (3, 4):
        for n_views in (1, 3):
            np.random.seed(7)
            random.seed(8)
            p = D.draw_train_params(n_views, cfg, n_channels=n_channels, n_backgrounds=0)
            state_np, state_py = np.random.get_state(), random.getstate()
            assert p.bg_index is None and tuple(p.bg_photo) == () and p.crop_draws is None
            np.random.seed(7)
            random.seed(8)
            o = OD.draw_train_params(n_views, dict(RANDOM_BG_COLOR_RANGE=cfg.TRAIN.RANDOM_BG_COLOR_RANGE, BRIGHTNESS=cfg.TRAIN.BRIGHTNESS,
                                                   CONTRAST=cfg.TRAIN.CONTRAST, SATURATION=cfg.TRAIN.SATURATION, NOISE_STD=cfg.TRAIN.NOISE_STD),
                                     n_channels=n_channels)
            assert np.array_equal(np.random.get_state()[1], state_np[1]) and np.random.get_state()[2:] == state_np[2:]
            assert random.getstate() == state_py
            assert list(p.bg) == list(o["bg"]) and list(p.jitter_value) == list(o["jitter_value"]) and list(p.jitter_order) == o["jitter_order"]
            assert list(p.noise_alpha) == list(o["noise_alpha"]) and list(p.flips) == o["flips"] and list(p.perm) == o["perm"]
    # a folder and three channels: RandomBackground returns before it draws, so nothing moves either
    np.random.seed(7)
    random.seed(8)
    q = D.draw_train_params(3, cfg, n_channels=3, n_backgrounds=5)
    state_np, state_py = np.random.get_state(), random.getstate()
    np.random.seed(7)
    random.seed(8)
    p = D.draw_train_params(3, cfg, n_channels=3)
    assert q == p and q.bg_index is None and tuple(q.bg_photo) == ()
    assert np.array_equal(np.random.get_state()[1], state_np[1]) and random.getstate() == state_py
    # a folder and four channels: exactly one more draw from `random`, the choice, between the colour and the coins
    np.random.seed(7)
    random.seed(8)
    q = D.draw_train_params(3, cfg, n_backgrounds=5)
    random.seed(8)
    want_index = random.choice(range(5))
    want_coins = [bool(random.randint(0, 1)) for _ in range(3)]
    want_flips = [bool(random.randint(0, 1)) for _ in range(3)]
    assert (q.bg_index, list(q.bg_photo), list(q.flips)) == (want_index, want_coins, want_flips)
    np.random.seed(7)
    p = D.draw_train_params(3, cfg)
    assert list(q.bg) == list(p.bg) and list(q.jitter_value) == list(p.jitter_value) and list(q.perm) == list(p.perm)
    with pytest.raises(ValueError, match="n_backgrounds"):
        D.draw_train_params(3, cfg, n_backgrounds=-1)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference_outputs(name):
    cfg = cfg_small()
    imgs, p = load_case(name, cfg)
    got = R.sample_reference(imgs, p, BANK, img_size=(OUT_H, OUT_W), crop_size=(cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W),
                             mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD)
    want = G[name + "_out"]
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), float(np.abs(got - want).max())


@pytest.mark.parametrize("name", NAMES)
def test_restatement_without_a_photograph_is_the_oracle(name):
    cfg = cfg_small()
    imgs, p = load_case(name, cfg)
    kw = dict(img_size=(OUT_H, OUT_W), crop_size=(cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W), mean=cfg.DATASET.MEAN, std=cfg.DATASET.STD)
    want = OD.transform_views(imgs, R.oracle_prm(p), **kw)
    assert np.array_equal(R.sample_reference(imgs, p, None, **kw), want)                       # no bank
    assert np.array_equal(R.transform_views_bg(imgs, R.oracle_prm(p), BANK[0], [False] * V, **kw), want)    # a photograph no view takes


def test_background_bank_refuses_what_the_reference_fails_on():
    cfg = cfg_small()
    ok = np.zeros((OUT_H, OUT_W, 3), np.uint8)
    for bad in ([np.zeros((OUT_H, OUT_W + 1, 3), np.uint8)],                                  # another size
                [ok, np.zeros((OUT_H - 1, OUT_W, 3), np.uint8)],
                [np.zeros((OUT_W, OUT_H, 3), np.uint8)],                                      # transposed
                [np.zeros((OUT_H, OUT_W, 4), np.uint8)],                                      # four channels
                [np.zeros((OUT_H, OUT_W), np.uint8)],                                         # greyscale: another rank
                [ok.astype(np.float32)],                                                      # another dtype
                [torch.zeros(OUT_H, OUT_W, 3)],
                np.zeros((2, OUT_H, OUT_W + 1, 3), np.uint8),                                 # stacked, another size
                np.zeros((OUT_H, OUT_W, 3), np.uint8),                                        # a single photograph is not a stack
                np.zeros((0, OUT_H, OUT_W, 3), np.uint8),
                torch.zeros(2, OUT_H, OUT_W, 3, dtype=torch.int16)):
        with pytest.raises(ValueError, match="the reference fails on it too"):
            D.background_bank(bad, cfg)
    with pytest.raises(ValueError, match="no photographs"):
        D.background_bank([], cfg)
    for good in ([ok, ok], np.stack([ok, ok]), torch.from_numpy(np.stack([ok]))):             # well-formed: only the GPU is missing
        with pytest.raises(RuntimeError, match="GPU"):
            D.background_bank(good, cfg, device="cpu")


def test_augment_views_refuses_a_malformed_bank_or_table_before_it_looks_for_a_gpu():
    cfg = cfg_small()
    x = torch.zeros(2, V, 37, 53, 4, dtype=torch.uint8)                                        # CPU tensors throughout
    bank = torch.from_numpy(BANK.copy())

    def prm(**kw):
        p = D.val_params(V, cfg)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    with pytest.raises(ValueError, match="bg_photo flags"):
        D.augment_views(x, [prm(), prm(bg_index=0, bg_photo=[True, False])], cfg, backgrounds=bank)
    with pytest.raises(ValueError, match="bg_photo flags"):
        D.augment_views(x, [prm(bg_photo=[True] * (V + 1)), prm()], cfg, backgrounds=bank)
    with pytest.raises(ValueError, match="photograph 3 of a bank of 3"):
        D.augment_views(x, [prm(bg_index=3, bg_photo=[True] * V), prm()], cfg, backgrounds=bank)
    with pytest.raises(ValueError, match="photograph -1 of a bank of 3"):
        D.augment_views(x, [prm(), prm(bg_index=-1, bg_photo=[False] * V)], cfg, backgrounds=bank)
    with pytest.raises(ValueError, match="IMG_H x IMG_W"):
        D.augment_views(x, [prm(), prm()], cfg, backgrounds=torch.zeros(3, OUT_H, OUT_W + 1, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="IMG_H x IMG_W"):
        D.augment_views(x, [prm(), prm()], S.default_cfg(), backgrounds=bank)                  # a 40 x 48 bank for 224 x 224 outputs
    with pytest.raises(ValueError, match="IMG_H x IMG_W"):
        D.augment_views(x, [prm(), prm()], cfg, backgrounds=bank.float())
    with pytest.raises(ValueError, match="IMG_H x IMG_W"):
        D.augment_views(x, [prm(), prm()], cfg, backgrounds=BANK)                              # an array: the bank is a tensor on the GPU
    with pytest.raises(RuntimeError, match="GPU"):                                             # well-formed: only the GPU is missing
        D.augment_views(x, [prm(bg_index=2, bg_photo=[True, False, True]), prm()], cfg, backgrounds=bank)
    table = D._bg_index_table([prm(bg_index=2, bg_photo=[True, False, True]), prm(), prm(bg_index=1), prm(bg_photo=[True] * V)], V, cfg, bank)
    assert table.dtype == np.int32 and table.tolist() == [2, -1, 2] + [-1] * 9               # no index, or no flags: the flat colour


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\bint\s+" + ENTRY + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
    assert m, f"{ENTRY} is not declared"
    comment = (m.group(1) or "") + (m.group(2) or "")
    assert "utils/data_transforms.py:415-452" in comment and "RandomBackground" in comment
    assert "bank[idx][oy][sx][c] / 255.f" in comment and "-1 <= idx < n_bank" in comment and "BEFORE anything is launched" in comment
    for arg in ("const unsigned char* bank", "int n_bank", "const int* bg_index_host", "int* bg_index_dev_ws"):
        assert arg in m.group(0), arg


def test_exported_and_bound():
    assert ENTRY in hip.EXPORTED_SYMBOLS
    lib = hip.load()                          # dlopen only: no GPU call is made
    at = lib.sv_augment_views_bg.argtypes
    assert len(hip._argtypes(ENTRY)) == 19 and len(at) == 19
    assert all(at[i] is ctypes.c_int for i in (1, 2, 3, 4, 5, 6, 7, 8, 9, 13)) and all(at[i] is ctypes.c_void_p for i in (0, 10, 11, 12, 14, 15, 16, 17, 18))
    # the new entry takes the arguments of sv_augment_views and four more
    assert len(lib.sv_augment_views.argtypes) == 15


# fake device addresses: every call below is refused before anything could read them
def _entry_args(table, n_bank=3, bank=0x6000, I=None, **over):
    tab = (ctypes.c_int * len(table))(*table)
    a = dict(src=0x1000, I=len(table) if I is None else I, V=1, Hs=37, Ws=53, C=4, crop_h=128, crop_w=128, out_h=OUT_H, out_w=OUT_W, params_dev=0x3000,
             flip_dev=None, bank=bank, n_bank=n_bank, bg_index_host=ctypes.addressof(tab), bg_index_dev_ws=0x7000, grey_sum_ws=0x4000, out=0x5000,
             stream=None)
    a.update(over)
    return tab, list(a.values())


@pytest.mark.parametrize("what,match,table,kw", [
    ("index = n_bank", "photograph 3 of a bank of 3", [0, 3, -1], {}),
    ("index = -2", "photograph -2 of a bank of 3", [-1, -1, -2], {}),
    ("large index", "photograph 2147483647", [2147483647], {}),
    ("NULL bank with an index >= 0", "the bank is NULL", [-1, 1], dict(bank=None)),
    ("empty bank", "photograph 0 of a bank of 0", [0], dict(n_bank=0)),
    ("negative bank size", "bank of -1", [-1], dict(n_bank=-1)),
    ("no host table", "bad arguments", [-1], dict(bg_index_host=None)),
    ("no table workspace", "bad arguments", [-1], dict(bg_index_dev_ws=None)),
    ("no source", "bad arguments", [-1], dict(src=None)),
    ("I not a multiple of V", "bad shapes", [-1, -1, -1], dict(V=2)),
    ("two channels", "bad shapes", [-1], dict(C=2)),
    ("too many images", "65535", [-1], dict(I=70000)),
    ("output too large", "bad output size", [-1], dict(out_h=1 << 15, out_w=1 << 15)),
])
def test_the_entry_refuses_a_malformed_table_on_the_host(what, match, table, kw):
    """Every refusal returns an error code with a message from the host-side checks; nothing is launched (no GPU is needed here)."""
    lib = hip.load()
    tab, args = _entry_args(table, **kw)
    rc = lib.sv_augment_views_bg(*args)
    msg = lib.sv_last_error().decode()
    assert rc != 0 and match in msg and "augment_views_bg" in msg, (what, rc, msg)
