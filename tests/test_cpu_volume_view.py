"""Volume views (csrc/render.hip sv_render_volumes, data.view_camera / render_views_batch / image_file) without a GPU: the header
declares the entry with its rule and cites what the reference draws, the ctypes table binds it, the argument refusals - host-side checks
that run before any GPU call - answer SV_ERR_INVALID with the entry's name; the numpy restatement (tests/volume_view_ref.py, the expected
value of test_gpu_volume_view.py) has the camera matplotlib recorded and draws the silhouettes and face colours of the reference's own
pictures (tests/golden/volume_view_cases.npz, written by utils/helpers.py:50-88 itself); its float32 and float64 variants agree within
the cap the GPU comparison uses; data.image_file writes PNG and PPM.

The 32^3 checkerboard is not in the fixture (its picture would put the file above the largest fixture committed before it).  Checked once
when the fixture was written, against the reference's picture of it: both silhouette exception sets empty, float32 and float64 ids
equal, all 12 976 face-interior pixels within 2 levels of the table."""
import ctypes
import functools
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import volume_view_ref as R  # noqa: E402

import swinvox_amd as S  # noqa: E402
from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import harness  # noqa: E402
from swinvox_amd import hip  # noqa: E402
from swinvox_amd.models import Decoder, Encoder, Merger, Refiner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "volume_view_cases.npz"))
CASES = ("boxes", "sphere", "rand31x33x32")
ENTRY = "sv_render_volumes"
SV_ERR_INVALID = -1
SIZE = (480, 640)
# share of the 3x3-uniform pixels of a visible face within 2 levels of the recorded colour of its normal, as measured on the fixture when
# this test was written (the rest: matplotlib's painter's-sort artefacts on coplanar regions and anti-aliased edge lines); the floors
# asserted are these minus 0.03
MEASURED_SHARE = {"boxes": {"+x": 0.9687, "+y": 0.9322, "+z": 0.9708}, "sphere": {"+x": 0.9715, "+y": 0.9283, "+z": 0.9642},
                  "rand31x33x32": {"+x": 1.0, "+y": 1.0, "+z": 1.0}}


def cap(size):
    """pixels of one image that may differ between two evaluations of the rule in different arithmetic"""
    return max(2, int(1e-4 * size[0] * size[1]))


def golden(name):
    """(bool volume, picture uint8 [3, 480, 640], plate, proj [4, 4], trans [3, 3]) of a fixture case"""
    dims = [int(d) for d in G[name + "_dims"]]
    vol = np.unpackbits(G[name + "_occ"])[:int(np.prod(dims))].astype(bool).reshape(dims)
    plate = G["plate_%dx%dx%d" % tuple(dims)].transpose(2, 0, 1)
    img = plate.copy()
    crop, (r0, c0) = G[name + "_image"].transpose(2, 0, 1), G[name + "_offset"]
    img[:, r0:r0 + crop.shape[1], c0:c0 + crop.shape[2]] = crop
    return vol, img, plate, G[name + "_proj"], G[name + "_trans"]


@functools.lru_cache(maxsize=None)
def golden_ids(name, dtype=np.float32):
    vol = golden(name)[0]
    ids = R.render_ids(vol, R.view_camera(vol.shape), SIZE, dtype)
    ids.setflags(write=False)
    return ids


def silhouette_exceptions(img, plate, hit):
    """(drawn pixels outside the hit mask dilated by 2, pixels of the hit mask eroded by 1 that are not drawn)"""
    drawn = (img != plate).any(axis=0)
    return int((drawn & ~R.dilate(hit, 2)).sum()), int((R.erode(hit, 1) & ~drawn).sum())


# ---- small cases, shared with the GPU test ------------------------------------------------------------------------------------------------
def _cams_for(dims, size):
    return {"ref": R.view_camera(dims, size=size), "ortho": R.view_camera(dims, size=size, proj_type="ortho"),
            "level": R.view_camera(dims, 0, 0, size=size), "level_ortho": R.view_camera(dims, 0, 0, size=size, proj_type="ortho")}


@functools.lru_cache(maxsize=None)
def small_cases():
    """name -> (bool [B, a, b, c], [cameras], (H, W)).  Sizes where neither side is a multiple of the 16-pixel tile, one- and two-word
    rows, both LDS sizes of the kernel, direction components that are exactly 0 (elev 0 / azim 0: the orthographic rays run along -x)."""
    rng = np.random.default_rng(20261021)
    out = {}
    c8 = _cams_for((8, 8, 8), (45, 70))
    rand8 = rng.random((3, 8, 8, 8)) < 0.3
    out["rand8"] = (rand8, [c8["ref"]], (45, 70))
    out["rand8_ortho"] = (rand8, [c8["ortho"]], (45, 70))
    out["rand8_level"] = (rand8, [c8["level"], c8["level_ortho"]], (45, 70))
    out["rand8_three_cameras"] = (rand8, [R.view_camera((8, 8, 8), 30, 45, (45, 70)), R.view_camera((8, 8, 8), -20, 160, (45, 70)),
                                          R.view_camera((8, 8, 8), 75, 250, (45, 70), "ortho")], (45, 70))
    away = np.array(c8["ref"])
    away[3:] = -away[3:]                                                       # looks the other way: tin < 0 everywhere
    aside = np.array(c8["ortho"])
    aside[0] += 100.0 * aside[1]                                               # 100 columns to the right of a 70-column image
    out["rand8_not_reached"] = (rand8, [away, aside], (45, 70))
    out["empty_full8"] = (np.stack([np.zeros((8, 8, 8), bool), np.ones((8, 8, 8), bool)]), [c8["ref"], c8["ortho"]], (45, 70))
    out["one"] = (np.ones((1, 1, 1, 1), bool), list(_cams_for((1, 1, 1), (40, 56)).values()), (40, 56))
    for dims in ((5, 7, 3), (3, 4, 40), (2, 2, 64)):
        cams = _cams_for(dims, (50, 66))
        out["rand%dx%dx%d" % dims] = (np.stack([rng.random(dims) < 0.5, np.ones(dims, bool)]), [cams["ref"], cams["ortho"], cams["level"]], (50, 66))
    out["rand64"] = ((rng.random((1, 64, 64, 64)) < 0.02), [R.view_camera((64, 64, 64), size=(96, 96))], (96, 96))
    out["sweep8"] = (np.eye(512, dtype=bool).reshape(512, 8, 8, 8), [R.view_camera((8, 8, 8), size=(48, 48))], (48, 48))
    return out


@functools.lru_cache(maxsize=None)
def small_ids(name, dtype=np.float32):
    """int32 [B, n_cams, H, W] of a small case by the restatement; computed once, read-only"""
    vols, cams, size = small_cases()[name]
    ids = np.stack([np.stack([R.render_ids(v, c, size, dtype) for c in cams]) for v in vols])
    ids.setflags(write=False)
    return ids


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)typedef struct sv_view_camera \{ float o0\[3\], ox\[3\], oy\[3\], d0\[3\], dx\[3\], dy\[3\]; \} sv_view_camera;\s*"
                  r"int\s+" + ENTRY + r"\s*\(([^;]*)\)\s*;", hdr, flags=re.S)
    assert m, f"{ENTRY} is not declared"
    comment, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    for cite in ("utils/helpers.py:50-88", "core/test.py:178-187", "utils/binvox_rw.py:306-343"):
        assert cite in comment, cite
    for rule in ("-x, +x, -y, +y, -z, +z", "((i*d1 + j)*d2 + k)*6 + face", "first arg-max", "first arg-min", "tin < tout and tin > 0",
                 "(col+0.5)", "right or of its lower neighbour", "no fma contraction"):
        assert rule in comment, rule
    # the argument list, type for type, against the ctypes table
    kinds = []
    for a in args:
        kinds.append(ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_int)
    assert kinds == hip._argtypes(ENTRY) and len(kinds) == 20
    assert args[0].startswith("const void* vol") and args[7].startswith("const sv_view_camera* cams_host") and args[-1] == "void* stream"


def test_exported_and_bound():
    assert ENTRY in hip.EXPORTED_SYMBOLS
    lib = hip.load()                          # dlopen only: no GPU call is made
    at = lib.sv_render_volumes.argtypes
    assert len(at) == 20 and at[6] is ctypes.c_float
    assert all(at[i] is ctypes.c_int for i in (1, 2, 3, 4, 5, 8, 10, 11)) and all(at[i] is ctypes.c_void_p for i in (0, 7, 9, 12, 13, 14, 15, 16, 17, 18, 19))
    assert ctypes.sizeof(hip.ViewCamera) == 72
    src = open(os.path.join(ROOT, "swinvox_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\brender\.hip\b", src, flags=re.M)


# fake device addresses: every call below is refused before anything could read them; the host arrays are real
VOL, CAMS_WS, MASK, IDS, RGB, PLATE = (0x10000 * (i + 1) for i in range(6))
FACE = (ctypes.c_ubyte * 18)(*range(18))
EDGE = (ctypes.c_ubyte * 3)(0, 0, 0)
BG = (ctypes.c_ubyte * 3)(255, 255, 255)


def _cam_array(cams):
    flat = np.ascontiguousarray(np.stack([np.asarray(c, np.float64).reshape(18) for c in cams]).astype(np.float32))
    return (hip.ViewCamera * len(cams)).from_buffer_copy(flat.tobytes())


GOOD_CAMS = _cam_array([R.view_camera((4, 6, 10), size=(45, 70)), R.view_camera((4, 6, 10), size=(45, 70), proj_type="ortho")])


def _bad_cam(index, value, proj_type="persp"):
    c = R.view_camera((4, 6, 10), size=(45, 70), proj_type=proj_type).reshape(18)
    c[index] = value
    return _cam_array([R.view_camera((4, 6, 10), size=(45, 70)), c])


def _eye(x, y, z):
    c = R.view_camera((4, 6, 10), size=(45, 70))
    c[0] = (x, y, z)
    return _cam_array([c])


def _args(**over):
    a = dict(vol=VOL, dtype=0, B=2, d0=4, d1=6, d2=10, th=-1.0, cams=GOOD_CAMS, n_cams=2, cams_ws=CAMS_WS, H=45, W=70, face=FACE, edge=EDGE, bg=BG,
             plate=None, mask=MASK, ids=IDS, rgb=RGB)
    a.update(over)
    host = lambda x: None if x is None else ctypes.addressof(x)              # noqa: E731
    return (a["vol"], a["dtype"], a["B"], a["d0"], a["d1"], a["d2"], a["th"], host(a["cams"]), a["n_cams"], a["cams_ws"], a["H"], a["W"],
            host(a["face"]), host(a["edge"]), host(a["bg"]), a["plate"], a["mask"], a["ids"], a["rgb"], None)


@pytest.mark.parametrize("what,over", [
    ("vol null", dict(vol=None)),
    ("cameras null", dict(cams=None)),
    ("camera scratch null", dict(cams_ws=None)),
    ("face colours null", dict(face=None)),
    ("edge colour null", dict(edge=None)),
    ("background null", dict(bg=None)),
    ("mask scratch null", dict(mask=None)),
    ("ids null", dict(ids=None)),
    ("ids null without rgb", dict(ids=None, rgb=None)),
    ("B = 0", dict(B=0)),
    ("B < 0", dict(B=-3)),
    ("n_cams = 0", dict(n_cams=0)),
    ("n_cams < 0", dict(n_cams=-1)),
    ("H = 0", dict(H=0)),
    ("W = 0", dict(W=0)),
    ("H < 0", dict(H=-45)),
    ("H W above 2^24", dict(H=4097, W=4096)),
    ("H W wraps an int", dict(H=1 << 16, W=1 << 16)),
    ("d0 = 0", dict(d0=0)),
    ("d1 < 0", dict(d1=-1)),
    ("d2 = 0", dict(d2=0)),
    ("d0 = 65", dict(d0=65)),
    ("d1 = 65", dict(d1=65)),
    ("d2 = 1024", dict(d2=1024)),
    ("dtype 2", dict(dtype=2)),
    ("dtype -1", dict(dtype=-1)),
    ("threshold 1", dict(th=1.0)),
    ("threshold above 1", dict(th=1.5)),
    ("threshold 0", dict(th=0.0)),
    ("threshold NaN", dict(th=float("nan"))),
    ("threshold with uint8", dict(dtype=1, th=0.5)),
    ("camera NaN origin", dict(cams=_bad_cam(1, float("nan")))),
    ("camera inf direction", dict(cams=_bad_cam(10, float("inf")))),
    ("camera -inf step", dict(cams=_bad_cam(17, float("-inf")))),
    ("ortho camera NaN", dict(cams=_bad_cam(4, float("nan"), "ortho"))),
    ("eye inside the box", dict(cams=_eye(2.0, 3.0, 5.0), n_cams=1)),
    ("eye on a face of the box", dict(cams=_eye(4.0, 3.0, 5.0), n_cams=1)),
    ("eye on a corner of the box", dict(cams=_eye(0.0, 0.0, 0.0), n_cams=1)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    rc = lib.sv_render_volumes(*_args(**over))
    assert rc == SV_ERR_INVALID, (what, rc)
    assert ENTRY in lib.sv_last_error().decode(), (what, lib.sv_last_error())


def test_python_refusals():
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.render_views_batch(torch.zeros(1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.render_views_batch(torch.zeros(1, 4, 4, 4), threshold=0.5, size=(8, 8))
    cfg = S.default_cfg()
    nets = [Encoder(cfg), Decoder(cfg), Merger(cfg), Refiner(cfg)]
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        harness.reconstruct(nets, cfg, torch.zeros(1, 1, 3, 224, 224), view_threshold=0.5, view_size=(45, 70))
    with pytest.raises(ValueError, match="proj_type"):
        D.view_camera((4, 4, 4), proj_type="fisheye")
    with pytest.raises(ValueError, match="dims"):
        D.view_camera((4, 0, 4))
    with pytest.raises(ValueError, match="dims"):
        D.view_camera((4, 4, 4), size=(0, 10))


# ---- camera --------------------------------------------------------------------------------------------------------------------------------
def test_view_camera_is_the_restatement():
    for dims in ((32, 32, 32), (31, 33, 32), (1, 1, 1), (5, 7, 3), (2, 2, 64)):
        for kw in ({}, dict(proj_type="ortho"), dict(elev=0, azim=0), dict(elev=-20, azim=160, size=(45, 70)), dict(elev=100, azim=10, size=(96, 96))):
            a, b = D.view_camera(dims, **kw), R.view_camera(dims, **kw)
            assert a.shape == (6, 3) and a.dtype == np.float64 and np.array_equal(a, b), (dims, kw)


@pytest.mark.parametrize("name", CASES)
def test_camera_is_the_one_matplotlib_used(name):
    """the eight corners of the box, put through the recorded get_proj() and transData, against the inverse map of view_camera's rays:
    corner = o0 + s (d0 + c dx + r dy) is linear in (s, s c, s r)"""
    vol, _, _, proj, trans = golden(name)
    cam = D.view_camera(vol.shape)
    assert not cam[1].any() and not cam[2].any()
    for corner in range(8):
        p = np.array([vol.shape[0] * (corner >> 2), vol.shape[1] * ((corner >> 1) & 1), vol.shape[2] * (corner & 1), 1.0])
        q = proj @ p
        xy = trans @ np.array([q[0] / q[3], q[1] / q[3], 1.0])
        col, row = xy[0], SIZE[0] - xy[1]                                       # display y runs upwards
        s = np.linalg.solve(np.stack([cam[3], cam[4], cam[5]], axis=1), p[:3] - cam[0])
        assert s[0] > 0 and abs(s[1] / s[0] - col) < 1e-6 and abs(s[2] / s[0] - row) < 1e-6, (corner, s[1] / s[0] - col, s[2] / s[0] - row)


def test_ortho_camera_has_one_direction():
    for dims in ((32, 32, 32), (31, 33, 32)):
        persp, ortho = D.view_camera(dims), D.view_camera(dims, proj_type="ortho")
        assert not ortho[4].any() and not ortho[5].any() and ortho[1].any() and ortho[2].any()
        # it looks along the perspective camera's central ray, the line from the eye to the centre of the box
        centre = 0.5 * np.asarray(dims, np.float64)
        assert np.allclose(np.cross(ortho[3], persp[0] - centre), 0.0, atol=1e-9)
        assert np.dot(ortho[3], centre - persp[0]) > 0
    level = D.view_camera((8, 8, 8), 0, 0, proj_type="ortho")
    assert level[3, 0] < 0 and level[3, 1] == 0 and level[3, 2] == 0           # direction components that are exactly zero


# ---- the restatement against the reference's pictures ----------------------------------------------------------------------------------
def test_fixture_is_intact():
    want = sorted([n + s for n in CASES for s in ("_dims", "_occ", "_image", "_offset", "_proj", "_trans")] +
                  ["plate_32x32x32", "plate_31x33x32", "face_rgb"])
    assert sorted(G.files) == want
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "volume_view_cases.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "bbox_crop_cases.npz"))
    for name in CASES:
        vol, img, plate, proj, trans = golden(name)
        assert img.shape == plate.shape == (3,) + SIZE and img.dtype == np.uint8 and proj.shape == (4, 4) and trans.shape == (3, 3)
        assert 0 < vol.sum() < vol.size
    assert golden("sphere")[0].sum() == 9328 and golden("rand31x33x32")[0].shape == (31, 33, 32)
    assert 0.04 < golden("rand31x33x32")[0].mean() < 0.06


def test_recorded_colours_are_the_default_table():
    assert G["face_rgb"].tolist() == [list(c) for c in D.VIEW_FACE_RGB]
    assert list(D.VIEW_FACE_RGB[1]) == list(D.VIEW_FACE_RGB[3]) == [13, 50, 75] and list(D.VIEW_FACE_RGB[5]) == [24, 91, 138]


@pytest.mark.parametrize("name", CASES)
def test_restatement_draws_the_reference_silhouette(name):
    _, img, plate, _, _ = golden(name)
    outside, inside = silhouette_exceptions(img, plate, golden_ids(name) >= 0)
    print(f"{name}: drawn pixels outside the dilated hit mask {outside}, eroded hit mask pixels not drawn {inside}")
    assert (outside, inside) == (0, 0)


@pytest.mark.parametrize("name", CASES)
def test_restatement_face_colours(name):
    _, img, _, _, _ = golden(name)
    ids = golden_ids(name)
    inner = R.uniform3x3(ids) & (ids >= 0)
    seen = set()
    for face in range(6):
        m = inner & (ids % 6 == face)
        if not m.any():
            continue
        seen.add(R.FACE_NAMES[face])
        share = float((np.abs(img[:, m].astype(np.int32) - G["face_rgb"][face][:, None].astype(np.int32)).max(axis=0) <= 2).mean())
        print(f"{name} {R.FACE_NAMES[face]}: {int(m.sum())} face-interior pixels, {share:.4f} within 2 levels of {G['face_rgb'][face].tolist()}")
        assert share >= MEASURED_SHARE[name][R.FACE_NAMES[face]] - 0.03, (name, face, share)
    assert seen == {"+x", "+y", "+z"}                                          # the faces the reference's view shows


# ---- sensitivity of the definition to its arithmetic -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_float32_and_float64_agree_on_the_fixtures(name):
    a, b = golden_ids(name), golden_ids(name, np.float64)
    n = int((a != b).sum())
    print(f"{name}: float32 and float64 ids differ in {n} of {a.size} pixels")
    assert n <= cap(SIZE)
    assert R.in_neighbourhood(a, b)[a != b].all()


@pytest.mark.parametrize("name", sorted(small_cases()))
def test_float32_and_float64_agree_on_the_small_cases(name):
    a, b = small_ids(name), small_ids(name, np.float64)
    size = small_cases()[name][2]
    per_image = (a != b).reshape(-1, size[0] * size[1]).sum(axis=1)
    print(f"{name}: float32 and float64 ids differ in at most {int(per_image.max())} of {size[0] * size[1]} pixels of an image ({int(per_image.sum())} in all)")
    assert per_image.max() <= cap(size)


def test_small_cases_cover_what_they_name():
    assert (small_ids("rand8_not_reached") == -1).all() and (small_ids("empty_full8")[0] == -1).all()
    full = small_ids("empty_full8")[1]
    assert set(np.unique(full[0] % 6)) - {5} == {1, 3} and (full >= -1).all()
    one = small_ids("one")
    assert set(np.unique(one[0, 0])) == {-1, 1, 3, 5} and set(np.unique(one[0, 3])) == {-1, 1}     # level ortho: the +x face alone
    sweep = small_ids("sweep8")
    for v in (0, 77, 511):                                                     # every volume shows its one voxel and nothing else
        assert set(np.unique(sweep[v, 0] // 6)) == {-1, v}
    assert all((small_ids(n) >= 0).any() for n in small_cases() if n != "rand8_not_reached")
    ids64 = small_ids("rand64")
    assert ids64.max() // 6 >= 64 * 64 * 32                                    # voxels of the upper half are seen: two-word rows, 32 KB mask


def test_shading_rule():
    ids = np.array([[-1, -1, 7, 7], [-1, 7, 7, 7], [13, 13, 7, 7], [13, 13, 7, 7]], np.int32)
    face = np.arange(18, dtype=np.uint8).reshape(6, 3) + 100
    rgb = R.shade(ids, face, edge_rgb=(1, 2, 3), background=(250, 251, 252))
    assert rgb.shape == (3, 4, 4) and rgb.dtype == np.uint8
    edge = np.array([[0, 1, 0, 0], [1, 1, 0, 0], [0, 1, 0, 0], [0, 1, 0, 0]], bool)
    assert np.array_equal(R.edge_mask(ids), edge)
    assert rgb[:, 0, 0].tolist() == [250, 251, 252] and rgb[:, 0, 1].tolist() == [1, 2, 3]
    assert rgb[:, 0, 2].tolist() == face[1].tolist() and rgb[:, 3, 0].tolist() == face[1].tolist() and rgb[:, 3, 3].tolist() == face[1].tolist()
    plate = np.arange(48, dtype=np.uint8).reshape(3, 4, 4)
    assert R.shade(ids, face, background=plate)[:, 0, 0].tolist() == plate[:, 0, 0].tolist()


# ---- data.image_file ---------------------------------------------------------------------------------------------------------------------
def _picture():
    ids = golden_ids("sphere")[140:341:5, 220:421:3]
    return R.shade(ids, D.VIEW_FACE_RGB)


def test_png_decodes_to_the_input():
    img = _picture()
    H, W = img.shape[1:]
    raw = D.image_file(img)
    assert raw == D.image_file(torch.from_numpy(img), "png")
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(raw):
        n, kind = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append((kind, body))
        pos += 12 + n
    assert pos == len(raw) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    assert chunks[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)           # 8-bit RGB, deflate, adaptive filtering, no interlace
    lines = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + 3 * W)
    assert not lines[:, 0].any()                                                 # filter 0 on every scanline: nothing to undo
    assert np.array_equal(lines[:, 1:].reshape(H, W, 3).transpose(2, 0, 1), img)


def test_ppm_round_trips_and_errors():
    img = _picture()
    H, W = img.shape[1:]
    raw = D.image_file(img, "ppm")
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert raw.startswith(head) and len(raw) == len(head) + 3 * H * W
    assert np.array_equal(np.frombuffer(raw[len(head):], np.uint8).reshape(H, W, 3).transpose(2, 0, 1), img)
    with pytest.raises(ValueError, match="format"):
        D.image_file(img, "gif")
    for bad in (img[0], img.astype(np.int32), img[:2], np.zeros((3, 0, 4), np.uint8)):
        with pytest.raises(ValueError, match="uint8"):
            D.image_file(bad)
