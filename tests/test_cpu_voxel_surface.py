"""The exposed-voxel-face mesh (csrc/dataprep.hip sv_voxel_surface, data.extract_surface_batch / mesh_file / encode_mesh_batch)
without a GPU: the header declares the entry and cites what the reference draws, the ctypes table binds it, the argument refusals -
host-side checks that run before any GPU call - answer SV_ERR_INVALID with the entry's name, the fixtures
(tests/golden/voxel_surface_cases.npz, the face sets matplotlib's Axes3D.voxels builds, which is what utils/helpers.py:50-88 calls)
are intact and equal to the numpy restatement (tests/voxel_surface_ref.py, the expected value of test_gpu_voxel_surface.py), the
restatement's meshes are closed, outward-oriented and enclose the filled voxels, and data.mesh_file writes PLY / OFF / OBJ."""
import ctypes
import os
import re
import struct
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from voxel_surface_ref import canonical_faces, revoxelise, surface, used_by_cells  # noqa: E402

from swinvox_amd import data as D  # noqa: E402
from swinvox_amd import hip  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "voxel_surface_cases.npz"))
CASES = ("one", "rand2x3x4", "rand5x4x3", "rand7x2x5", "rand8", "full4", "dense6", "empty3")
ENTRY = "sv_voxel_surface"
SV_ERR_INVALID = -1
ONE_VERTS = [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 1], [1, 1, 0], [1, 1, 1]]
ONE_FACES = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]


def golden(name):
    """(bool volume, canonical [m, 4, 3] face set matplotlib built) of a fixture"""
    dims = [int(d) for d in G[name + "_dims"]]
    return np.unpackbits(G[name + "_occ"])[:int(np.prod(dims))].astype(bool).reshape(dims), G[name + "_faces"]


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\bint\s+" + ENTRY + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
    assert m, f"{ENTRY} is not declared"
    comment = (m.group(1) or "") + (m.group(2) or "")
    for cite in ("utils/helpers.py:50-88", "core/test.py:178-187", "utils/binvox_rw.py:306-343"):
        assert cite in comment, cite
    assert "-x, +x, -y, +y, -z, +z" in comment and "(x*d1 + y)*d2 + z" in comment and "(i*(d1+1) + j)*(d2+1) + k" in comment
    assert "counter-clockwise" in comment


def test_exported_and_bound():
    assert ENTRY in hip.EXPORTED_SYMBOLS
    lib = hip.load()                          # dlopen only: no GPU call is made
    at = lib.sv_voxel_surface.argtypes
    assert len(hip._argtypes(ENTRY)) == 13 and len(at) == 13
    assert at[6] is ctypes.c_float and at[8] is ctypes.c_longlong and at[10] is ctypes.c_longlong
    assert all(at[i] is ctypes.c_int for i in range(1, 6)) and all(at[i] is ctypes.c_void_p for i in (0, 7, 9, 11, 12))


# fake, suitably aligned device addresses: every call below is refused before anything could read them
VOL, VERTS, FACES, COUNTS = (0x10000 * (i + 1) for i in range(4))
VCAP, FCAP = 5 * 7 * 11, 3 * 240 + 24 + 60 + 40


def _args(**over):
    a = dict(vol=VOL, dtype=0, B=2, d0=4, d1=6, d2=10, th=-1.0, verts=VERTS, vcap=VCAP, faces=FACES, fcap=FCAP, counts=COUNTS)
    a.update(over)
    return (a["vol"], a["dtype"], a["B"], a["d0"], a["d1"], a["d2"], a["th"], a["verts"], a["vcap"], a["faces"], a["fcap"], a["counts"],
            None)


@pytest.mark.parametrize("what,over", [
    ("vol null", dict(vol=None)),
    ("verts null", dict(verts=None)),
    ("faces null", dict(faces=None)),
    ("counts null", dict(counts=None)),
    ("B = 0", dict(B=0)),
    ("B < 0", dict(B=-3)),
    ("d0 = 0", dict(d0=0)),
    ("d1 < 0", dict(d1=-1)),
    ("d2 = 0", dict(d2=0)),
    ("d0 = 65", dict(d0=65, vcap=1 << 20, fcap=1 << 20)),
    ("d1 = 65", dict(d1=65, vcap=1 << 20, fcap=1 << 20)),
    ("d2 = 1024", dict(d2=1024, vcap=1 << 24, fcap=1 << 24)),
    ("dtype 2", dict(dtype=2)),
    ("dtype -1", dict(dtype=-1)),
    ("threshold 1", dict(th=1.0)),
    ("threshold above 1", dict(th=1.5)),
    ("threshold 0", dict(th=0.0)),
    ("threshold NaN", dict(th=float("nan"))),
    ("threshold with uint8", dict(dtype=1, th=0.5)),
    ("vertex capacity one short", dict(vcap=VCAP - 1)),
    ("vertex capacity 0", dict(vcap=0)),
    ("face capacity one short", dict(fcap=FCAP - 1)),
    ("face capacity 0", dict(fcap=0)),
    ("face capacity of the voxel count only", dict(fcap=240)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    rc = lib.sv_voxel_surface(*_args(**over))
    assert rc == SV_ERR_INVALID, (what, rc)
    assert ENTRY in lib.sv_last_error().decode(), (what, lib.sv_last_error())


def test_extract_rejects_cpu_tensors():
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.extract_surface_batch(torch.zeros(1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.encode_mesh_batch(torch.zeros(1, 4, 4, 4))


# ---- fixture and restatement ------------------------------------------------------------------------------------------------
def test_fixture_is_intact():
    assert sorted(G.files) == sorted(n + s for n in CASES for s in ("_dims", "_occ", "_faces"))
    want = {"one": ((1, 1, 1), 1, 6), "full4": ((4, 4, 4), 64, 96), "empty3": ((3, 3, 3), 0, 0), "rand2x3x4": ((2, 3, 4), None, None),
            "rand5x4x3": ((5, 4, 3), None, None), "rand7x2x5": ((7, 2, 5), None, None), "rand8": ((8, 8, 8), None, None),
            "dense6": ((6, 6, 6), None, None)}
    for name in CASES:
        vol, faces = golden(name)
        dims, filled, n_faces = want[name]
        assert vol.shape == dims and faces.ndim == 3 and faces.shape[1:] == (4, 3) and faces.dtype == np.int16, name
        assert filled is None or (int(vol.sum()), len(faces)) == (filled, n_faces), name
        assert np.array_equal(canonical_faces(faces), faces), name                      # stored in canonical order
        assert len(np.unique(faces.reshape(len(faces), 12), axis=0)) == len(faces), name   # a set: no face twice
        assert faces.size == 0 or (faces.min() >= 0 and (faces.max(axis=(0, 1)) <= np.asarray(dims)).all()), name
    assert 0.6 < golden("dense6")[0].mean() < 0.8 and 0 < golden("rand8")[0].sum() < 512


@pytest.mark.parametrize("name", CASES)
def test_restatement_draws_what_matplotlib_draws(name):
    vol, faces = golden(name)
    verts, quads = surface(vol)
    assert verts.dtype == np.int32 and quads.dtype == np.int32 and verts.shape[1:] == (3,) and quads.shape[1:] == (4,)
    assert np.array_equal(canonical_faces(verts[quads]), faces)


def test_one_voxel_literal():
    verts, faces = surface(np.ones((1, 1, 1), bool))
    assert verts.tolist() == ONE_VERTS and faces.tolist() == ONE_FACES


def random_volumes():
    rng = np.random.default_rng(11)
    for shape, p in (((1, 1, 1), 1.0), ((3, 1, 2), 0.5), ((4, 6, 10), 0.3), ((9, 7, 5), 0.7), ((16, 16, 16), 0.5), ((31, 33, 32), 0.1),
                     ((12, 12, 12), 0.95), ((5, 5, 5), 0.0)):
        yield rng.random(shape) < p


def test_restatement_invariants():
    for vol in random_volumes():
        d0, d1, d2 = vol.shape
        verts, faces = surface(vol)
        n_exposed = sum(int((np.pad(vol, 1)[1 + a:1 + a + d0, 1 + b:1 + b + d1, 1 + c:1 + c + d2] < vol).sum())
                        for a, b, c in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)))
        assert len(faces) == n_exposed <= 3 * d0 * d1 * d2 + d0 * d1 + d1 * d2 + d0 * d2
        assert len(verts) <= (d0 + 1) * (d1 + 1) * (d2 + 1)
        # vertices: strictly ascending lattice index, every one referenced, and exactly the points the 8-cell rule names
        lat = (verts[:, 0].astype(np.int64) * (d1 + 1) + verts[:, 1]) * (d2 + 1) + verts[:, 2]
        assert (np.diff(lat) > 0).all()
        assert np.array_equal(np.unique(faces), np.arange(len(verts)))
        assert np.array_equal(np.flatnonzero(used_by_cells(vol).reshape(-1)), lat)
        # 6 x signed volume, in integers: each quad (a, b, c, d) as the triangles (a, b, c) and (a, c, d)
        q = verts.astype(np.int64)[faces]
        det = lambda a, b, c: np.einsum("ni,ni->n", a, np.cross(b, c))               # noqa: E731
        six_v = int(det(q[:, 0], q[:, 1], q[:, 2]).sum() + det(q[:, 0], q[:, 2], q[:, 3]).sum()) if len(q) else 0
        assert six_v == 6 * int(vol.sum())
        # closed and consistently oriented: every directed edge occurs as often as its reverse
        e = np.stack([faces, np.roll(faces, -1, axis=1)], axis=2).reshape(-1, 2).astype(np.int64)
        fwd, n_fwd = np.unique(e[:, 0] * (len(verts) + 1) + e[:, 1], return_counts=True)
        rev, n_rev = np.unique(e[:, 1] * (len(verts) + 1) + e[:, 0], return_counts=True)
        assert np.array_equal(fwd, rev) and np.array_equal(n_fwd, n_rev)
        # the +-z faces alone give the volume back (the round trip the GPU test makes against the binvox writer)
        assert np.array_equal(revoxelise(verts, faces, vol.shape), vol)


def test_face_order_is_voxel_then_direction():
    vol = np.zeros((3, 3, 3), bool)
    vol[0, 2, 1] = vol[1, 1, 1] = vol[2, 0, 0] = True                                # three isolated voxels: 6 faces each, in voxel order
    verts, faces = surface(vol)
    assert len(faces) == 18
    for n, (x, y, z) in enumerate(((0, 2, 1), (1, 1, 1), (2, 0, 0))):
        cube = verts[faces[6 * n:6 * n + 6]] - np.asarray([x, y, z])
        lone_v, lone_f = surface(np.ones((1, 1, 1), bool))
        assert np.array_equal(cube, lone_v[lone_f])


# ---- data.mesh_file ---------------------------------------------------------------------------------------------------------
def parse_ply(raw):
    head, _, body = raw.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "comment swinvox_amd exposed voxel faces"]
    n, m = int(lines[3].split()[2]), int(lines[7].split()[2])
    assert lines[3:] == [f"element vertex {n}", "property float x", "property float y", "property float z", f"element face {m}",
                         "property list uchar int vertex_indices", ""]
    assert len(body) == 12 * n + 17 * m
    xyz = np.frombuffer(body[:12 * n], "<f4").reshape(n, 3)
    rec = np.frombuffer(body[12 * n:], np.dtype([("n", "u1"), ("v", "<i4", (4,))]))
    assert (rec["n"] == 4).all()
    return xyz, rec["v"].reshape(m, 4)


def parse_off(raw):
    lines = raw.decode("ascii").split("\n")
    assert lines[0] == "OFF" and lines[-1] == ""
    n, m, zero = map(int, lines[1].split())
    assert zero == 0 and len(lines) == 3 + n + m
    xyz = np.asarray([list(map(float, ln.split())) for ln in lines[2:2 + n]], np.float64).reshape(n, 3)
    rows = [list(map(int, ln.split())) for ln in lines[2 + n:2 + n + m]]
    assert all(r[0] == 4 and len(r) == 5 for r in rows)
    return xyz, np.asarray([r[1:] for r in rows], np.int64).reshape(m, 4)


def parse_obj(raw):
    lines = raw.decode("ascii").split("\n")
    assert lines[-1] == ""
    v = [ln.split()[1:] for ln in lines if ln.startswith("v ")]
    f = [ln.split()[1:] for ln in lines if ln.startswith("f ")]
    assert len(v) + len(f) == len(lines) - 1
    return np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 4) - 1


PARSERS = {"ply": parse_ply, "off": parse_off, "obj": parse_obj}


def test_ply_of_one_voxel_is_these_bytes():
    want = (b"ply\nformat binary_little_endian 1.0\ncomment swinvox_amd exposed voxel faces\nelement vertex 8\n"
            b"property float x\nproperty float y\nproperty float z\nelement face 6\nproperty list uchar int vertex_indices\nend_header\n")
    want += b"".join(struct.pack("<3f", *v) for v in ONE_VERTS)
    want += b"".join(struct.pack("<B4i", 4, *f) for f in ONE_FACES)
    assert len(want) - want.index(b"end_header\n") - 11 == 8 * 12 + 6 * 17
    assert D.mesh_file(np.asarray(ONE_VERTS, np.int32), np.asarray(ONE_FACES, np.int32)) == want
    assert D.mesh_file(ONE_VERTS, ONE_FACES, "ply") == want


@pytest.mark.parametrize("fmt", ["ply", "off", "obj"])
def test_mesh_file_parses_back(fmt):
    vol = np.random.default_rng(4).random((4, 6, 10)) < 0.35
    verts, faces = surface(vol)
    xyz, quads = PARSERS[fmt](D.mesh_file(verts, faces, fmt))
    assert np.array_equal(xyz, verts) and np.array_equal(quads, faces)                 # lattice units without a scale
    tr, sc = (-0.5, 0.25, 2.0), 0.75
    want = np.asarray(tr, np.float64)[None] + sc * verts.astype(np.float64) / 10.0     # max(dims) = 10
    xyz, quads = PARSERS[fmt](D.mesh_file(verts, faces, fmt, dims=vol.shape, translate=tr, scale=sc))
    assert np.array_equal(quads, faces)
    if fmt == "ply":
        assert np.array_equal(xyz, want.astype(np.float32))
    else:
        assert np.array_equal(xyz, np.asarray([[float("%.9g" % c) for c in p] for p in want]))
        assert np.abs(xyz - want).max() <= 5e-9 * np.abs(want).max()                   # %.9g: nine significant digits
    unit, _ = PARSERS[fmt](D.mesh_file(verts, faces, fmt, dims=vol.shape, scale=1.0))
    assert unit.max() == 1.0 and unit.min() >= 0.0                                     # normalised to the largest dimension


def test_mesh_file_empty_and_errors():
    none_v, none_f = surface(np.zeros((3, 3, 3), bool))
    assert none_v.shape == (0, 3) and none_f.shape == (0, 4)
    for fmt in PARSERS:
        for kw in ({}, dict(dims=(3, 3, 3), translate=(1.0, 2.0, 3.0), scale=2.0)):
            xyz, quads = PARSERS[fmt](D.mesh_file(none_v, none_f, fmt, **kw))
            assert xyz.shape == (0, 3) and quads.shape == (0, 4)
    assert D.mesh_file(none_v, none_f, "off") == b"OFF\n0 0 0\n" and D.mesh_file(none_v, none_f, "obj") == b""
    with pytest.raises(ValueError, match="format"):
        D.mesh_file(ONE_VERTS, ONE_FACES, "stl")
    with pytest.raises(ValueError, match="dims"):
        D.mesh_file(ONE_VERTS, ONE_FACES, scale=1.0)
    with pytest.raises(ValueError, match="translate needs a scale"):
        D.mesh_file(ONE_VERTS, ONE_FACES, translate=(1.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="outside the vertex list"):
        D.mesh_file(ONE_VERTS[:7], ONE_FACES)
