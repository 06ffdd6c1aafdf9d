"""Mesh voxelisation on the GPU (data.voxelise_mesh_batch / meshes_to_binvox -> sv_voxelise_meshes): every volume EQUAL, bit for bit, to
the numpy restatement of the rule (tests/mesh_voxel_ref.py, itself checked in test_cpu_mesh_voxelise.py) - the rule is integer arithmetic,
so there is no tolerance anywhere in this file - and, for the voxel surfaces sv_voxel_surface extracts, to the volume they came from."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_voxel_ref as MR  # noqa: E402
from test_cpu_voxel_surface import CASES, golden  # noqa: E402
from voxel_surface_ref import revoxelise  # noqa: E402

from swinvox_amd import data as D  # noqa: E402

S = MR.S


def units(verts):
    """snapped integers -> voxel units; exact in float64, and snapping gives the integers back"""
    return np.asarray(verts, np.float64) / S


def run(meshes, dims, mode, dev, **kw):
    vols, _, _ = D.voxelise_mesh_batch(meshes, dims, mode=mode, fit=None, device=dev, **kw)
    assert tuple(vols.shape) == (len(meshes), ) + tuple(dims)
    return vols.cpu().numpy()


# ---- round trip: the exposed faces of a volume enclose that volume ------------------------------------------------------------------
def _roundtrip_volumes():
    rng = np.random.default_rng(7)
    vols = {name: golden(name)[0] for name in CASES}
    vols["rand8_30"] = rng.random((8, 8, 8)) < 0.3
    vols["31x33x32_5"] = rng.random((31, 33, 32)) < 0.05
    vols["1x1x1"] = np.ones((1, 1, 1), bool)
    vols["2x2x64"] = rng.random((2, 2, 64)) < 0.5                            # two words per row
    vols["64_5"] = rng.random((64, 64, 64)) < 0.05
    x, y, z = np.indices((32, 32, 32))
    vols["checkerboard32"] = (x + y + z) % 2 == 0                            # 98 304 quads = 196 608 triangles: 192 chunks of one mesh
    return vols


ROUNDTRIP = _roundtrip_volumes()


@pytest.mark.parametrize("name", list(ROUNDTRIP))
def test_round_trip_through_the_voxel_surface(dev, name):
    vol = ROUNDTRIP[name]
    mesh, = D.extract_surface_batch(torch.from_numpy(vol[None]).to(dev))
    if name == "checkerboard32":
        assert 2 * len(mesh[1]) == 196608
    got = run([mesh], vol.shape, "solid", dev)[0]
    assert got.dtype == np.float32 and np.array_equal(got != 0, vol) and set(np.unique(got)) <= {0.0, 1.0}
    assert np.array_equal(got != 0, revoxelise(mesh[0], mesh[1], vol.shape))
    if vol.size <= 512:                                                      # the small ones also in the other modes, against the restatement
        tris = D.pack_meshes([mesh], vol.shape, fit=None)[0][3 * len(mesh[0]):-1].reshape(-1, 3)
        for mode in ("surface", "both"):
            assert np.array_equal(run([mesh], vol.shape, mode, dev)[0] != 0, MR.voxelise(mesh[0].astype(np.int64) * S, tris, vol.shape, mode)), mode


# ---- triangle soups and ties against the restatement ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def soup_case(dims, seed=1, n=200):
    verts, tris = MR.soup(dims, seed, n)
    return verts, tris, {mode: MR.voxelise(verts, tris, dims, mode, clip=n > 200) for mode in MR.MODES}


@pytest.mark.parametrize("mode", MR.MODES)
@pytest.mark.parametrize("dims", [(8, 8, 8), (5, 7, 3)])
def test_triangle_soup_equals_the_restatement(dev, dims, mode):
    verts, tris, want = soup_case(dims)
    assert len(tris) == 200
    got = run([(units(verts), tris)], dims, mode, dev)[0]
    assert np.array_equal(got != 0, want[mode]), int((got != 0).sum() - want[mode].sum())
    assert want[mode].any() and not want["solid"].all()


@pytest.mark.parametrize("name", list(MR.tie_cases()))
def test_tie_cases_equal_the_restatement(dev, name):
    verts, tris, dims = MR.tie_cases()[name]
    for mode in MR.MODES:
        assert np.array_equal(run([(units(verts), tris)], dims, mode, dev)[0] != 0, MR.voxelise(verts, tris, dims, mode)), mode


def test_triangle_order_and_chunk_boundaries_do_not_show(dev):
    """2 500 triangles are three chunks of one mesh; shuffled they fall into other chunks, and the one that spans the grid (worked on by
    the whole workgroup) into another place; split into meshes of 1 024, 1 and 1 475 triangles their volumes combine by XOR and OR."""
    dims = (8, 8, 8)
    verts, tris, want = soup_case(dims, seed=2, n=2500)
    perm = np.random.default_rng(0).permutation(len(tris))
    parts = [tris[:1024], tris[1024:1025], tris[1025:]]
    for mode in MR.MODES:
        whole = run([(units(verts), tris)], dims, mode, dev)[0] != 0
        assert np.array_equal(whole, want[mode]), mode
        assert np.array_equal(run([(units(verts), tris[perm])], dims, mode, dev)[0] != 0, whole), mode
    split = run([(units(verts), p) for p in parts], dims, "solid", dev) != 0
    assert np.array_equal(split[0] ^ split[1] ^ split[2], want["solid"])
    split = run([(units(verts), p) for p in parts], dims, "surface", dev) != 0
    assert np.array_equal(split[0] | split[1] | split[2], want["surface"])


# ---- batching, raggedness, dtypes ---------------------------------------------------------------------------------------------------------
def _ragged_batch():
    dims = (8, 8, 8)
    v1, t1, _ = soup_case(dims)
    v2, t2, dims2 = MR.tie_cases()["octahedron_apex_on_a_centre_column"]
    assert dims2 == dims
    empty = (np.zeros((0, 3)), np.zeros((0, 3), np.int64))
    return dims, [(units(v1), t1), (units(v2), t2), empty, (units(v1), t1[:7]), (np.zeros((4, 3)), np.zeros((0, 3), np.int64)), (units(v2), t2[::-1])]


def test_batched_equals_one_by_one_with_an_empty_mesh_in_the_middle(dev):
    dims, meshes = _ragged_batch()
    for mode in MR.MODES:
        together = run(meshes, dims, mode, dev)
        for i, m in enumerate(meshes):
            assert np.array_equal(together[i], run([m], dims, mode, dev)[0]), (mode, i)
        assert not together[2].any() and not together[4].any()              # no triangles: an empty volume
        assert np.array_equal(together[1], together[5])
    assert np.array_equal(together[0] != 0, soup_case(dims)[2]["both"])


def test_uint8_and_bool_equal_float32(dev):
    dims, meshes = _ragged_batch()
    f32 = run(meshes, dims, "both", dev)
    u8 = run(meshes, dims, "both", dev, dtype=torch.uint8)
    b = run(meshes, dims, "both", dev, dtype=torch.bool)
    assert u8.dtype == np.uint8 and b.dtype == np.bool_ and set(np.unique(u8)) <= {0, 1}
    assert np.array_equal(u8, f32.astype(np.uint8)) and np.array_equal(b, f32 != 0)


def test_an_out_of_range_triangle_index_raises_and_faults_nothing(dev):
    dims = (8, 8, 8)
    verts, tris, want = soup_case(dims)
    for wrong in (len(verts), -1, 2 ** 31 - 1, -2 ** 31, 2 ** 40):
        broken = tris.copy()
        broken[17, 1] = wrong
        with pytest.raises(ValueError, match="mesh 1: 1 face"):
            D.voxelise_mesh_batch([(units(verts), tris), (units(verts), broken)], dims, fit=None, device=dev)
    few = (units(verts[:30]), tris)                                          # 190 of the 200 faces name a vertex the mesh does not have
    with pytest.raises(ValueError, match="mesh 0: 190 face"):
        D.voxelise_mesh_batch([few, (units(verts), tris)], dims, fit=None, device=dev)
    assert np.array_equal(run([(units(verts), tris)], dims, "both", dev)[0] != 0, want["both"])   # and the device is as it was


# ---- files, fit, binvox ---------------------------------------------------------------------------------------------------------------
def test_mesh_files_with_a_fit_and_the_binvox_converter(dev):
    vol = ROUNDTRIP["rand8_30"]
    dims = vol.shape
    mesh, = D.extract_surface_batch(torch.from_numpy(vol[None]).to(dev))
    translate, scale = [-0.5, -0.25, 0.125], 2.0
    files = [D.mesh_file(mesh[0], mesh[1], fmt, dims, translate, scale) for fmt in ("ply", "off", "obj")]
    vols, trs, scs = D.voxelise_mesh_batch(files, dims, mode="solid", fit=(translate, scale), dtype=torch.bool, device=dev)
    assert trs == [translate] * 3 and scs == [scale] * 3
    assert all(np.array_equal(v, vol) for v in vols.cpu().numpy())
    # fitted to the bounding box, a transposed copy next to it: the converter's files decode to the same volumes and carry the fit
    verts, tris, _ = soup_case((8, 8, 8))
    swap = np.asarray([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)        # the reference's (2, 0, 1) transposition as a matrix
    meshes = [(verts * 0.37 + 5.0, tris), (verts[: 3 * 60] * 0.01, tris[:60])]
    for transform in (None, swap):
        vols, trs, scs = D.voxelise_mesh_batch(meshes, 16, fit="bbox", transform=transform, dtype=torch.uint8, device=dev)
        files = D.meshes_to_binvox(meshes, 16, fit="bbox", transform=transform, device=dev)
        assert torch.equal(D.decode_binvox_batch(files, dev), vols.float())
        for f, tr, sc, mesh in zip(files, trs, scs, meshes):
            hd, ht, hs, _ = D.parse_binvox_header(f)
            assert hd == [16, 16, 16] and ht == tr and hs == sc
            v = mesh[0] if transform is None else mesh[0] @ transform.T
            assert (tr, sc) == D.mesh_grid_fit(v, 16)
            packed = D.pack_meshes([(v, mesh[1])], 16, fit=(tr, sc))[0]
            want = MR.voxelise(packed[:3 * len(v)].reshape(-1, 3), mesh[1], (16, 16, 16), "both", clip=True)
        assert np.array_equal(vols[1].cpu().numpy() != 0, want)              # the last mesh against the restatement
    assert vols.any()
