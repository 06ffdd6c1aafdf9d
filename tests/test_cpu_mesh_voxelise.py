"""Host side of the mesh voxelisation (swinvox_amd/data.py: parse_mesh, mesh_grid_fit, snap_vertices, pack_meshes; sv_voxelise_meshes'
refusals) and the numpy restatement of its rule (tests/mesh_voxel_ref.py) against two checks that share none of its arithmetic: point in
polyhedron by orientation determinants for the solid mode, exact clipping with fractions.Fraction for the surface mode.  No GPU."""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from swinvox_amd import data as D
from swinvox_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_voxel_ref as MR  # noqa: E402
import voxel_surface_ref as VS  # noqa: E402

S, H = MR.S, MR.H


# ---- files ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["ply", "off", "obj"])
def test_parse_mesh_reads_back_what_mesh_file_writes(fmt):
    occ = np.random.default_rng(3).random((5, 4, 6)) < 0.3
    verts, quads = VS.surface(occ)
    v, t = D.parse_mesh(D.mesh_file(verts, quads, fmt))
    assert v.dtype == np.float64 and t.dtype == np.int64
    assert (v == verts).all()
    want = np.stack([quads[:, [0, 1, 2]], quads[:, [0, 2, 3]]], axis=1).reshape(-1, 3)      # each quad as its two triangles
    assert (t == want).all()
    v0, t0 = D.parse_mesh(D.mesh_file(np.zeros((0, 3)), np.zeros((0, 4), int), fmt))       # an empty mesh is a valid file
    assert v0.shape == (0, 3) and t0.shape == (0, 3)


def test_parse_mesh_off_forms():
    plain = b"OFF\n4 2 0\n0 0 0\n1 0 0\n1 1 0\n0 1 0.5\n3 0 1 2\n3 0 2 3\n"
    v, t = D.parse_mesh(plain)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.5]] and t.tolist() == [[0, 1, 2], [0, 2, 3]]
    commented = b"# made by hand\nOFF 5 2 0   # counts on the header line\n\n0 0 0\n1 0 0 # a vertex\n1 1 0\n0 1 0\n0.5 2 0\n#\n5 0 1 2 4 3\n3 0 1 2\n"
    v, t = D.parse_mesh(commented)
    assert len(v) == 5 and t.tolist() == [[0, 1, 2], [0, 2, 4], [0, 4, 3], [0, 1, 2]]      # the pentagon as a fan
    coff = b"COFF\n3 1 0\n0 0 0 255 0 0 255\n1 0 0 0 255 0 255\n0 1 0 0 0 255 255\n3 0 1 2 0.5 0.5 0.5\n"
    v, t = D.parse_mesh(coff)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0]] and t.tolist() == [[0, 1, 2]]
    with pytest.raises(ValueError, match="names vertex"):
        D.parse_mesh(b"OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n")
    with pytest.raises(ValueError, match="promises"):
        D.parse_mesh(b"OFF\n3 2 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 2\n")


def test_parse_mesh_obj_forms():
    obj = (b"# comment\nmtllib x.mtl\no thing\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\n"
           b"f 1 2 3\nf 1/1 3/1 4/1\nf 1/1/1 2/1/1 3/1/1 4/1/1\nf 1//1 2//1 4//1\nf -4 -3 -1\n"
           b"v 2 2 2 1.0\nf -1 1 2\n")
    v, t = D.parse_mesh(obj)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 2, 2]]
    assert t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 3], [4, 0, 1]]
    with pytest.raises(ValueError, match="index 0"):
        D.parse_mesh(b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n")
    with pytest.raises(ValueError, match="names vertex"):
        D.parse_mesh(b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")


def test_parse_mesh_ply_ascii_and_mixed_binary():
    ascii_ply = (b"ply\nformat ascii 1.0\ncomment by hand\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
                 b"property uchar red\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n"
                 b"0 0 0 9\n1 0 0 9\n1 1 0 9\n0 1 0 9\n4 0 1 2 3\n3 0 1 2\n")
    v, t = D.parse_mesh(ascii_ply)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]] and t.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 2]]
    head = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty double z\nproperty double y\nproperty double x\n"
            b"element face 2\nproperty list uchar ushort vertex_index\nend_header\n")
    body = np.asarray([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0.25, 1, 0]], "<f8").tobytes()            # z y x
    body += b"\x04" + np.asarray([0, 1, 2, 3], "<u2").tobytes() + b"\x03" + np.asarray([3, 2, 1], "<u2").tobytes()
    v, t = D.parse_mesh(head + body)
    assert v.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0.25]] and t.tolist() == [[0, 1, 2], [0, 2, 3], [3, 2, 1]]
    with pytest.raises(ValueError, match="neither ascii nor"):
        D.parse_mesh(b"ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n")


# ---- fit and snapping -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_mesh_grid_fit_maps_the_longest_side_onto_the_grid(axis):
    side = np.asarray([1.0, 2.0, 0.5])
    side[axis] = 5.0
    lo = np.asarray([-3.0, 10.0, 0.25])
    box = np.asarray([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)]) * side + lo
    tr, sc = D.mesh_grid_fit(box, 16)
    grid = (box - np.asarray(tr)) * 16 / sc                                                 # the .binvox header convention
    assert np.allclose(grid[:, axis].min(), 0.0, atol=1e-12) and np.allclose(grid[:, axis].max(), 16.0, atol=1e-12)
    assert np.allclose(0.5 * (grid.min(axis=0) + grid.max(axis=0)), 8.0, atol=1e-12)       # centred on every axis
    assert np.allclose(grid.max(axis=0) - grid.min(axis=0), side * 16 / 5.0, atol=1e-12)   # one scale for all axes
    tr, sc = D.mesh_grid_fit(box, 16, margin=0.125)
    grid = (box - np.asarray(tr)) * 16 / sc
    assert np.allclose([grid[:, axis].min(), grid[:, axis].max()], [2.0, 14.0], atol=1e-12)
    tr, sc = D.mesh_grid_fit(box, (8, 16, 32))                                              # not a cube: the side that fills its axis first decides
    grid = (box - np.asarray(tr)) * 32 / sc
    ext = grid.max(axis=0) - grid.min(axis=0)
    assert (ext <= np.asarray([8, 16, 32]) + 1e-9).all() and np.isclose(ext / np.asarray([8, 16, 32]), 1.0).any()
    assert np.allclose(0.5 * (grid.min(axis=0) + grid.max(axis=0)), [4, 8, 16], atol=1e-9)
    with pytest.raises(ValueError, match="at least one vertex"):
        D.mesh_grid_fit(np.zeros((0, 3)), 16)
    with pytest.raises(ValueError, match="margin"):
        D.mesh_grid_fit(box, 16, margin=0.5)


def test_snapping_rounds_half_up_and_refuses_what_lies_outside():
    g = np.asarray([[0.0, 1.0, 2.5], [0.5 / 1024, -0.5 / 1024, 1.49999 / 1024], [-8.0, 16.0, 3.0 + 1.5 / 1024]])
    assert D.snap_vertices(g, 8).tolist() == [[0, 1024, 2560], [1, 0, 1], [-8192, 16384, 3074]]  # floor(p S + 0.5): halves go up
    assert D.snap_vertices(g, 8).dtype == np.int32
    for bad, axis in (([16.001, 0, 0], 0), ([0, -8.001, 0], 1), ([0, 0, 1e9], 2)):
        with pytest.raises(ValueError, match=f"on axis {axis}, outside \\[-8, 16\\] voxels"):
            D.snap_vertices(np.asarray([bad]), 8)
    with pytest.raises(ValueError, match="outside \\[-2, 4\\]"):                             # the range is per axis
        D.snap_vertices(np.asarray([[0, 0, 5.0]]), (8, 8, 2))
    with pytest.raises(ValueError, match="not finite"):
        D.snap_vertices(np.asarray([[0, np.nan, 0]]), 8)


def test_pack_meshes_table_fit_and_transform():
    tri = (np.asarray([[0, 0, 0], [2, 0, 0], [0, 4, 0], [0, 0, 1.0]]), np.asarray([[0, 1, 2], [0, 1, 3]]))
    quad = (np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.int32), np.asarray([[0, 1, 2, 3]]))
    empty = (np.zeros((0, 3)), np.zeros((0, 3), int))
    packed, table, nv, nt, trs, scs = D.pack_meshes([tri, empty, quad], 8, fit=None)
    assert table.tolist() == [[0, 4, 0, 2], [4, 0, 2, 0], [4, 4, 2, 2]] and (nv, nt) == (8, 4)
    assert packed.dtype == np.int32 and len(packed) == 3 * nv + 3 * nt + 1
    assert packed[:12].tolist() == [0, 0, 0, 2048, 0, 0, 0, 4096, 0, 0, 0, 1024]
    assert packed[3 * nv:3 * nv + 12].tolist() == [0, 1, 2, 0, 1, 3, 0, 1, 2, 0, 2, 3]      # the quad as a fan
    assert trs == [[0.0, 0.0, 0.0]] * 3 and scs == [8.0] * 3                                # voxel units: grid = (p - 0) * 8 / 8
    packed, _, _, _, trs, scs = D.pack_meshes([tri], 8, fit="bbox")
    assert packed[:12].reshape(4, 3).tolist() == [[2048, 0, 3072], [6144, 0, 3072], [2048, 8192, 3072], [2048, 0, 5120]]
    assert trs == [[-1.0, 0.0, -1.5]] and scs == [4.0]
    packed, _, _, _, trs, scs = D.pack_meshes([tri], 8, fit=([1.0, 1.0, 1.0], 16.0))
    assert packed[:6].tolist() == [-512, -512, -512, 512, -512, -512]
    swap = np.asarray([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 2.0]])                         # the (2, 0, 1) transposition, then a shift
    packed, _, _, _, _, _ = D.pack_meshes([tri], 8, fit=None, transform=swap)
    assert packed[:12].reshape(4, 3).tolist() == [[0, 0, 2048], [0, 2048, 2048], [0, 0, 6144], [1024, 0, 2048]]
    with pytest.raises(ValueError, match="mesh 1: vertex 0 has coordinate 17"):
        D.pack_meshes([tri, (np.asarray([[17.0, 0, 0]]), empty[1])], 8, fit=None)
    with pytest.raises(ValueError, match="3 x 3 or 3 x 4"):
        D.pack_meshes([tri], 8, transform=np.eye(4))
    with pytest.raises(ValueError, match="no meshes"):
        D.pack_meshes([], 8)
    with pytest.raises(ValueError, match="1 .. 64"):
        D.pack_meshes([tri], 65)
    with pytest.raises(ValueError, match="k >= 3"):
        D.pack_meshes([(tri[0], np.asarray([[0, 1]]))], 8)
    with pytest.raises(ValueError, match="mode"):
        D.voxelise_mesh_batch([tri], 8, mode="filled")
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.voxelise_mesh_batch([tri], 8, device="cpu")


# ---- the C entry's refusals ---------------------------------------------------------------------------------------------------------
def test_the_entry_refuses_a_malformed_call_on_the_host():
    """Every refusal returns an error code with a message from the host-side checks; nothing is launched (no GPU is needed here)."""
    lib = hip.load()
    assert "sv_voxelise_meshes" in hip.EXPORTED_SYMBOLS and "sv_voxelise_meshes_workspace_bytes" in hip.EXPORTED_SYMBOLS

    def refused(match, table=((0, 4, 0, 2), ), null=(), **kw):
        tab = (ctypes.c_longlong * (4 * len(table)))(*[x for row in table for x in row])
        a = dict(verts=0x1000, total_verts=4, tris=0x2000, total_tris=2, mesh_table=ctypes.addressof(tab), B=len(table), d0=8, d1=8, d2=8, mode=2,
                 out_dtype=0, out=0x3000, workspace=0x4000, stream=None)       # dummy device addresses, never dereferenced
        a.update(kw)
        for k in null:
            a[k] = None
        rc = lib.sv_voxelise_meshes(*a.values())
        msg = lib.sv_last_error().decode()
        assert rc != 0 and match in msg, (rc, msg)

    refused("vertex offset", table=((1, 4, 0, 2), ))                         # one vertex past the buffer
    refused("vertex offset", table=((-1, 2, 0, 2), ))
    refused("vertex offset", table=((0, -1, 0, 2), ))
    refused("vertex offset", table=((0, 4, 0, 2), (4, 1, 0, 0)))
    refused("triangle offset", table=((0, 4, 1, 2), ))
    refused("triangle offset", table=((0, 4, 0, 3), ))
    refused("triangle offset", table=((0, 4, -2, 1), ))
    refused("triangle offset", table=((0, 4, 0, 1 << 62), ))                 # no overflow in offset + count
    refused("2^31 - 1", table=((0, 1 << 31, 0, 2), ), total_verts=1 << 32)
    refused("every dim must lie in 1 .. 64", d0=0)
    refused("every dim must lie in 1 .. 64", d1=65)
    refused("every dim must lie in 1 .. 64", d2=-3)
    refused("mode", mode=3)
    refused("mode", mode=-1)
    refused("out_dtype", out_dtype=2)
    refused("meshes", B=0)
    refused("meshes", B=70000)
    refused("bad arguments", null=("out", ))
    refused("bad arguments", null=("workspace", ))
    refused("bad arguments", null=("mesh_table", ))
    refused("buffers of", null=("verts", ))                                  # vertices promised, no buffer
    refused("buffers of", null=("tris", ))
    refused("buffers of", total_tris=-1)
    refused("8-byte aligned", workspace=0x4004)
    q = lib.sv_voxelise_meshes_workspace_bytes
    assert q(3, 32, 32, 32) == 3 * 32 + 16 + 3 * 2 * 32 * 32 * 4                # table, counters padded to 8 bytes, two masks per mesh
    assert q(1, 2, 2, 64) == 32 + 8 + 2 * 2 * 2 * 2 * 4                         # two words per row above 32
    assert q(0, 8, 8, 8) == 0 and q(1, 8, 65, 8) == 0 and q(1, 0, 8, 8) == 0


# ---- the restatement against independent checks ----------------------------------------------------------------------------------------
def _det3(u, v, w):
    return (u[..., 0] * (v[..., 1] * w[..., 2] - v[..., 2] * w[..., 1]) - u[..., 1] * (v[..., 0] * w[..., 2] - v[..., 2] * w[..., 0]) +
            u[..., 2] * (v[..., 0] * w[..., 1] - v[..., 1] * w[..., 0]))


def _in_tetrahedron(P, tet):
    """P int64 [..., 3], tet int64 [4, 3] -> (strictly inside, on the closed boundary) by four orientation determinants"""
    a, b, c, d = tet
    o = int(_det3(b - a, c - a, d - a))
    assert o != 0
    s = 1 if o > 0 else -1                                 # P in the place of each vertex in turn keeps the orientation iff P is inside
    dets = [s * _det3(b - P, c - P, d - P), s * _det3(P - a, c - a, d - a), s * _det3(b - a, P - a, d - a), s * _det3(b - a, c - a, P - a)]
    inside = np.logical_and.reduce([x > 0 for x in dets])
    closed = np.logical_and.reduce([x >= 0 for x in dets])
    return inside, closed & ~inside


TET_FACES = np.asarray([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])


def _centres(dims):
    g = np.stack(np.meshgrid(*[(2 * np.arange(d, dtype=np.int64) + 1) * H for d in dims], indexing="ij"), axis=-1)
    return g


def test_determinant_check_knows_a_corner_tetrahedron():
    tet = np.asarray([[0, 0, 0], [4 * S, 0, 0], [0, 4 * S, 0], [0, 0, 4 * S]], np.int64)
    inside, on = _in_tetrahedron(_centres((8, 8, 8)), tet)
    i, j, k = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    assert (inside == (i + j + k + 1.5 < 4)).all() and (on == (2 * (i + j + k) + 3 == 8)).all()


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_solid_restatement_against_point_in_polyhedron(seed):
    """One tetrahedron anywhere in an 8-grid (even seeds) or two disjoint ones, left and right of x = 4 (odd seeds), faces in random
    orientation and order.  Compared at the centres that lie on no face - a condition, not a tolerance: at most 1 % are excluded."""
    rng = np.random.default_rng(seed)
    dims = (8, 8, 8)
    tets = []
    for half in ((0, 8), ) if seed % 2 == 0 else ((0, 4), (4, 8)):
        while True:
            tet = np.stack([rng.integers(half[0] * S, half[1] * S + 1, 4), rng.integers(0, 8 * S + 1, 4), rng.integers(0, 8 * S + 1, 4)], axis=1)
            if abs(int(_det3(tet[1] - tet[0], tet[2] - tet[0], tet[3] - tet[0]))) > 6 * (2 * S) ** 3:   # at least a few voxels of volume
                break
        tets.append(tet.astype(np.int64))
    verts = np.concatenate(tets)
    tris = np.concatenate([TET_FACES + 4 * n for n in range(len(tets))])
    tris = np.stack([t[::-1] if rng.random() < 0.5 else np.roll(t, rng.integers(0, 3)) for t in tris])[rng.permutation(len(tris))]
    P = _centres(dims)
    inside, on = np.zeros(dims, bool), np.zeros(dims, bool)
    for tet in tets:
        i, o = _in_tetrahedron(P, tet)
        inside |= i
        on |= o
    assert on.mean() <= 0.01 and inside.sum() >= 6
    got = MR.solid(verts, tris, dims)
    assert (got[~on] == inside[~on]).all()
    assert (MR.solid(verts, tris, dims, clip=True) == got).all()


def _clip_polygon(poly, axis, bound, keep_above):
    """Sutherland-Hodgman against one closed half-space, exact: points are triples of Fractions"""
    def inside(p):
        return p[axis] >= bound if keep_above else p[axis] <= bound
    out = []
    for n, cur in enumerate(poly):
        nxt = poly[(n + 1) % len(poly)]
        if inside(cur):
            out.append(cur)
        if inside(cur) != inside(nxt):
            t = (bound - cur[axis]) / (nxt[axis] - cur[axis])
            out.append(tuple(c + t * (m - c) for c, m in zip(cur, nxt)))
    return out


def _cube_meets_triangle(tri, ijk):
    poly = [tuple(Fraction(int(x)) for x in p) for p in tri]
    for axis in range(3):
        for bound, above in ((ijk[axis] * S, True), ((ijk[axis] + 1) * S, False)):
            poly = _clip_polygon(poly, axis, Fraction(bound), above)
            if not poly:
                return False
    return True


def _surface_by_clipping(verts, tris, dims):
    out = np.zeros(dims, bool)
    for t in tris:
        tri = verts[t]
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        if not n.any():
            continue
        for ijk in np.ndindex(*dims):
            if not out[ijk]:
                out[ijk] = _cube_meets_triangle(tri, ijk)
    return out


def test_surface_restatement_against_exact_clipping():
    rng = np.random.default_rng(21)
    dims = (8, 8, 8)
    pts = [rng.integers(0, 8 * S + 1, (3, 3)) for _ in range(4)]                             # anywhere
    pts += [rng.integers(0, 17, (3, 3)) * H for _ in range(4)]                               # on the half-voxel lattice: touching cases
    pts += [rng.integers(0, 8, 3) * S + rng.integers(1, S, (3, 3)) for _ in range(2)]        # inside one voxel
    pts.append(np.asarray([[2 * S, S, S], [2 * S, 5 * S, S], [2 * S, S, 6 * S]]))            # in a lattice plane: both sides
    pts.append(np.asarray([[-3 * S, -2 * S, 9 * S], [11 * S, 3 * S, -S], [S, 12 * S, 4 * S]]))   # vertices outside the grid
    a, b = rng.integers(0, 8 * S + 1, (2, 3))
    pts.append(np.asarray([a, b, (a + b) // 2 + [0, 1, 0]]))                                  # a sliver
    pts.append(np.asarray([[S, S, S], [3 * S, 3 * S, 3 * S], [2 * S, 2 * S, 2 * S]]))        # zero normal: skipped
    for tri in pts:
        verts, tris = np.asarray(tri, np.int64), np.asarray([[0, 1, 2]])
        got = MR.surface(verts, tris, dims)
        assert (got == _surface_by_clipping(verts, tris, dims)).all()
        assert (MR.surface(verts, tris, dims, clip=True) == got).all()
    plane = MR.surface(np.asarray(pts[10], np.int64), np.asarray([[0, 1, 2]]), dims)
    assert plane[1].any() and plane[2].any() and (plane[1] == plane[2]).all() and not plane[0].any() and not plane[3].any()
    assert not MR.surface(np.asarray(pts[-1], np.int64), np.asarray([[0, 1, 2]]), dims).any()


@pytest.mark.parametrize("dims", [(8, 8, 8), (5, 7, 3)])
def test_clipping_the_restatement_to_bounding_boxes_changes_nothing(dims):
    verts, tris = MR.soup(dims, seed=5)
    for mode in MR.MODES:
        assert (MR.voxelise(verts, tris, dims, mode, clip=True) == MR.voxelise(verts, tris, dims, mode)).all()
    assert (MR.voxelise(verts, tris, dims, "both") == (MR.solid(verts, tris, dims) | MR.surface(verts, tris, dims))).all()


# ---- ties, by the written rule -----------------------------------------------------------------------------------------------------------
def test_tie_octahedron_with_an_apex_on_a_centre_column():
    verts, tris, dims = MR.tie_cases()["octahedron_apex_on_a_centre_column"]
    got = MR.solid(verts, tris, dims)
    # the apexes sit on the column of voxel (4, 4) and every slanted edge runs over a row of centres: whichever triangles own those ties,
    # a closed surface toggles every column an even number of times - nothing leaks to the top of the grid
    assert not got[:, :, 7].any() and not got[:, :, 0].any()
    c = np.asarray([9 * H, 9 * H, 4 * S + 3])
    P = _centres(dims)
    inside = np.zeros(dims, bool)
    on = np.zeros(dims, bool)
    for t in tris:                                                                           # the octahedron as eight tetrahedra about its centre
        i, o = _in_tetrahedron(P, np.concatenate([verts[t], c[None]]))
        inside |= i
        on |= o
    on &= ~inside                                                                            # inner faces of the decomposition: decided by hand below
    assert (got[~on] == inside[~on]).all()
    assert got[4, 4, 1:7].all() and not got[4, 4, 7] and not got[4, 4, 0]                    # the apex column: centres 1.5 .. 6.5 lie between the apexes
    alone = [int(MR.solid(verts, t[None], dims)[4, 4, 7]) for t in tris]                     # which faces, taken alone, cover the apex column
    assert sum(alone[:4]) == 1 and sum(alone[4:]) == 1                                       # one of the four lower and one of the four upper


def test_tie_edge_along_a_column_line():
    verts, tris, dims = MR.tie_cases()["edge_along_a_column_line"]
    got = MR.solid(verts, tris, dims)
    # the ridge x = 4.5 voxels lies on the centres of row i = 4; exactly one of the two roof planes owns each of them, so with the floor
    # (z = 1 voxel) every covered column is toggled twice: set from k = 1 up to the roof, nothing above it
    roof_height = {1: 3, 2: 4, 3: 5, 4: 6, 5: 4, 6: 3}                                        # first k whose centre lies above the roof, per i
    for i in range(8):
        for j in range(8):
            want = np.zeros(8, bool)
            if i in roof_height and 1 <= j <= 6:
                want[1:roof_height[i]] = True
            assert (got[i, j] == want).all(), (i, j, got[i, j])
    owners = [int(MR.solid(verts, t[None], dims)[4, 3, 7]) for t in tris[:4]]
    assert sum(owners) == 1                                                                   # the ridge column belongs to one roof triangle


def test_tie_centre_on_a_triangle_plane():
    verts, tris, dims = MR.tie_cases()["centre_on_a_triangle_plane"]
    got = MR.solid(verts, tris, dims)
    want = np.zeros(dims, bool)
    want[1:3, 1:3, 2:4] = True                       # bottom at the centre of k = 1: not strictly below it, so k = 1 stays empty; top at k = 3: set
    assert (got == want).all()
    both = MR.voxelise(verts, tris, dims, "both")
    shell = np.zeros(dims, bool)
    shell[0:4, 0:4, 1:4] = True                      # the closed box [1, 3]^2 x [1.5, 3.5] touches the cubes around it
    assert (both == shell).all()
