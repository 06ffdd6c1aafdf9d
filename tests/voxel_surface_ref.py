"""Numpy restatement of the exposed-voxel-face mesh (sv_voxel_surface in include/swinvox_hip.h): the expected value of
test_cpu_voxel_surface.py and test_gpu_voxel_surface.py.  Test infrastructure only; the product does not import it.

  exposed face  voxel (x, y, z) is filled and its neighbour in the direction is empty or outside; directions -x +x -y +y -z +z
  face order    ascending voxel index (x * d1 + y) * d2 + z, then direction
  corners       CORNERS[direction] added to (x, y, z), counter-clockwise seen from outside
  vertices      the lattice points that are a corner of an exposed face, each once, ascending (i * (d1 + 1) + j) * (d2 + 1) + k
"""
import numpy as np

DIRS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
CORNERS = (((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)),
           ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)),
           ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)),
           ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)),
           ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)),
           ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)))


def surface(occ):
    """bool [d0, d1, d2] -> (verts int32 [n, 3], faces int32 [m, 4])"""
    occ = np.asarray(occ).astype(bool)
    d0, d1, d2 = occ.shape
    pad = np.pad(occ, 1)
    voxel = np.arange(occ.size).reshape(occ.shape)
    keys, quads = [], []
    for d, (dx, dy, dz) in enumerate(DIRS):
        neighbour = pad[1 + dx:1 + dx + d0, 1 + dy:1 + dy + d1, 1 + dz:1 + dz + d2]
        x, y, z = np.nonzero(occ & ~neighbour)
        keys.append(voxel[x, y, z] * 6 + d)
        quads.append(np.stack([x, y, z], axis=1)[:, None, :] + np.asarray(CORNERS[d])[None])
    quads = np.concatenate(quads)[np.argsort(np.concatenate(keys), kind="stable")]          # [m, 4, 3]
    lat = (quads[..., 0] * (d1 + 1) + quads[..., 1]) * (d2 + 1) + quads[..., 2]
    used = np.unique(lat)                                                                   # ascending, each once
    verts = np.stack([used // ((d1 + 1) * (d2 + 1)), used // (d2 + 1) % (d1 + 1), used % (d2 + 1)], axis=1)
    return verts.astype(np.int32).reshape(-1, 3), np.searchsorted(used, lat).astype(np.int32).reshape(-1, 4)


def used_by_cells(occ):
    """The 8-cell rule: bool [d0 + 1, d1 + 1, d2 + 1], a lattice point is used iff its 8 surrounding cells (outside = empty) are
    neither all filled nor all empty."""
    pad = np.pad(np.asarray(occ).astype(np.int32), 1)
    n = sum(pad[a:pad.shape[0] - 1 + a, b:pad.shape[1] - 1 + b, c:pad.shape[2] - 1 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1))
    return (n > 0) & (n < 8)


def canonical_faces(corners):
    """[m, 4, 3] corner points -> the same face SET as an array: corners sorted inside a face, faces sorted"""
    c = np.asarray(corners, dtype=np.int64).reshape(-1, 4, 3)
    key = (c[..., 0] * 1000 + c[..., 1]) * 1000 + c[..., 2]
    c = np.take_along_axis(c, np.argsort(key, axis=1)[..., None], axis=1)
    flat = c.reshape(len(c), 12)
    return flat[np.lexsort(flat.T[::-1])].reshape(-1, 4, 3).astype(np.int16)


def revoxelise(verts, faces, dims):
    """The volume a closed voxel surface encloses, from its +-z faces alone: a voxel (x, y, z) is inside iff an odd number of
    z-normal faces of its column (x, y) lie at heights <= z."""
    d0, d1, d2 = dims
    cross = np.zeros((d0, d1, d2 + 1), np.int64)
    q = np.asarray(verts)[np.asarray(faces)].reshape(-1, 4, 3)
    flat = q[(q[..., 2] == q[:, :1, 2]).all(axis=1)]                                        # the faces of constant z
    np.add.at(cross, (flat[..., 0].min(axis=1), flat[..., 1].min(axis=1), flat[:, 0, 2]), 1)
    return (np.cumsum(cross, axis=2)[..., :d2] % 2).astype(bool)
