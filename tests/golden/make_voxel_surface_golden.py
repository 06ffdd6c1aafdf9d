#!/usr/bin/env python3
"""Golden vectors for the exposed-voxel-face mesh: the face set matplotlib's Axes3D.voxels(volume) builds, which is the call the
reference's get_volume_views (utils/helpers.py:50-88) makes on `volume >= 0.5` and what core/test.py:178-187 renders.  voxels()
makes one Poly3DCollection per filled voxel from that voxel's exposed quads; the corner points it hands to the collections are
recorded here through a subclass, so nothing is drawn and no private attribute is read.  The fixture stores, per case, the dims,
the bit-packed volume and the faces as [m, 4, 3] integer corner points in canonical order (corners sorted inside a face, faces
sorted: a face SET - matplotlib's own face and corner order is a drawing detail).

Needs matplotlib (3.10.8 wrote the committed file); the tests read only the .npz.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_voxel_surface_golden.py"""
import os
import sys

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
from mpl_toolkits.mplot3d import art3d  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
from voxel_surface_ref import canonical_faces, surface  # noqa: E402

RECORDED = []


class RecordingCollection(art3d.Poly3DCollection):
    def __init__(self, verts, *args, **kwargs):
        RECORDED.extend(np.asarray(v) for v in verts)
        super().__init__(verts, *args, **kwargs)


def matplotlib_faces(volume):
    """[m, 4, 3] corner points of every quad Axes3D.voxels(volume) creates"""
    del RECORDED[:]
    fig = plt.figure()
    ax = fig.add_subplot(projection="3d")
    original = art3d.Poly3DCollection
    art3d.Poly3DCollection = RecordingCollection
    try:
        polygons = ax.voxels(volume)
    finally:
        art3d.Poly3DCollection = original
        plt.close(fig)
    assert set(map(tuple, np.argwhere(volume))) >= set(tuple(int(c) for c in k) for k in polygons)
    quads = np.asarray(RECORDED, dtype=np.float64).reshape(-1, 4, 3)
    assert np.array_equal(quads, np.round(quads)), "voxels() without x, y, z puts corners on the integer lattice"
    return quads.astype(np.int64)


rng = np.random.default_rng(20261021)
cases = {
    "one": np.ones((1, 1, 1), bool),
    "rand2x3x4": rng.random((2, 3, 4)) < 0.5,
    "rand5x4x3": rng.random((5, 4, 3)) < 0.4,
    "rand7x2x5": rng.random((7, 2, 5)) < 0.6,
    "rand8": rng.random((8, 8, 8)) < 0.3,
    "full4": np.ones((4, 4, 4), bool),
    "dense6": rng.random((6, 6, 6)) < 0.7,
    "empty3": np.zeros((3, 3, 3), bool),
}

out = {}
for name, vol in cases.items():
    faces = canonical_faces(matplotlib_faces(vol))
    verts, quads = surface(vol)
    same = np.array_equal(canonical_faces(verts[quads]), faces)
    print(f"{name:10s} dims {vol.shape}  filled {int(vol.sum()):4d}  matplotlib faces {len(faces):4d}  restatement agrees: {same}")
    out[name + "_dims"] = np.asarray(vol.shape, np.int32)
    out[name + "_occ"] = np.packbits(vol.reshape(-1))
    out[name + "_faces"] = faces
np.savez_compressed(os.path.join(HERE, "voxel_surface_cases.npz"), **out)
print("wrote", os.path.join(HERE, "voxel_surface_cases.npz"))
