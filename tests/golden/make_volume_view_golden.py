#!/usr/bin/env python3
"""Golden pictures for the volume views: the REFERENCE's own get_volume_views (utils/helpers.py:50-88), imported from the reference tree
and run as written.  helpers.py imports torchvision, which is not installed: a stand-in module that holds nothing covers the import
(the function does not use it).  The function calls matplotlib.pyplot.savefig before it closes its figure; a wrapper round savefig
records, for the current axes, get_proj() and transData.get_matrix() - the camera the picture was drawn with.  The colours matplotlib
shades the faces with are recorded per face normal through a subclass of Poly3DCollection (PolyCollection.get_facecolor() right after
construction: the shaded colours in face order, before any depth sort), as make_voxel_surface_golden.py records the corner points.

Per case the fixture stores the bit-packed volume, the returned [3, H, W] picture cropped to the bounding rectangle of its drawn pixels
(picture != plate) with the rectangle's offset, and the two matrices; once per distinct dims the picture of the all-empty volume (the
plate: panes, grid, ticks); once the shaded colours as uint8.  Pictures are stored [h, w, 3] (interleaved channels deflate to two thirds
of the planar size).  Only data.  The 32^3 checkerboard is not a case: its picture alone deflates to 113 KB, which would put the file
above the largest fixture committed before it; tests/test_cpu_volume_view.py says how its silhouette was checked once.

Needs matplotlib (3.10.8 wrote the committed file); the tests read only the .npz.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_volume_view_golden.py"""
import importlib.util
import os
import sys
import tempfile
import types

import matplotlib

matplotlib.use("Agg")
import matplotlib.pyplot as plt  # noqa: E402
import numpy as np  # noqa: E402
from matplotlib.collections import PolyCollection  # noqa: E402
from mpl_toolkits.mplot3d import art3d  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
from volume_view_ref import FACE_NAMES, render_ids, uniform3x3, view_camera  # noqa: E402

if "torchvision" not in sys.modules:
    try:
        import torchvision  # noqa: F401
    except ImportError:
        tv = types.ModuleType("torchvision")
        tv.transforms = types.ModuleType("torchvision.transforms")
        sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, tv.transforms
spec = importlib.util.spec_from_file_location("ref_helpers", os.path.join(os.environ.get("SWINVOX_REFERENCE", "/root/reference"), "utils", "helpers.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

SEEN = {}
NORMALS = {(-1, 0, 0): 0, (1, 0, 0): 1, (0, -1, 0): 2, (0, 1, 0): 3, (0, 0, -1): 4, (0, 0, 1): 5}
COLOURS = {}


class RecordingCollection(art3d.Poly3DCollection):
    def __init__(self, verts, *args, **kwargs):
        super().__init__(verts, *args, **kwargs)
        for quad, rgba in zip(verts, PolyCollection.get_facecolor(self)):
            q = np.asarray(quad, np.float64)
            n = np.cross(q[1] - q[0], q[2] - q[1])
            COLOURS.setdefault(NORMALS[tuple(int(c) for c in np.sign(np.round(n)))], set()).add(tuple(float(c) for c in rgba[:3]))


_savefig = plt.savefig


def recording_savefig(*args, **kwargs):
    ax = plt.gca()
    SEEN["proj"] = np.array(ax.get_proj(), np.float64)
    SEEN["trans"] = np.array(ax.transData.get_matrix(), np.float64)
    return _savefig(*args, **kwargs)


def reference_picture(vol):
    original = art3d.Poly3DCollection
    art3d.Poly3DCollection = RecordingCollection
    plt.savefig = recording_savefig
    try:
        with tempfile.TemporaryDirectory() as tmp:
            img = ref.get_volume_views(vol.astype(np.float32), tmp, "GV", 0, 0)
    finally:
        art3d.Poly3DCollection = original
        plt.savefig = _savefig
    return np.array(img, np.uint8), SEEN["proj"].copy(), SEEN["trans"].copy()


rng = np.random.default_rng(20261021)
x, y, z = np.indices((32, 32, 32))
boxes = np.zeros((32, 32, 32), bool)
boxes[4:14, 6:20, 3:12] = True
boxes[16:28, 10:18, 8:26] = True
boxes |= rng.random((32, 32, 32)) < 0.01
cases = {
    "boxes": boxes,
    "sphere": (x - 15.5) ** 2 + (y - 15.5) ** 2 + (z - 15.5) ** 2 <= 13.0 ** 2,
    "rand31x33x32": rng.random((31, 33, 32)) < 0.05,
}

out, plates = {}, {}
for name, vol in cases.items():
    dims = tuple(vol.shape)
    if dims not in plates:
        plates[dims], _, _ = reference_picture(np.zeros(dims, bool))
        out["plate_%dx%dx%d" % dims] = np.ascontiguousarray(plates[dims].transpose(1, 2, 0))
    img, proj, trans = reference_picture(vol)
    assert img.shape == (3, 480, 640)
    drawn = (img != plates[dims]).any(axis=0)
    rows, cols = np.flatnonzero(drawn.any(axis=1)), np.flatnonzero(drawn.any(axis=0))
    r0, r1, c0, c1 = rows[0], rows[-1] + 1, cols[0], cols[-1] + 1
    out[name + "_dims"] = np.asarray(dims, np.int32)
    out[name + "_occ"] = np.packbits(vol.reshape(-1))
    out[name + "_image"] = np.ascontiguousarray(img[:, r0:r1, c0:c1].transpose(1, 2, 0))
    out[name + "_offset"] = np.asarray([r0, c0], np.int32)
    out[name + "_proj"], out[name + "_trans"] = proj, trans
    ids = render_ids(vol, view_camera(dims), (480, 640))
    print(f"{name:13s} dims {dims}  filled {int(vol.sum()):6d}  drawn {int(drawn.sum()):6d}  hit {int((ids >= 0).sum()):6d}  crop {r1 - r0} x {c1 - c0}")
assert sorted(COLOURS) == list(range(6)) and all(len(v) == 1 for v in COLOURS.values()), COLOURS
table = np.asarray([[int(c * 255 + 0.5) for c in next(iter(COLOURS[n]))] for n in range(6)], np.uint8)   # Agg's rounding of a float colour
out["face_rgb"] = table
# the table is what the pictures show: the commonest colour among the face-interior pixels of each visible normal
ids = render_ids(cases["sphere"], view_camera((32, 32, 32)), (480, 640))
full = np.array(plates[(32, 32, 32)])
r0, c0 = out["sphere_offset"]
crop = out["sphere_image"].transpose(2, 0, 1)
full[:, r0:r0 + crop.shape[1], c0:c0 + crop.shape[2]] = crop
for face in (1, 3, 5):
    m = uniform3x3(ids) & (ids >= 0) & (ids % 6 == face)
    px, n = np.unique(full[:, m].T, axis=0, return_counts=True)
    print(FACE_NAMES[face], "table", table[face].tolist(), "commonest in the picture", px[np.argmax(n)].tolist())
    assert px[np.argmax(n)].tolist() == table[face].tolist()
path = os.path.join(HERE, "volume_view_cases.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
