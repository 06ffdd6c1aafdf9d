"""Input preparation on the device: counterparts of utils/data_loaders.py:52-88 (get_datum),
utils/binvox_rw.py:105-149 and utils/data_transforms.py as composed at core/train.py:44-65.

The reference expands every sample on the CPU inside DataLoader workers (np.repeat for the voxels; cv2.resize and five numpy
passes per rendering).  Here the workers only read bytes: run-length pairs and 8-bit renderings go to the GPU as they are and
two entry points expand a whole batch - sv_binvox_decode and sv_augment_views.  Random augmentation parameters are drawn on
the host in the reference's call order (draw_train_params), so a seeded run sees the same crops / colours / flips.
Renderings pasted over photographs (RandomBackground with a folder, utils/data_transforms.py:415-452): augment_views(..., backgrounds=
background_bank(...)) -> sv_augment_views_bg, the photograph and the per-view choice drawn by draw_train_params(n_backgrounds=N).
Photographs with bounding boxes (the Pascal3D / Pix3D loaders, utils/data_loaders.py:176-203, :311-338) go through augment_images:
images of differing sizes in one packed buffer, the reference's crop integers computed on the host (bbox_crop_rect), one launch pair.
Ground truth from model files (utils/binvox_converter.py, which shells out to the external binvox program): parse_mesh reads OFF / OBJ / PLY,
voxelise_mesh_batch -> sv_voxelise_meshes voxelises a ragged batch in exact integer arithmetic, meshes_to_binvox writes the files.
"""
from __future__ import annotations

import ctypes as C
import random
import struct
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .hip import call, ptr

EIGVALS = (0.2175, 0.0188, 0.0045)                                        # utils/data_transforms.py:362-364
EIGVECS = ((-0.5675, 0.7192, 0.4009), (-0.5808, -0.0045, -0.8140), (-0.5836, -0.6948, 0.4203))


# ---- binvox ----------------------------------------------------------------------------------------------------------------
def parse_binvox_header(raw: bytes) -> Tuple[List[int], List[float], float, int]:
    """utils/binvox_rw.py:105-116: returns (dims, translate, scale, offset of the run-length payload)."""
    pos, lines = 0, []
    for _ in range(5):
        end = raw.find(b"\n", pos)
        if end < 0:
            raise IOError("[ERROR] Not a binvox file")
        lines.append(raw[pos:end].strip())
        pos = end + 1
    if not lines[0].startswith(b"#binvox"):
        raise IOError("[ERROR] Not a binvox file")
    dims = list(map(int, lines[1].split(b" ")[1:]))
    translate = list(map(float, lines[2].split(b" ")[1:]))
    scale = list(map(float, lines[3].split(b" ")[1:]))[0]
    return dims, translate, scale, pos


def decode_binvox_batch(files: Sequence[bytes], device, fix_coords: bool = True, check: bool = True) -> torch.Tensor:
    """B binvox files (whole file contents) with equal dims -> float32 occupancy [B, d0, d2, d1] (xyz order; [B, d0, d1, d2]
    with fix_coords=False), i.e. read_as_3d_array(f).data.astype(np.float32) of utils/data_loaders.py:83-86 for a batch.
    check=True synchronises once to verify that every stream describes exactly d0*d1*d2 voxels."""
    if not files:
        raise ValueError("decode_binvox_batch: no files")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("swinvox_amd: tensors must live on the GPU (no CPU path exists in the product)")
    dims0, offs, chunks = None, [0], []
    for raw in files:
        dims, _, _, pos = parse_binvox_header(raw)
        if dims0 is None:
            dims0 = dims
        elif dims != dims0:
            raise ValueError(f"decode_binvox_batch: mixed volume sizes {dims0} and {dims}")
        payload = raw[pos:]
        if len(payload) % 2:
            raise ValueError("decode_binvox_batch: odd run-length payload")
        chunks.append(payload)
        offs.append(offs[-1] + len(payload) // 2)
    rle = torch.frombuffer(bytearray(b"".join(chunks)) or bytearray(2), dtype=torch.uint8).to(dev)
    off = torch.tensor(offs, dtype=torch.int64).to(dev)
    B, (d0, d1, d2) = len(files), dims0
    out = torch.zeros((B, d0, d2, d1) if fix_coords else (B, d0, d1, d2), dtype=torch.float32, device=dev)
    decoded = torch.empty(B, dtype=torch.int32, device=dev)
    call("sv_binvox_decode", ptr(rle), ptr(off), B, d0, d1, d2, 1 if fix_coords else 0, ptr(out), ptr(decoded))
    if check:
        bad = (decoded != d0 * d1 * d2).nonzero().flatten().tolist()
        if bad:
            raise ValueError(f"decode_binvox_batch: run lengths of volume(s) {bad} do not add up to {d0 * d1 * d2} voxels")
    return out


def binvox_header(dims, translate=(0.0, 0.0, 0.0), scale=1.0) -> bytes:
    """The five header lines utils/binvox_rw.py:254-262 writes, formatted the same way (str() of every number)."""
    return ("#binvox 1\ndim %s\ntranslate %s\nscale %s\ndata\n"
            % (" ".join(map(str, dims)), " ".join(map(str, translate)), str(scale))).encode("latin-1")


def _per_volume(value, B: int, is_single, what: str, who: str = "encode_binvox_batch") -> list:
    if is_single(value):
        return [value] * B
    value = list(value)
    if len(value) != B:
        raise ValueError(f"{who}: {what} must be one value or one per volume ({B}), got {len(value)}")
    return value


def encode_binvox_batch(volumes: torch.Tensor, threshold: Optional[float] = None, translate=(0.0, 0.0, 0.0), scale=1.0,
                        fix_coords: bool = True) -> List[bytes]:
    """[B, a, b, c] on the GPU -> B binvox files (whole file contents), the bytes utils/binvox_rw.py:239-292 (write) produces,
    zero-count pairs included (see sv_binvox_encode in the header).  float32 / uint8 / bool volumes are occupancy (set iff != 0);
    with `threshold` in (0, 1) the volumes are float32 logits and a voxel is set iff sigmoid(x) >= threshold, the predicate of
    voxel_metrics.  The header dims are (a, c, b) with fix_coords (xyz input, as decode_binvox_batch returns it), (a, b, c)
    without, so decode_binvox_batch(encode_binvox_batch(v)) == v.  translate (three numbers) and scale (a number) may also be
    given per volume.  One kernel launch and two device-to-host copies whatever B is: the pair counts, then the payload
    trimmed to the longest stream."""
    hip.check_cuda(volumes)
    if volumes.dim() != 4 or volumes.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise RuntimeError("encode_binvox_batch expects float32, uint8 or bool [B, a, b, c]")
    if threshold is not None and (not 0.0 < float(threshold) < 1.0 or volumes.dtype != torch.float32):
        raise ValueError("encode_binvox_batch: threshold must lie in (0, 1) and needs float32 logits")
    B, a, b, c = volumes.shape
    if B == 0:
        raise ValueError("encode_binvox_batch: no volumes")
    d0, d1, d2 = (a, c, b) if fix_coords else (a, b, c)
    trs = _per_volume(translate, B, lambda t: not hasattr(t[0], "__len__"), "translate")
    scs = _per_volume(scale, B, lambda s: not hasattr(s, "__len__"), "scale")
    vol = volumes.contiguous()
    if vol.dtype == torch.bool:
        vol = vol.view(torch.uint8)
    total = d0 * d1 * d2
    pairs = torch.empty(B, total, 2, dtype=torch.uint8, device=vol.device)
    n_pairs = torch.empty(B, dtype=torch.int32, device=vol.device)
    call("sv_binvox_encode", ptr(vol), 0 if vol.dtype == torch.float32 else 1, B, d0, d1, d2, 1 if fix_coords else 0,
         -1.0 if threshold is None else float(threshold), ptr(pairs), total, ptr(n_pairs))
    counts = n_pairs.tolist()
    payload = pairs[:, :max(counts)].cpu().numpy()
    return [binvox_header((d0, d1, d2), trs[i], scs[i]) + payload[i, :counts[i]].tobytes() for i in range(B)]


# ---- exposed voxel faces ---------------------------------------------------------------------------------------------------
SURFACE_MAX_DIM = 64                                                       # sv_voxel_surface keeps a volume's bit masks in LDS


def extract_surface_batch(volumes: torch.Tensor, threshold: Optional[float] = None) -> List[Tuple[np.ndarray, np.ndarray]]:
    """[B, a, b, c] on the GPU -> per volume (verts int32 [n, 3], faces int32 [m, 4]) on the host: the quads that separate a set
    voxel from an unset one or from the outside, the face set utils/helpers.py:50-88 hands to Axes3D.voxels (core/test.py:178-187).
    Axes are the array's own (no fix_coords transposition); vertices are lattice points (i, j, k) in ascending lattice order, faces
    follow ascending voxel index and then the directions -x +x -y +y -z +z, corners counter-clockwise seen from outside (see
    sv_voxel_surface in the header).  float32 / uint8 / bool volumes are occupancy (set iff != 0); with `threshold` in (0, 1) the
    volumes are float32 logits and a voxel is set iff sigmoid(x) >= threshold, the predicate of voxel_metrics and
    encode_binvox_batch.  One kernel launch and two device-to-host copies whatever B is: the counts, then both payloads trimmed
    to the longest in the batch."""
    hip.check_cuda(volumes)
    if volumes.dim() != 4 or volumes.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise RuntimeError("extract_surface_batch expects float32, uint8 or bool [B, a, b, c]")
    if threshold is not None and (not 0.0 < float(threshold) < 1.0 or volumes.dtype != torch.float32):
        raise ValueError("extract_surface_batch: threshold must lie in (0, 1) and needs float32 logits")
    B, d0, d1, d2 = volumes.shape
    if B == 0:
        raise ValueError("extract_surface_batch: no volumes")
    if min(d0, d1, d2) < 1 or max(d0, d1, d2) > SURFACE_MAX_DIM:
        raise ValueError(f"extract_surface_batch: dims {(d0, d1, d2)}, every dim must lie in 1 .. {SURFACE_MAX_DIM}")
    vol = volumes.contiguous()
    if vol.dtype == torch.bool:
        vol = vol.view(torch.uint8)
    vcap = (d0 + 1) * (d1 + 1) * (d2 + 1)
    fcap = 3 * d0 * d1 * d2 + d0 * d1 + d1 * d2 + d0 * d2
    verts = torch.empty(B, vcap, dtype=torch.int32, device=vol.device)
    faces = torch.empty(B, fcap, 4, dtype=torch.int32, device=vol.device)
    counts = torch.empty(B, 2, dtype=torch.int32, device=vol.device)
    call("sv_voxel_surface", ptr(vol), 0 if vol.dtype == torch.float32 else 1, B, d0, d1, d2,
         -1.0 if threshold is None else float(threshold), ptr(verts), vcap, ptr(faces), fcap, ptr(counts))
    cnt = counts.tolist()
    nv, nf = max(c[0] for c in cnt), max(c[1] for c in cnt)
    both = torch.cat([verts[:, :nv], faces[:, :nf].reshape(B, 4 * nf)], dim=1).cpu().numpy()
    out = []
    for i, (n, m) in enumerate(cnt):
        lat = both[i, :n]
        ijk = np.stack([lat // ((d1 + 1) * (d2 + 1)), lat // (d2 + 1) % (d1 + 1), lat % (d2 + 1)], axis=1).astype(np.int32)
        out.append((ijk, both[i, nv:nv + 4 * m].reshape(m, 4).copy()))
    return out


_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\ncomment swinvox_amd exposed voxel faces\nelement vertex %d\n"
               "property float x\nproperty float y\nproperty float z\nelement face %d\nproperty list uchar int vertex_indices\nend_header\n")


def mesh_file(verts, faces, fmt: str = "ply", dims=None, translate=(0.0, 0.0, 0.0), scale=None) -> bytes:
    """A quad mesh (verts [n, 3] lattice points, faces [m, 4] indices into them) as the contents of a .ply (binary little endian),
    .off or .obj file; pure host code.  Coordinates are lattice units when `scale` is None, otherwise
    translate + scale * idx / max(dims) in float64 - the binvox header convention: voxel corner idx of a model normalised to its
    largest dimension.  An empty mesh is a valid file in every format."""
    verts = np.asarray(verts).reshape(-1, 3)
    faces = np.asarray(faces).reshape(-1, 4).astype(np.int64)
    n, m = len(verts), len(faces)
    if m and (faces.min() < 0 or faces.max() >= n):
        raise ValueError("mesh_file: a face index lies outside the vertex list")
    if scale is None:
        if any(float(t) != 0.0 for t in translate):
            raise ValueError("mesh_file: translate needs a scale (coordinates are lattice units without one)")
        xyz = verts.astype(np.float64)
    else:
        if dims is None:
            raise ValueError("mesh_file: scale needs the volume's dims")
        xyz = np.asarray(translate, np.float64)[None, :] + float(scale) * verts.astype(np.float64) / float(max(dims))
    if fmt == "ply":
        rec = np.empty(m, dtype=np.dtype([("n", "u1"), ("v", "<i4", (4,))]))
        rec["n"], rec["v"] = 4, faces
        return (_PLY_HEADER % (n, m)).encode("ascii") + xyz.astype("<f4").tobytes() + rec.tobytes()
    if fmt == "off":
        lines = ["OFF", "%d %d 0" % (n, m)]
        lines += ["%.9g %.9g %.9g" % tuple(p) for p in xyz.tolist()]
        lines += ["4 %d %d %d %d" % tuple(f) for f in faces.tolist()]
    elif fmt == "obj":
        lines = ["v %.9g %.9g %.9g" % tuple(p) for p in xyz.tolist()]
        lines += ["f %d %d %d %d" % tuple(f) for f in (faces + 1).tolist()]
    else:
        raise ValueError(f"mesh_file: format {fmt!r} is none of 'ply', 'off', 'obj'")
    return ("\n".join(lines) + "\n").encode("ascii") if lines else b""


def encode_mesh_batch(volumes: torch.Tensor, threshold: Optional[float] = None, fmt: str = "ply", translate=(0.0, 0.0, 0.0),
                      scale=None) -> List[bytes]:
    """[B, a, b, c] on the GPU -> B mesh files (extract_surface_batch + mesh_file with dims = (a, b, c)).  translate (three
    numbers) and scale (a number or None) may also be given per volume."""
    if fmt not in ("ply", "off", "obj"):
        raise ValueError(f"encode_mesh_batch: format {fmt!r} is none of 'ply', 'off', 'obj'")
    meshes = extract_surface_batch(volumes, threshold)
    B, dims = len(meshes), tuple(volumes.shape[1:])
    trs = _per_volume(translate, B, lambda t: not hasattr(t[0], "__len__"), "translate", "encode_mesh_batch")
    scs = _per_volume(scale, B, lambda s: not hasattr(s, "__len__"), "scale", "encode_mesh_batch")
    return [mesh_file(v, f, fmt, dims, trs[i], scs[i]) for i, (v, f) in enumerate(meshes)]


# ---- mesh voxelisation -----------------------------------------------------------------------------------------------------
VOXEL_UNITS = 1024                                                         # S of sv_voxelise_meshes: snapped units per voxel
_VOXELISE_MODES = {"solid": 0, "surface": 1, "both": 2}                    # SV_VOXELISE_*
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2", "int": "i4",
              "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _fan(polys) -> np.ndarray:
    """polygons (index lists, or an [m, k] array) -> int64 [t, 3]: polygon (p0 .. pk-1) becomes (p0, pi, pi+1), i = 1 .. k - 2, in order"""
    if isinstance(polys, np.ndarray):
        if polys.size == 0:
            return np.zeros((0, 3), np.int64)
        if polys.ndim != 2 or polys.shape[1] < 3:
            raise ValueError(f"faces are [m, k] with k >= 3 corners, got {list(polys.shape)}")
        f = polys.astype(np.int64)
        return np.stack([np.stack([f[:, 0], f[:, i], f[:, i + 1]], axis=1) for i in range(1, f.shape[1] - 1)], axis=1).reshape(-1, 3)
    tris = [(p[0], p[i], p[i + 1]) for p in polys for i in range(1, len(p) - 1)]
    return np.asarray(tris, np.int64).reshape(-1, 3)


def _parse_off(text: str):
    lines = [ln.split("#", 1)[0].split() for ln in text.splitlines()]
    lines = [ln for ln in lines if ln]
    head = lines[0]
    if head[0] not in ("OFF", "COFF"):
        raise ValueError(f"parse_mesh: an OFF file starts with OFF or COFF, got {head[0]!r}")
    if len(head) >= 3:                                                     # "OFF n m e" on one line
        counts, row = head[1:], 1
    else:
        counts, row = lines[1], 2
    n, m = int(counts[0]), int(counts[1])
    if len(lines) < row + n + m:
        raise ValueError(f"parse_mesh: the OFF header promises {n} vertices and {m} faces, the file holds {len(lines) - row} lines")
    verts = np.asarray([[float(x) for x in ln[:3]] for ln in lines[row:row + n]], np.float64).reshape(-1, 3)
    polys = []
    for ln in lines[row + n:row + n + m]:
        k = int(ln[0])
        if k < 3 or len(ln) < 1 + k:
            raise ValueError(f"parse_mesh: OFF face {' '.join(ln)!r} has fewer than 3 corners or misses indices")
        polys.append([int(x) for x in ln[1:1 + k]])                        # colours after the indices are ignored
    return verts, _fan(polys)


def _parse_obj(text: str):
    verts, polys = [], []
    for ln in text.splitlines():
        tok = ln.split("#", 1)[0].split()
        if not tok:
            continue
        if tok[0] == "v":
            verts.append([float(x) for x in tok[1:4]])
        elif tok[0] == "f":
            idx = [int(t.split("/")[0]) for t in tok[1:]]                  # i, i/t, i/t/n, i//n
            if len(idx) < 3 or 0 in idx:
                raise ValueError(f"parse_mesh: OBJ face {ln.strip()!r} has fewer than 3 corners or an index 0")
            polys.append([i - 1 if i > 0 else len(verts) + i for i in idx])   # negative: counted back from the vertices read so far
    return np.asarray(verts, np.float64).reshape(-1, 3), _fan(polys)


def _parse_ply(raw: bytes):
    end = raw.find(b"end_header")
    nl = raw.find(b"\n", end)
    if end < 0 or nl < 0:
        raise ValueError("parse_mesh: a PLY file without end_header")
    fmt, elements = None, []                                               # elements: [name, count, [(kind, ...), ...]]
    for ln in raw[:end].decode("latin-1").splitlines()[1:]:
        tok = ln.split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "format":
            fmt = tok[1]
        elif tok[0] == "element":
            elements.append([tok[1], int(tok[2]), []])
        elif tok[0] == "property":
            if tok[1] == "list":
                elements[-1][2].append(("list", _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]], tok[4]))
            else:
                elements[-1][2].append(("scalar", _PLY_TYPES[tok[1]], tok[2]))
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"parse_mesh: PLY format {fmt!r} is neither ascii nor binary_little_endian")
    body, pos = raw[nl + 1:], 0
    words = body.split() if fmt == "ascii" else None
    verts, polys = np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)
    for name, count, props in elements:
        if name not in ("vertex", "face"):
            if fmt == "ascii" or any(p[0] == "list" for p in props):
                raise ValueError(f"parse_mesh: PLY element {name!r} is not supported")
            pos += count * sum(np.dtype(p[1]).itemsize for p in props)
            continue
        if name == "vertex":
            if any(p[0] == "list" for p in props) or not {"x", "y", "z"} <= {p[2] for p in props}:
                raise ValueError("parse_mesh: PLY vertices need scalar properties x, y, z")
            if fmt == "ascii":
                tab = np.asarray(words[pos:pos + count * len(props)], np.float64).reshape(count, len(props))
                pos += count * len(props)
                col = {p[2]: i for i, p in enumerate(props)}
                verts = np.stack([tab[:, col[c]] for c in "xyz"], axis=1).reshape(-1, 3)
            else:
                dt = np.dtype([(p[2], "<" + p[1]) for p in props])
                tab = np.frombuffer(body, dt, count, pos)
                pos += count * dt.itemsize
                verts = np.stack([tab[c].astype(np.float64) for c in "xyz"], axis=1).reshape(-1, 3)
        else:
            if len(props) != 1 or props[0][0] != "list":
                raise ValueError("parse_mesh: PLY faces need exactly one list property (vertex_indices)")
            _, ct, it, _ = props[0]
            faces = []
            if fmt == "ascii":
                for _ in range(count):
                    k = int(words[pos])
                    faces.append([int(w) for w in words[pos + 1:pos + 1 + k]])
                    pos += 1 + k
            elif count:
                k0 = int(np.frombuffer(body, "<" + ct, 1, pos)[0])
                dt = np.dtype([("n", "<" + ct), ("v", "<" + it, (k0, ))])
                if len(body) - pos >= count * dt.itemsize and (np.frombuffer(body, dt, count, pos)["n"] == k0).all():   # every face alike
                    faces = np.frombuffer(body, dt, count, pos)["v"].astype(np.int64).reshape(count, k0)
                    pos += count * dt.itemsize
                else:
                    cs, isz = np.dtype(ct).itemsize, np.dtype(it).itemsize
                    for _ in range(count):
                        k = int(np.frombuffer(body, "<" + ct, 1, pos)[0])
                        faces.append(np.frombuffer(body, "<" + it, k, pos + cs).astype(np.int64).tolist())
                        pos += cs + k * isz
            if not isinstance(faces, np.ndarray) and any(len(f) < 3 for f in faces):
                raise ValueError("parse_mesh: a PLY face has fewer than 3 corners")
            polys = _fan(faces)
    return verts, polys


def parse_mesh(raw: bytes) -> Tuple[np.ndarray, np.ndarray]:
    """The contents of an OFF, OBJ or PLY file -> (verts float64 [n, 3], tris int64 [m, 3]); pure host code.  OFF: `COFF`, comment lines and
    colours behind the indices are tolerated; OBJ: `v` and `f` lines, corners written i, i/t, i/t/n or i//n, negative indices counted back
    from the vertices read so far, every other line ignored; PLY: ASCII, and binary little endian as mesh_file writes it (scalar vertex
    properties with x, y, z among them, one list property per face).  Polygons are fan-triangulated: (p0 .. pk-1) gives (p0, pi, pi+1) for
    i = 1 .. k - 2, so parse_mesh(mesh_file(v, f, fmt)) returns the lattice vertices and each quad as its two triangles.  An index outside
    the vertex list is a ValueError."""
    raw = bytes(raw)
    if raw[:3] == b"ply":
        verts, tris = _parse_ply(raw)
    else:
        text = raw.decode("latin-1")
        first = next((ln.split("#", 1)[0].split() for ln in text.splitlines() if ln.split("#", 1)[0].split()), None)
        if first is None:
            return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int64)       # mesh_file's empty OBJ
        verts, tris = _parse_off(text) if first[0] in ("OFF", "COFF") else _parse_obj(text)
    if len(tris) and (tris.min() < 0 or tris.max() >= len(verts)):
        raise ValueError(f"parse_mesh: a face names vertex {int(tris.min() if tris.min() < 0 else tris.max())} of {len(verts)}")
    return verts, tris


def _dims3(dims, who: str) -> Tuple[int, int, int]:
    d = (int(dims), ) * 3 if np.ndim(dims) == 0 else tuple(int(x) for x in dims)
    if len(d) != 3 or min(d) < 1 or max(d) > SURFACE_MAX_DIM:
        raise ValueError(f"{who}: dims {d}, three numbers in 1 .. {SURFACE_MAX_DIM}")
    return d


def mesh_grid_fit(verts, dims, margin: float = 0.0) -> Tuple[List[float], float]:
    """(translate, scale) of the .binvox header convention, grid coordinate = (p - translate) * max(dims) / scale, that maps the longest
    side of the vertices' bounding box onto the grid and centres the box in it - the documented meaning of `binvox -cb`.  For dims that are
    not a cube the side that fills its axis first decides.  margin: the fraction of every axis left free on each side (0 <= margin < 0.5).
    A bounding box without extent (one point) keeps one model unit per voxel."""
    d = np.asarray(_dims3(dims, "mesh_grid_fit"), np.float64)
    v = np.asarray(verts, np.float64).reshape(-1, 3)
    if not len(v) or not np.isfinite(v).all():
        raise ValueError("mesh_grid_fit: needs at least one vertex, and finite ones")
    if not 0.0 <= margin < 0.5:
        raise ValueError(f"mesh_grid_fit: margin {margin} must lie in [0, 0.5)")
    lo, hi = v.min(axis=0), v.max(axis=0)
    side = hi - lo
    per_unit = float(np.min(d[side > 0] * (1.0 - 2.0 * margin) / side[side > 0])) if (side > 0).any() else 1.0   # voxels per model unit
    translate = 0.5 * (lo + hi) - 0.5 * d / per_unit
    return [float(t) for t in translate], float(d.max() / per_unit)


def snap_vertices(grid_verts, dims, who: str = "snap_vertices") -> np.ndarray:
    """Vertices in voxel units (float64 [n, 3]) -> int32 [n, 3] in units of 1 / VOXEL_UNITS voxel: floor(p * VOXEL_UNITS + 0.5) in
    float64.  ValueError for a coordinate that is not finite or lies outside [-d, 2 d] voxels of its axis: sv_voxelise_meshes keeps its
    products inside int64 only for such coordinates."""
    d = np.asarray(_dims3(dims, who), np.float64)
    g = np.asarray(grid_verts, np.float64).reshape(-1, 3)
    if not np.isfinite(g).all():
        raise ValueError(f"{who}: a vertex is not finite")
    s = np.floor(g * VOXEL_UNITS + 0.5)
    bad = np.argwhere((s < -d * VOXEL_UNITS) | (s > 2 * d * VOXEL_UNITS))
    if len(bad):
        n, a = (int(x) for x in bad[0])
        raise ValueError(f"{who}: vertex {n} has coordinate {g[n, a]:.6g} on axis {a}, outside [{-d[a]:g}, {2 * d[a]:g}] voxels (one grid beside a "
                         f"grid of {int(d[a])}): the exact integer arithmetic is sized for that range; fit the mesh to the grid first")
    return s.astype(np.int32)


def _mesh_arrays(mesh, who: str) -> Tuple[np.ndarray, np.ndarray]:
    if isinstance(mesh, (bytes, bytearray, memoryview)):
        return parse_mesh(bytes(mesh))
    if len(mesh) != 2:
        raise ValueError(f"{who}: a mesh is (verts, faces) or the contents of a mesh file")
    verts = np.asarray(mesh[0], np.float64).reshape(-1, 3)
    try:
        tris = _fan(np.asarray(mesh[1]))
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    return verts, tris


def pack_meshes(meshes, dims=32, fit="bbox", transform=None, who: str = "pack_meshes"):
    """Host side of voxelise_mesh_batch: (packed int32 buffer - all snapped vertices, then all triangles -, mesh table int64 [B, 4] of
    sv_voxelise_meshes, total vertices, total triangles, translates, scales).  Nothing here touches the GPU."""
    d = _dims3(dims, who)
    D = float(max(d))
    if not len(meshes):
        raise ValueError(f"{who}: no meshes")
    M = None
    if transform is not None:
        M = np.asarray(transform, np.float64)
        if M.shape not in ((3, 3), (3, 4)) or not np.isfinite(M).all():
            raise ValueError(f"{who}: transform is a finite 3 x 3 or 3 x 4 matrix")
    fits = None
    if fit is not None and not (isinstance(fit, str) and fit == "bbox"):
        fit = list(fit)
        fits = [fit] * len(meshes) if len(fit) == 2 and not hasattr(fit[1], "__len__") else fit
        if len(fits) != len(meshes) or any(len(f) != 2 or len(f[0]) != 3 or not float(f[1]) > 0 for f in fits):
            raise ValueError(f"{who}: fit is 'bbox', None, (translate, scale) or one such pair per mesh, with scale > 0")
    vs, ts, table, translates, scales, nv, nt = [], [], [], [], [], 0, 0
    for i, mesh in enumerate(meshes):
        verts, tris = _mesh_arrays(mesh, who)
        if M is not None:
            verts = verts @ M[:, :3].T + (M[:, 3] if M.shape[1] == 4 else 0.0)
        if fit is None:
            tr, sc = [0.0, 0.0, 0.0], D                                   # vertices are voxel units already
        elif fits is not None:
            tr, sc = [float(x) for x in fits[i][0]], float(fits[i][1])
        elif len(verts):
            tr, sc = mesh_grid_fit(verts, d)
        else:
            tr, sc = [0.0, 0.0, 0.0], 1.0
        snapped = snap_vertices((verts - np.asarray(tr)[None, :]) * D / sc, d, f"{who}: mesh {i}")
        tris = np.where((tris < 0) | (tris > 0x7fffffff), -1, tris).astype(np.int32)   # what int32 cannot hold is out of range anyway
        vs.append(snapped.reshape(-1))
        ts.append(tris.reshape(-1))
        table.append([nv, len(snapped), nt, len(tris)])
        nv, nt = nv + len(snapped), nt + len(tris)
        translates.append(tr)
        scales.append(sc)
    packed = np.concatenate(vs + ts + [np.zeros(1, np.int32)])             # never empty
    return packed, np.asarray(table, np.int64).reshape(-1, 4), nv, nt, translates, scales


def voxelise_mesh_batch(meshes, dims=32, mode: str = "both", fit="bbox", transform=None, dtype=torch.float32, device="cuda"):
    """B triangle meshes -> (volumes [B, d0, d1, d2] on the GPU, translates, scales): what the reference's utils/binvox_converter.py asks
    the external `binvox` program for.  That program was never run next to this code and NO PARITY WITH IT IS CLAIMED; the rule - exact
    integer arithmetic on coordinates snapped to 1 / 1024 voxel - is written out at sv_voxelise_meshes in the header.
    meshes: a sequence of (verts [n, 3], faces [m, k >= 3], polygons fan-triangulated) or of file contents (parse_mesh).
    dims: one number or three, each in 1 .. 64.  mode: "solid" (parity along z: the inside of a closed surface), "surface" (every voxel
    whose closed cube a triangle touches) or "both" (their union, what `binvox -e` is documented to give).
    transform: a 3 x 3 or 3 x 4 matrix applied to the vertices first - the reference's -rotx / -rotz turns and its (2, 0, 1)
    transposition are such permutations of the axes.  fit: "bbox" = mesh_grid_fit per mesh; (translate, scale), or one pair per mesh, =
    the .binvox header convention grid = (p - translate) * max(dims) / scale; None = the vertices are voxel units already (translate 0,
    scale max(dims)).  The volumes are in xyz order, as decode_binvox_batch returns them, so they serve as `gt` directly; translates and
    scales are what the .binvox header of each volume says (meshes_to_binvox).  dtype: float32, uint8 or bool.
    A mesh without triangles gives an empty volume.  A vertex outside [-d, 2 d] voxels after the fit is a ValueError (snap_vertices), and
    so is a face that names a vertex its mesh does not have - counted on the device, never dereferenced.  One host-to-device copy of the
    packed vertices and triangles, one call of the entry, and one device-to-host copy: those counters."""
    if mode not in _VOXELISE_MODES:
        raise ValueError(f"voxelise_mesh_batch: mode {mode!r} is none of 'solid', 'surface', 'both'")
    if dtype not in (torch.float32, torch.uint8, torch.bool):
        raise ValueError("voxelise_mesh_batch: dtype is float32, uint8 or bool")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("swinvox_amd: tensors must live on the GPU (no CPU path exists in the product)")
    d0, d1, d2 = _dims3(dims, "voxelise_mesh_batch")
    packed, table, nv, nt, translates, scales = pack_meshes(meshes, (d0, d1, d2), fit, transform, "voxelise_mesh_batch")
    B = len(table)
    buf = torch.from_numpy(packed).to(dev)
    hip.check_cuda(buf)
    out = torch.empty(B, d0, d1, d2, dtype=torch.float32 if dtype == torch.float32 else torch.uint8, device=buf.device)
    ws = torch.empty(hip.load().sv_voxelise_meshes_workspace_bytes(B, d0, d1, d2), dtype=torch.uint8, device=buf.device)
    table = np.ascontiguousarray(table)
    call("sv_voxelise_meshes", ptr(buf), nv, ptr(buf) + 12 * nv, nt, table.ctypes.data, B, d0, d1, d2, _VOXELISE_MODES[mode],
         0 if dtype == torch.float32 else 1, ptr(out), ptr(ws))
    bad = ws[32 * B:36 * B].view(torch.int32).tolist()
    if any(bad):
        raise ValueError("voxelise_mesh_batch: " + ", ".join(f"mesh {i}: {n} face(s)" for i, n in enumerate(bad) if n) +
                         " name a vertex outside the mesh's vertex list")
    return (out.view(torch.bool) if dtype == torch.bool else out), translates, scales


def meshes_to_binvox(meshes, dims=32, **kw) -> List[bytes]:
    """B meshes -> B .binvox files (whole file contents), the job of the reference's utils/binvox_converter.py: voxelise_mesh_batch (its
    keywords pass through), then encode_binvox_batch with each mesh's translate and scale in the header, so that
    decode_binvox_batch(meshes_to_binvox(m)) is voxelise_mesh_batch(m)[0]."""
    kw.pop("dtype", None)
    volumes, translates, scales = voxelise_mesh_batch(meshes, dims, dtype=torch.uint8, **kw)
    return encode_binvox_batch(volumes, translate=translates, scale=scales)


# ---- volume views -----------------------------------------------------------------------------------------------------------
# the colours matplotlib shades the faces of Axes3D.voxels with (default light source, default face colour), in the face order
# -x +x -y +y -z +z, as 8-bit RGB; from the camera of get_volume_views +x, +y and +z are the visible ones
VIEW_FACE_RGB = ((27, 105, 159), (13, 50, 75), (27, 105, 159), (13, 50, 75), (17, 63, 96), (24, 91, 138))


def view_camera(dims, elev: float = 30, azim: float = 45, size=(480, 640), proj_type: str = "persp") -> np.ndarray:
    """The camera of the reference's get_volume_views (utils/helpers.py:50-88) for a volume of these dims, as the 18 numbers of
    sv_view_camera, float64 [6, 3] = o0, ox, oy, d0, dx, dy: the ray of pixel (row, col) starts at o0 + (col+0.5) ox + (row+0.5) oy
    and runs along d0 + (col+0.5) dx + (row+0.5) dy in the array's own coordinates, row 0 at the top.  It is what matplotlib's Axes3D
    arrives at in subplot(111) of a figure of size = (H, W) pixels (the default 6.4 x 4.8 in at 100 dpi for (480, 640)) with
    set_box_aspect([1, 1, 1]), limits 0 .. dims, view_init(elev, azim), focal length 1 and distance 10; other sizes scale that figure.
    proj_type "ortho" is the orthographic projection utils/binvox_rw.py:306-343 asks for (rays parallel, dx = dy = 0)."""
    if proj_type not in ("persp", "ortho"):
        raise ValueError(f"view_camera: proj_type {proj_type!r} is neither 'persp' nor 'ortho'")
    H, W = int(size[0]), int(size[1])
    d = np.asarray(dims, np.float64)
    if d.shape != (3,) or (d < 1).any() or H < 1 or W < 1:
        raise ValueError("view_camera: dims are three positive numbers, size is (H, W)")
    dist = 10.0                                                              # Axes3D._dist; the focal length is 1
    aspect = np.ones(3)
    aspect *= 1.8294640721620434 * 25 / 24 * 1 / np.linalg.norm(aspect)       # axes3d.py set_box_aspect
    scale = aspect / d                                                       # proj3d.world_transformation for limits 0 .. dims
    centre = 0.5 * aspect
    er, ar = np.deg2rad(elev), np.deg2rad(azim)
    eye = centre + dist * np.array([np.cos(er) * np.cos(ar), np.cos(er) * np.sin(ar), np.sin(er)])   # get_proj
    flipped = abs(np.deg2rad((elev + 180.0) % 360.0 - 180.0)) > np.pi / 2     # _calc_view_axes: the vertical axis turns over
    w = (eye - centre) / np.linalg.norm(eye - centre)                        # proj3d._view_axes: out of the screen, right, up
    u = np.cross(np.array([0.0, 0.0, -1.0 if flipped else 1.0]), w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    # the axes rectangle: subplot(111) spans 0.125 .. 0.9 by 0.11 .. 0.88 of the figure and apply_aspect shrinks it to a square about
    # its centre; set_top_view maps the view interval (-0.95 / dist, 0.9 / dist) onto it.  Display y runs upwards.
    side = min(0.775 * W, 0.77 * H)
    left, bottom = 0.125 * W + 0.5 * (0.775 * W - side), 0.11 * H + 0.5 * (0.77 * H - side)
    lo, span = -0.95 / dist, (0.9 + 0.95) / dist
    xa, xb = lo - left * span / side, span / side                            # view x = xa + xb (col + 0.5)
    ya, yb = lo + (H - bottom) * span / side, -span / side                   # view y = ya + yb (row + 0.5)
    cam = np.zeros((6, 3))
    if proj_type == "persp":                                                 # _persp_transformation: view x = e.x / -e.z
        cam[0], cam[3], cam[4], cam[5] = eye / scale, (xa * u + ya * v - w) / scale, xb * u / scale, yb * v / scale
    else:                                                                    # _ortho_transformation: view x = e.x / dist
        cam[0], cam[1], cam[2], cam[3] = (eye + dist * (xa * u + ya * v)) / scale, dist * xb * u / scale, dist * yb * v / scale, -w / scale
    return cam


def _rgb_bytes(value, n: int, what: str):
    arr = np.asarray(value)
    if arr.size != n or arr.dtype.kind not in "iu" or arr.min() < 0 or arr.max() > 255:
        raise ValueError(f"render_views_batch: {what} holds {n} integers in 0 .. 255")
    return (C.c_ubyte * n)(*[int(x) for x in arr.reshape(-1)])


def render_views_batch(volumes: torch.Tensor, threshold: Optional[float] = None, cameras=None, size=(480, 640), face_colors=None,
                       edge_color=(0, 0, 0), background=(255, 255, 255), return_ids: bool = False):
    """[B, a, b, c] on the GPU -> uint8 [B, n_cams, 3, H, W] on the GPU: the pictures the reference's evaluation loop draws of its
    reconstructions (utils/helpers.py:50-88 from core/test.py:178-187), for every volume of the batch and every camera, in the layout
    SummaryWriter.add_image takes.  With return_ids also the int32 [B, n_cams, H, W] id buffer (voxel index * 6 + face, -1 background).
    The rule - ray-cast, ids, edge pixels - is written out at sv_render_volumes in the header.  Axes are the array's own, as for
    extract_surface_batch, and so are the dtype and threshold rules: float32 / uint8 / bool volumes are occupancy (set iff != 0); with
    `threshold` in (0, 1) the volumes are float32 logits and a voxel is set iff sigmoid(x) >= threshold.
    cameras: None = the reference's single view, view_camera(dims, size=size); or a sequence of cameras ([6, 3] or 18 numbers each, a
    turntable for instance).  face_colors: six RGB triples for -x +x -y +y -z +z, None = VIEW_FACE_RGB, one table for all cameras.
    background: a colour, or a uint8 [3, H, W] tensor on the GPU (a plate with panes and ticks, say).  Left out: axis panes, grid, ticks
    and labels, anti-aliasing (edge lines are one pixel wide), translucent faces.  One call of the entry, no host synchronisation."""
    hip.check_cuda(volumes)
    if volumes.dim() != 4 or volumes.dtype not in (torch.float32, torch.uint8, torch.bool):
        raise RuntimeError("render_views_batch expects float32, uint8 or bool [B, a, b, c]")
    if threshold is not None and (not 0.0 < float(threshold) < 1.0 or volumes.dtype != torch.float32):
        raise ValueError("render_views_batch: threshold must lie in (0, 1) and needs float32 logits")
    B, d0, d1, d2 = volumes.shape
    if B == 0:
        raise ValueError("render_views_batch: no volumes")
    if min(d0, d1, d2) < 1 or max(d0, d1, d2) > SURFACE_MAX_DIM:
        raise ValueError(f"render_views_batch: dims {(d0, d1, d2)}, every dim must lie in 1 .. {SURFACE_MAX_DIM}")
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1 or H * W > 1 << 24:
        raise ValueError(f"render_views_batch: size {(H, W)}: at least 1 x 1 and at most 2^24 pixels")
    cams = [view_camera((d0, d1, d2), size=(H, W))] if cameras is None else [np.asarray(c, np.float64) for c in cameras]
    if not cams or any(c.size != 18 for c in cams):
        raise ValueError("render_views_batch: cameras is a non-empty sequence of 18 numbers each (o0, ox, oy, d0, dx, dy)")
    cam32 = np.ascontiguousarray(np.stack([c.reshape(18) for c in cams]).astype(np.float32))
    if not np.isfinite(cam32).all():
        raise ValueError("render_views_batch: a camera holds a number that is not finite in float32")
    for n, c in enumerate(cam32):
        if not c[3:9].any() and all(0.0 <= c[a] <= d for a, d in enumerate((d0, d1, d2))):
            raise ValueError(f"render_views_batch: the eye of camera {n} lies inside or on the volume's box")
    face = _rgb_bytes(VIEW_FACE_RGB if face_colors is None else face_colors, 18, "face_colors")
    edge = _rgb_bytes(edge_color, 3, "edge_color")
    plate = None
    if isinstance(background, torch.Tensor):
        hip.check_cuda(background)
        if background.dtype != torch.uint8 or tuple(background.shape) != (3, H, W):
            raise ValueError(f"render_views_batch: a background plate is uint8 [3, {H}, {W}]")
        plate, bg = background.contiguous(), _rgb_bytes((0, 0, 0), 3, "background")
    else:
        bg = _rgb_bytes(background, 3, "background")
    vol = volumes.contiguous()
    if vol.dtype == torch.bool:
        vol = vol.view(torch.uint8)
    dev, n_cams = vol.device, len(cams)
    cam_arr = (hip.ViewCamera * n_cams).from_buffer_copy(cam32.tobytes())
    cam_ws = torch.empty(n_cams * C.sizeof(hip.ViewCamera), dtype=torch.uint8, device=dev)
    mask_ws = torch.empty(B * d0 * d1 * (1 if d2 <= 32 else 2), dtype=torch.int32, device=dev)
    ids = torch.empty(B, n_cams, H, W, dtype=torch.int32, device=dev)
    rgb = torch.empty(B, n_cams, 3, H, W, dtype=torch.uint8, device=dev)
    call("sv_render_volumes", ptr(vol), 0 if vol.dtype == torch.float32 else 1, B, d0, d1, d2, -1.0 if threshold is None else float(threshold),
         C.addressof(cam_arr), n_cams, ptr(cam_ws), H, W, C.addressof(face), C.addressof(edge), C.addressof(bg), ptr(plate), ptr(mask_ws),
         ptr(ids), ptr(rgb))
    return (rgb, ids) if return_ids else rgb


def _png_chunk(kind: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def image_file(img, fmt: str = "png") -> bytes:
    """A uint8 [3, H, W] picture (an array, or a tensor on any device) as the contents of a .png (8-bit RGB, no interlace, every scanline
    with filter 0) or a binary .ppm (P6) file; pure host code, standard library only."""
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] != 3 or img.shape[1] < 1 or img.shape[2] < 1:
        raise ValueError("image_file expects uint8 [3, H, W]")
    H, W = img.shape[1:]
    rows = np.ascontiguousarray(img.transpose(1, 2, 0)).reshape(H, 3 * W)
    if fmt == "ppm":
        return b"P6\n%d %d\n255\n" % (W, H) + rows.tobytes()
    if fmt != "png":
        raise ValueError(f"image_file: format {fmt!r} is neither 'png' nor 'ppm'")
    raw = np.concatenate([np.zeros((H, 1), np.uint8), rows], axis=1).tobytes()   # filter type 0 in front of every scanline
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + _png_chunk(b"IDAT", zlib.compress(raw, 6))
            + _png_chunk(b"IEND", b""))


# ---- augmentation -----------------------------------------------------------------------------------------------------------
@dataclass
class AugParams:
    """Random state of one sample's transforms (shared by its V views, as in the reference) + per-view flips."""
    bg: Sequence[float]
    jitter_value: Sequence[float] = (1.0, 1.0, 1.0)       # brightness, contrast, saturation blend factors
    jitter_order: Sequence[int] = (0, 1, 2)
    noise_alpha: Sequence[float] = (0.0, 0.0, 0.0)        # PCA coefficients of RandomNoise
    flips: Sequence[bool] = field(default_factory=list)
    perm: Sequence[int] = (0, 1, 2)
    crop_draws: Optional[Sequence[float]] = None          # RandomCrop with a bounding box: scale, then left / right / top / bottom (:203-208)
    bg_index: Optional[int] = None                        # RandomBackground with a folder: the sample's photograph (random.choice, :439)
    bg_photo: Sequence[bool] = ()                         # ... and per view whether it takes it or the flat colour (random.randint, :447)

    def noise_rgb(self) -> np.ndarray:
        a = np.asarray(self.noise_alpha, dtype=np.float64)   # utils/data_transforms.py:373-383
        return np.sum(np.multiply(np.multiply(np.array(EIGVECS), np.tile(a, (3, 1))), np.tile(np.array(EIGVALS), (3, 1))), axis=1)


def draw_train_params(n_views: int, cfg, rng_np=np.random, rng_py=random, n_channels: int = 4, bounding_box=None,
                      n_backgrounds: int = 0) -> AugParams:
    """One __getitem__ worth of random draws in the reference's call order: RandomBackground (data_transforms.py:425-428, plus
    the per-image random.randint of :440), ColorJitter (:276-284), RandomNoise (:372), RandomFlip (:252-255),
    RandomPermuteRGB (:67).  RandomCrop draws nothing without a bounding box (:222-231).  RandomBackground returns before it draws
    anything when the renderings have no alpha channel (:428-430): pass n_channels=3 for RGB inputs.
    With a bounding_box (any non-None value; its numbers are not used here) RandomCrop, the first transform of the list
    (core/train.py:44-53), draws first: random.uniform(0.8, 1.2) and four random.uniform(.4, .6) (:203-208) -> crop_draws.
    With n_backgrounds > 0 (RandomBackground given a folder of that many files, :416-421) and four channels the sample's photograph is
    drawn after the colour - random.choice over the files (:439), here over range(n_backgrounds) - and the per-view coin flips that
    follow are kept as bg_photo instead of thrown away.  With n_backgrounds == 0 every draw is what it was without the argument."""
    if n_backgrounds < 0:
        raise ValueError(f"draw_train_params: n_backgrounds = {n_backgrounds}")
    crop_draws, bg_index, bg_photo = None, None, ()
    if bounding_box is not None:
        _refuse_box_with_views(n_views, "draw_train_params")
        crop_draws = [rng_py.uniform(0.8, 1.2)] + [rng_py.uniform(.4, .6) for _ in range(4)]
    t = cfg.TRAIN
    rg = t.RANDOM_BG_COLOR_RANGE
    if n_channels == 4:
        bg = np.array([rng_np.randint(rg[i][0], rg[i][1] + 1) for i in range(3)]) / 255.0
        if n_backgrounds > 0:
            bg_index = int(rng_py.choice(range(n_backgrounds)))
        coins = [bool(rng_py.randint(0, 1)) for _ in range(n_views)]       # drawn with or without a folder
        bg_photo = coins if n_backgrounds > 0 else ()
    else:
        bg = np.ones(3)                       # unused: the composite step is skipped for 3-channel images
    jv = [1 + rng_np.uniform(low=-t.BRIGHTNESS, high=t.BRIGHTNESS), 1 + rng_np.uniform(low=-t.CONTRAST, high=t.CONTRAST),
          1 + rng_np.uniform(low=-t.SATURATION, high=t.SATURATION)]
    order = np.array(range(3))
    rng_np.shuffle(order)
    alpha = rng_np.normal(loc=0, scale=t.NOISE_STD, size=3)
    flips = [bool(rng_py.randint(0, 1)) for _ in range(n_views)]
    perm = rng_np.permutation(3)
    return AugParams(bg=bg.tolist(), jitter_value=jv, jitter_order=[int(i) for i in order], noise_alpha=alpha.tolist(), flips=flips,
                     perm=[int(i) for i in perm], crop_draws=crop_draws, bg_index=bg_index, bg_photo=bg_photo)


def val_params(n_views: int, cfg, n_channels: int = 4) -> AugParams:
    """core/train.py:60-65: CenterCrop, RandomBackground(cfg.TEST.RANDOM_BG_COLOR_RANGE), Normalize, ToTensor (no draws for RGB inputs)."""
    rg = cfg.TEST.RANDOM_BG_COLOR_RANGE
    bg = np.array([np.random.randint(rg[i][0], rg[i][1] + 1) for i in range(3)]) / 255.0 if n_channels == 4 else np.ones(3)
    return AugParams(bg=bg.tolist(), flips=[False] * n_views)


def _refuse_box_with_views(n_views: int, who: str) -> None:
    if n_views != 1:
        raise ValueError(f"{who}: a bounding box goes with one view per sample, got {n_views}: the reference multiplies the box by the image "
                         "size again for every view (data_transforms.py:94-99 sits inside the per-image loop), which compounds for "
                         "V > 1 and is not reproduced")


def bbox_crop_rect(img_height: int, img_width: int, bounding_box=None, crop_draws=None, crop_size=None):
    """Integers of the reference's crop: (x_left, x_right, y_top, y_bottom, pad_l, pad_r, pad_t, pad_b); the kept rectangle is
    img[y_top:y_bottom + 1, x_left:x_right + 1] (inclusive) and np.pad(..., mode='edge') by the pads makes the crop that is resized.
    With a bounding_box (x0, y0, x1, y1 in fractions of the image): utils/data_transforms.py:93-130 (CenterCrop; crop_draws None)
    and :187-226 (RandomCrop; crop_draws = the five uniform draws of AugParams.crop_draws) in Python doubles and int(), so truncation
    toward zero and rounding are the reference's.  Without one: the centre crop of :137-147 / :233-243 when the image is larger
    than crop_size = (crop_h, crop_w) in both directions, else the whole image; pads 0.
    ValueError when the clamped rectangle is empty (a box outside the image, or one of negative extent): the reference slices
    nothing there and fails inside cv2.resize (for x_right or y_bottom below -1 its slice end wraps round instead; not reproduced)."""
    H, W = int(img_height), int(img_width)
    if H <= 0 or W <= 0:
        raise ValueError(f"bbox_crop_rect: bad image size {H} x {W}")
    if bounding_box is None:
        if crop_size is not None and H > crop_size[0] and W > crop_size[1] and crop_size[0] > 0 and crop_size[1] > 0:
            x_left, y_top = int(W - crop_size[1]) // 2, int(H - crop_size[0]) // 2
            return x_left, x_left + int(crop_size[1]) - 1, y_top, y_top + int(crop_size[0]) - 1, 0, 0, 0, 0
        return 0, W - 1, 0, H - 1, 0, 0, 0, 0
    if len(bounding_box) != 4:
        raise ValueError("bbox_crop_rect: a bounding box is (x0, y0, x1, y1) in fractions of the image")
    box = [float(bounding_box[0]) * W, float(bounding_box[1]) * H, float(bounding_box[2]) * W, float(bounding_box[3]) * H]
    if not all(np.isfinite(box)):
        raise ValueError(f"bbox_crop_rect: box {tuple(bounding_box)} is not finite")
    bbox_width, bbox_height = box[2] - box[0], box[3] - box[1]
    x_mid, y_mid = (box[2] + box[0]) * .5, (box[3] + box[1]) * .5
    size = max(bbox_width, bbox_height)
    if crop_draws is None:                                    # CenterCrop :108-112
        left = right = top = bottom = .5
    else:                                                     # RandomCrop :202-208
        if len(crop_draws) != 5:
            raise ValueError("bbox_crop_rect: crop_draws holds five numbers (scale, left, right, top, bottom)")
        scale, left, right, top, bottom = (float(d) for d in crop_draws)
        size = size * scale
    x_left, x_right = int(x_mid - size * left), int(x_mid + size * right)
    y_top, y_bottom = int(y_mid - size * top), int(y_mid + size * bottom)
    pad_l = pad_r = pad_t = pad_b = 0
    if x_left < 0:
        pad_l, x_left = -x_left, 0
    if x_right >= W:
        pad_r, x_right = x_right - W + 1, W - 1
    if y_top < 0:
        pad_t, y_top = -y_top, 0
    if y_bottom >= H:
        pad_b, y_bottom = y_bottom - H + 1, H - 1
    if x_left > x_right or y_top > y_bottom:
        raise ValueError(f"bbox_crop_rect: box {tuple(bounding_box)} keeps columns [{x_left}, {x_right}] and rows [{y_top}, {y_bottom}] of a "
                         f"{H} x {W} image: the rectangle is empty")
    return x_left, x_right, y_top, y_bottom, pad_l, pad_r, pad_t, pad_b


def _pack_aug_samples(params: Sequence[AugParams], V: int, cfg, who: str):
    """host side of the sv_aug_sample table and the flip bytes: (ctypes array, uint8 [len(params) * V])"""
    B = len(params)
    arr = (hip.AugSample * B)()
    flips = np.zeros(B * V, dtype=np.uint8)
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    for b, p in enumerate(params):
        if sorted(p.jitter_order) != [0, 1, 2] or sorted(p.perm) != [0, 1, 2] or len(p.flips) != V:
            raise ValueError(f"{who}: malformed AugParams")
        nz = p.noise_rgb()
        s = arr[b]
        for c in range(3):
            s.bg[c], s.jitter_value[c], s.jitter_order[c] = float(p.bg[c]), float(p.jitter_value[c]), int(p.jitter_order[c])
            s.noise[c] = float(nz[2 - c])                     # the reference adds noise_rgb[i] to channel 2 - i (:386-390)
            s.perm[c], s.mean[c], s.std[c] = int(p.perm[c]), float(mean[c]), float(std[c])
        flips[b * V:(b + 1) * V] = np.asarray(p.flips, dtype=np.uint8)
    return arr, flips


def background_bank(photos, cfg, device="cuda") -> torch.Tensor:
    """The photographs of RandomBackground's folder (utils/data_transforms.py:416-421) as one uint8 [N, IMG_H, IMG_W, 3] tensor on the
    GPU, contiguous: what augment_views(..., backgrounds=) reads.  photos: a list of uint8 [IMG_H, IMG_W, 3] arrays (numpy or tensors)
    as cv2.imread returns them - the channel order of the stored renderings -, or an already stacked array or tensor.  Nothing is
    resized or cropped: any other size, rank or dtype is a ValueError, because the reference fails on it too (its
    alpha * bg_color at :448 cannot broadcast a photograph that is not the size of the resized rendering)."""
    H, W = cfg.CONST.IMG_H, cfg.CONST.IMG_W
    why = (f"background_bank: a photograph is uint8 [{H}, {W}, 3] (cfg.CONST.IMG_H x IMG_W, three channels), got %s; the reference fails on it "
           "too: its blend cannot broadcast a photograph of another size onto the resized rendering (utils/data_transforms.py:448)")
    if isinstance(photos, (list, tuple)):
        if not photos:
            raise ValueError("background_bank: no photographs")
        host = []
        for ph in photos:
            if isinstance(ph, torch.Tensor):
                if ph.dtype != torch.uint8 or tuple(ph.shape) != (H, W, 3):
                    raise ValueError(why % f"{ph.dtype} {list(ph.shape)}")
                host.append(ph)
            else:
                ph = np.asarray(ph)
                if ph.dtype != np.uint8 or ph.shape != (H, W, 3):
                    raise ValueError(why % f"{ph.dtype} {list(ph.shape)}")
                host.append(torch.from_numpy(np.ascontiguousarray(ph)))
        bank = torch.stack(host)
    else:
        bank = photos if isinstance(photos, torch.Tensor) else None
        if bank is None:
            arr = np.asarray(photos)
            if arr.dtype != np.uint8:
                raise ValueError(why % f"{arr.dtype} {list(arr.shape)}")
            bank = torch.from_numpy(np.ascontiguousarray(arr))
        if bank.dtype != torch.uint8 or bank.dim() != 4 or bank.shape[0] < 1 or tuple(bank.shape[1:]) != (H, W, 3):
            raise ValueError(why % f"a stack {bank.dtype} {list(bank.shape)}")
    dev = bank.device if bank.is_cuda else torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("swinvox_amd: tensors must live on the GPU (no CPU path exists in the product)")
    return bank.to(dev).contiguous()


def _bg_index_table(params: Sequence[AugParams], V: int, cfg, backgrounds) -> np.ndarray:
    """host side of sv_augment_views_bg's table, int32 [len(params) * V]: the sample's photograph for a view whose coin says so, else -1"""
    H, W = cfg.CONST.IMG_H, cfg.CONST.IMG_W
    if not isinstance(backgrounds, torch.Tensor) or backgrounds.dtype != torch.uint8 or backgrounds.dim() != 4 or \
            backgrounds.shape[0] < 1 or tuple(backgrounds.shape[1:]) != (H, W, 3):
        got = f"{backgrounds.dtype} {list(backgrounds.shape)}" if isinstance(backgrounds, torch.Tensor) else type(backgrounds).__name__
        raise ValueError(f"augment_views: backgrounds is a uint8 [N, {H}, {W}, 3] tensor (data.background_bank; cfg.CONST.IMG_H x IMG_W), got {got}")
    n_bank = backgrounds.shape[0]
    table = np.full(len(params) * V, -1, dtype=np.int32)
    for b, p in enumerate(params):
        if len(p.bg_photo) not in (0, V):
            raise ValueError(f"augment_views: sample {b} has {len(p.bg_photo)} bg_photo flags for {V} views (none, or one per view)")
        if p.bg_index is None:
            continue
        if not 0 <= int(p.bg_index) < n_bank:
            raise ValueError(f"augment_views: sample {b} asks for photograph {p.bg_index} of a bank of {n_bank}")
        for v, take in enumerate(p.bg_photo):
            if take:
                table[b * V + v] = int(p.bg_index)
    return table


def augment_views(images_u8: torch.Tensor, params: Sequence[AugParams], cfg, backgrounds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """images_u8 [B, V, Hs, Ws, C] uint8 on the GPU (C = 4 with alpha or 3, channel order as stored) -> float32
    [B, V, 3, IMG_H, IMG_W]: the tensor the reference's DataLoader hands to core/train.py:222.
    backgrounds: None, or a bank of photographs (background_bank) - RandomBackground with a folder (utils/data_transforms.py:437-448).
    View v of sample b then shows photograph params[b].bg_index where the rendering is transparent if params[b].bg_photo[v] is set,
    and the flat colour params[b].bg otherwise (always, for a sample whose bg_index is None); draw_train_params(n_backgrounds=N) draws
    both.  The bank and the parameters are checked (ValueError) before anything else happens."""
    table = None
    if backgrounds is not None:
        if images_u8.dim() != 5:
            raise RuntimeError("augment_views expects uint8 [B, V, Hs, Ws, C]")
        table = _bg_index_table(params, images_u8.shape[1], cfg, backgrounds)
        hip.check_cuda(backgrounds)
    hip.check_cuda(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 5:
        raise RuntimeError("augment_views expects uint8 [B, V, Hs, Ws, C]")
    B, V, Hs, Ws, Cc = images_u8.shape
    if len(params) != B:
        raise ValueError("augment_views: one AugParams per sample")
    images_u8 = images_u8.contiguous()
    arr, flips = _pack_aug_samples(params, V, cfg, "augment_views")
    dev = images_u8.device
    prm = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    fl = torch.from_numpy(flips).to(dev)
    ws = torch.empty(B * V, dtype=torch.float64, device=dev)
    H, W = cfg.CONST.IMG_H, cfg.CONST.IMG_W
    out = torch.empty(B, V, 3, H, W, dtype=torch.float32, device=dev)
    if table is None:
        call("sv_augment_views", ptr(images_u8), B * V, V, Hs, Ws, Cc, cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W, H, W, ptr(prm), ptr(fl),
             ptr(ws), ptr(out))
        return out
    if backgrounds.device != dev:
        raise RuntimeError(f"augment_views: the bank lives on {backgrounds.device}, the renderings on {dev}")
    bank = backgrounds.contiguous()
    table_dev = torch.empty(B * V, dtype=torch.int32, device=dev)
    call("sv_augment_views_bg", ptr(images_u8), B * V, V, Hs, Ws, Cc, cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W, H, W, ptr(prm), ptr(fl),
         ptr(bank), bank.shape[0], table.ctypes.data, ptr(table_dev), ptr(ws), ptr(out))
    return out


def augment_images(images, boxes, params: Sequence[AugParams], cfg, sizes=None, device="cuda") -> torch.Tensor:
    """A batch of photographs of differing sizes, one view per sample, each cropped to its bounding box: what the reference's
    Pascal3D / Pix3D datasets hand to core/train.py:222 (utils/data_loaders.py:176-203, :311-338 with the transform lists of
    core/train.py:44-59) -> float32 [B, 1, 3, IMG_H, IMG_W].
    images: a list of B uint8 arrays (numpy or CPU tensors) [Hs_i, Ws_i, C] with one C (3, or 4 with alpha) for the whole batch; a 2-D
    greyscale image is stacked to three channels (data_loaders.py:194-196).  They are packed end to end into one buffer that goes to
    `device` in one copy.  Or: that packed buffer itself, a 1-D uint8 tensor already on the GPU, with sizes = [(Hs_i, Ws_i, C), ...]
    in packing order.
    boxes: None, or per image None / (x0, y0, x1, y1) in fractions of the image.  A boxed image is cropped by bbox_crop_rect with
    its AugParams.crop_draws (None = CenterCrop, the validation list), an unboxed one by the centre-crop rule of augment_views."""
    if isinstance(images, torch.Tensor) and sizes is None:
        raise RuntimeError("augment_images: a packed buffer comes with sizes = [(Hs, Ws, C), ...]; separate images go in a list")
    B = len(sizes) if isinstance(images, torch.Tensor) else len(images)
    if B == 0:
        raise ValueError("augment_images: no images")
    if len(params) != B:
        raise ValueError("augment_images: one AugParams per image")
    boxes = [None] * B if boxes is None else list(boxes)
    if len(boxes) != B:
        raise ValueError("augment_images: one bounding box (or None) per image")
    if isinstance(images, torch.Tensor):
        hip.check_cuda(images)
        if images.dtype != torch.uint8 or images.dim() != 1 or not images.is_contiguous():
            raise RuntimeError("augment_images expects the packed buffer as contiguous 1-D uint8")
        if any(len(s) != 3 for s in sizes):
            raise RuntimeError("augment_images: sizes holds one (Hs, Ws, C) per packed image")
        shapes, packed = [tuple(int(v) for v in s) for s in sizes], images
    else:
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("swinvox_amd: tensors must live on the GPU (no CPU path exists in the product)")
        host = []
        for im in images:
            im = im.numpy() if isinstance(im, torch.Tensor) else np.asarray(im)
            if im.dtype != np.uint8 or im.ndim not in (2, 3):
                raise RuntimeError("augment_images expects uint8 images [Hs, Ws, C] (or [Hs, Ws] greyscale)")
            if im.ndim == 2:
                im = np.stack((im, ) * 3, -1)
            host.append(im)
        shapes = [im.shape for im in host]
        packed = None
    Cc = shapes[0][2]
    if Cc not in (3, 4) or any(s[2] != Cc for s in shapes) or any(s[0] <= 0 or s[1] <= 0 for s in shapes):
        raise RuntimeError(f"augment_images: every image of a call is [Hs, Ws, C] with the same C = 3 or 4, got {sorted(set(shapes))}")
    crop = (cfg.CONST.CROP_IMG_H, cfg.CONST.CROP_IMG_W)
    desc, off = (hip.AugImage * B)(), 0
    for i, ((Hs, Ws, _), box, p) in enumerate(zip(shapes, boxes, params)):
        rect = bbox_crop_rect(Hs, Ws, box, p.crop_draws if box is not None else None, crop)
        if max(rect[4:]) > 1 << 24:                           # the entry's limit; checked here because a ctypes int field wraps silently
            raise ValueError(f"augment_images: box {tuple(box)} pads image {i} by {rect[4:]} pixels (at most 2^24)")
        d = desc[i]
        d.offset, d.Hs, d.Ws = off, Hs, Ws
        d.x_left, d.x_right, d.y_top, d.y_bottom, d.pad_l, d.pad_r, d.pad_t, d.pad_b = rect
        off += Hs * Ws * Cc
    arr, flips = _pack_aug_samples(params, 1, cfg, "augment_images")
    if packed is None:
        buf = np.empty(off, dtype=np.uint8)
        for d, im in zip(desc, host):
            buf[d.offset:d.offset + im.size] = im.reshape(-1)
        packed = torch.from_numpy(buf).to(dev)
        hip.check_cuda(packed)
    elif packed.numel() < off:
        raise RuntimeError(f"augment_images: the packed buffer holds {packed.numel()} bytes, sizes describe {off}")
    dev = packed.device
    prm = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    fl = torch.from_numpy(flips).to(dev)
    ws = torch.empty(B, dtype=torch.float64, device=dev)
    desc_dev = torch.empty(B * C.sizeof(hip.AugImage), dtype=torch.uint8, device=dev)
    H, W = cfg.CONST.IMG_H, cfg.CONST.IMG_W
    out = torch.empty(B, 1, 3, H, W, dtype=torch.float32, device=dev)
    call("sv_augment_images", ptr(packed), packed.numel(), B, Cc, C.addressof(desc), ptr(desc_dev), H, W, ptr(prm), ptr(fl), ptr(ws), ptr(out))
    return out
