"""The picture of a voxel volume, as a definition: a ray-cast of the camera the reference's get_volume_views (utils/helpers.py:50-88)
ends up with, one face id per pixel, and an integer shading rule on the ids.  numpy only; imports nothing from the package.  It is the
expected value of sv_render_volumes (include/swinvox_hip.h states the same rule) and is itself pinned to the reference's pictures by
tests/test_cpu_volume_view.py.

A camera is 18 numbers [6, 3] = o0, ox, oy, d0, dx, dy: the ray of pixel (row, col) has origin = o0 + (col+0.5) ox + (row+0.5) oy and
dir = d0 + (col+0.5) dx + (row+0.5) dy in the array's own coordinates (voxel (i, j, k) fills [i, i+1] x [j, j+1] x [k, k+1]); row 0 is
the top of the image."""
import numpy as np

FACE_NAMES = ("-x", "+x", "-y", "+y", "-z", "+z")


def view_camera(dims, elev=30, azim=45, size=(480, 640), proj_type="persp"):
    """float64 [6, 3]: the camera of matplotlib's Axes3D for limits 0..dims, set_box_aspect([1, 1, 1]), view_init(elev, azim), focal
    length 1 and distance 10 in subplot(111) of a figure of size = (H, W) pixels (6.4 x 4.8 in at 100 dpi for (480, 640)); restated
    from axes3d.py (set_box_aspect, get_proj, set_top_view, apply_aspect) and proj3d.py.  "ortho" is proj_type='ortho' there."""
    if proj_type not in ("persp", "ortho"):
        raise ValueError(f"view_camera: proj_type {proj_type!r} is neither 'persp' nor 'ortho'")
    H, W = int(size[0]), int(size[1])
    d = np.asarray(dims, np.float64)
    if d.shape != (3,) or (d < 1).any() or H < 1 or W < 1:
        raise ValueError("view_camera: dims are three positive numbers, size is (H, W)")
    dist = 10.0
    aspect = np.ones(3)
    aspect *= 1.8294640721620434 * 25 / 24 * 1 / np.linalg.norm(aspect)          # set_box_aspect
    scale = aspect / d                                                          # world = data * scale (world_transformation, limits 0..dims)
    R = 0.5 * aspect
    er, ar = np.deg2rad(elev), np.deg2rad(azim)
    ps = np.array([np.cos(er) * np.cos(ar), np.cos(er) * np.sin(ar), np.sin(er)])
    eye = R + dist * ps
    en = (elev + 180.0) % 360.0 - 180.0                                         # art3d._norm_angle
    V = np.array([0.0, 0.0, -1.0 if abs(np.deg2rad(en)) > np.pi / 2 else 1.0])
    w = (eye - R) / np.linalg.norm(eye - R)
    u = np.cross(V, w)
    u = u / np.linalg.norm(u)
    v = np.cross(w, u)
    # subplot(111): left .125 right .9 bottom .11 top .88 of the figure, shrunk to a square (apply_aspect) about its centre; the view
    # limits of set_top_view are (-0.95 / dist, 0.9 / dist) on both axes.  Display y runs upwards: y = H - (row + 0.5).
    side = min(0.775 * W, 0.77 * H)
    ax0, ay0 = 0.125 * W + 0.5 * (0.775 * W - side), 0.11 * H + 0.5 * (0.77 * H - side)
    lo, span = -0.95 / dist, (0.9 + 0.95) / dist
    xa, xb = lo - ax0 * span / side, span / side                                # x' = xa + xb (col + 0.5)
    ya, yb = lo + (H - ay0) * span / side, -span / side                         # y' = ya + yb (row + 0.5)
    cam = np.zeros((6, 3))
    if proj_type == "persp":                                                    # clip x = e.x, clip w = -e.z: the ray x' u + y' v - w from the eye
        cam[0] = eye / scale
        cam[3] = (xa * u + ya * v - w) / scale
        cam[4] = xb * u / scale
        cam[5] = yb * v / scale
    else:                                                                       # clip x = 2 e.x, clip w = 2 dist: e.x = dist x'
        cam[0] = (eye + dist * (xa * u + ya * v)) / scale
        cam[1] = dist * xb * u / scale
        cam[2] = dist * yb * v / scale
        cam[3] = -w / scale
    return cam


def top_down_camera(dims, size=None):
    """orthographic, looking along -z from above: pixel (row, col) sees the column (i = row, j = col) when size = (d0, d1)"""
    d0, d1, d2 = (int(x) for x in dims)
    H, W = (d0, d1) if size is None else size
    cam = np.zeros((6, 3))
    cam[0] = (0.0, 0.0, d2 + 1.0)
    cam[1] = (0.0, d1 / W, 0.0)
    cam[2] = (d0 / H, 0.0, 0.0)
    cam[3] = (0.0, 0.0, -1.0)
    return cam


def render_ids(vol, cam, size, dtype=np.float32):
    """int32 [H, W]: id = ((i d1 + j) d2 + k) 6 + face of the first set voxel on each pixel's ray and the face (-x +x -y +y -z +z) the ray
    entered it through, -1 for background.  Every step is one operation in `dtype` (float32 is the definition, float64 the variant of
    the sensitivity check)."""
    vol = np.asarray(vol) != 0
    D = vol.shape
    H, W = int(size[0]), int(size[1])
    f = dtype
    cam = np.asarray(cam, np.float64).reshape(6, 3).astype(f)
    px = np.broadcast_to(np.arange(W, dtype=f)[None, :] + f(0.5), (H, W)).reshape(-1)
    py = np.broadcast_to(np.arange(H, dtype=f)[:, None] + f(0.5), (H, W)).reshape(-1)
    n = H * W
    inf = f(np.inf)
    o, d, tnear, tfar = [], [], [], []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for a in range(3):
            oa = (cam[0, a] + px * cam[1, a]) + py * cam[2, a]
            da = (cam[3, a] + px * cam[4, a]) + py * cam[5, a]
            nz = da != 0
            safe = np.where(nz, da, f(1))
            t0 = (f(0) - oa) / safe
            t1 = (f(D[a]) - oa) / safe
            inside = (oa >= 0) & (oa < f(D[a]))
            tnear.append(np.where(nz, np.minimum(t0, t1), np.where(inside, -inf, inf)).astype(f))
            tfar.append(np.where(nz, np.maximum(t0, t1), np.where(inside, inf, -inf)).astype(f))
            o.append(oa)
            d.append(da)
        tn = np.stack(tnear)
        axis = np.argmax(tn, axis=0)                                            # first arg-max: x before y before z
        tin = tn.max(axis=0)
        tout = np.minimum(np.minimum(tfar[0], tfar[1]), tfar[2])
        hit = (tin < tout) & (tin > 0)
        idx = np.flatnonzero(hit)
        ids = np.full(n, -1, np.int32)
        if idx.size == 0:
            return ids.reshape(H, W)
        axis, tin = axis[idx], tin[idx]
        o = [x[idx] for x in o]
        d = [x[idx] for x in d]
        cell, step, tmax, tdelta = [], [], [], []
        for a in range(3):
            p = o[a] + d[a] * tin
            c = np.minimum(np.maximum(np.floor(p), f(0)), f(D[a] - 1)).astype(np.int32)
            pos = d[a] > 0
            c = np.where(axis == a, np.where(pos, 0, D[a] - 1), c).astype(np.int32)
            nz = d[a] != 0
            safe = np.where(nz, d[a], f(1))
            cell.append(c)
            step.append(np.where(nz, np.where(pos, 1, -1), 0).astype(np.int32))
            tmax.append(np.where(nz, ((c + pos.astype(np.int32)).astype(f) - o[a]) / safe, inf).astype(f))
            tdelta.append(np.where(nz, np.abs(f(1) / safe), inf).astype(f))
        cell, step, tmax, tdelta = np.stack(cell), np.stack(step), np.stack(tmax), np.stack(tdelta)
        face = (2 * axis + (step[axis, np.arange(idx.size)] < 0)).astype(np.int32)
        out = np.full(idx.size, -1, np.int32)
        live = np.arange(idx.size)
        for _ in range(D[0] + D[1] + D[2]):
            if live.size == 0:
                break
            ci, cj, ck = cell[0, live], cell[1, live], cell[2, live]
            filled = vol[ci, cj, ck]
            out[live[filled]] = ((ci[filled] * D[1] + cj[filled]) * D[2] + ck[filled]) * 6 + face[live[filled]]
            live = live[~filled]
            if live.size == 0:
                break
            a = np.argmin(tmax[:, live], axis=0)                                # first arg-min
            cell[a, live] += step[a, live]
            tmax[a, live] += tdelta[a, live]
            face[live] = 2 * a + (step[a, live] < 0)
            c = cell[a, live]
            live = live[(c >= 0) & (c < np.asarray(D)[a])]
    ids[idx] = out
    return ids.reshape(H, W)


def edge_mask(ids):
    """a pixel is an edge pixel iff its id differs from its right or its lower neighbour's (the pixel itself at the last column / row)"""
    right = np.concatenate([ids[..., :, 1:], ids[..., :, -1:]], axis=-1)
    below = np.concatenate([ids[..., 1:, :], ids[..., -1:, :]], axis=-2)
    return (ids != right) | (ids != below)


def shade(ids, face_rgb, edge_rgb=(0, 0, 0), background=(255, 255, 255)):
    """uint8 [..., 3, H, W] from ids [..., H, W]: edge pixels edge_rgb, other hit pixels face_rgb[id % 6], other background pixels the
    background - a colour, or a uint8 [3, H, W] plate"""
    ids = np.asarray(ids)
    face_rgb = np.asarray(face_rgb, np.uint8).reshape(6, 3)
    bg = np.asarray(background, np.uint8)
    bg = np.broadcast_to(bg[:, None, None] if bg.ndim == 1 else bg, (3,) + ids.shape[-2:])
    edge = edge_mask(ids)
    out = np.empty(ids.shape[:-2] + (3,) + ids.shape[-2:], np.uint8)
    for c in range(3):
        plane = np.where(ids >= 0, face_rgb[np.maximum(ids, 0) % 6, c], bg[c])
        out[..., c, :, :] = np.where(edge, np.uint8(edge_rgb[c]), plane)
    return out


def dilate(mask, r):
    """square (Chebyshev) dilation by r pixels"""
    m = np.pad(mask, r)
    H, W = mask.shape
    out = np.zeros_like(mask)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= m[dy:dy + H, dx:dx + W]
    return out


def erode(mask, r):
    return ~dilate(~mask, r)


def uniform3x3(ids):
    """pixels whose 3 x 3 neighbourhood (inside the image) holds one id"""
    H, W = ids.shape
    m = np.pad(ids, 1, mode="edge")
    same = np.ones((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            same &= m[dy:dy + H, dx:dx + W] == ids
    return same


def in_neighbourhood(got, want):
    """per pixel: got's id occurs in want's 3 x 3 neighbourhood of that pixel"""
    H, W = want.shape
    m = np.pad(want, 1, mode="edge")
    ok = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            ok |= m[dy:dy + H, dx:dx + W] == got
    return ok
