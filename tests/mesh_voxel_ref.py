"""Numpy int64 restatement of the mesh voxelisation rule (sv_voxelise_meshes in include/swinvox_hip.h): the expected value of
test_cpu_mesh_voxelise.py and test_gpu_mesh_voxelise.py.  Test infrastructure only; the product does not import it.

  units     S = 1024 per voxel; voxel (i, j, k) is the closed cube [iS, (i+1)S] x [jS, (j+1)S] x [kS, (k+1)S], its centre the lattice
            point ((2i+1)H, (2j+1)H, (2k+1)H), H = S / 2.  verts are integers in these units, each inside [-d S, 2 d S] of its axis.
  solid     per triangle a, b, c with n = (b - a) x (c - a): skipped when n.z == 0; for the edge tests b and c change places when
            n.z < 0.  Column (Px, Py) is covered when every directed edge u -> v, d = v - u, has E = d.x (Py - u.y) - d.y (Px - u.x) > 0,
            or E == 0 and (d.y < 0 or (d.y == 0 and d.x < 0)).  Voxel k of a covered column is toggled iff
            sgn(n.z) (n.x (Px - a.x) + n.y (Py - a.y) + n.z (zk - a.z)) > 0.  Set = toggled an odd number of times.
  surface   per triangle with n != 0: set iff no one of 13 axes separates the triangle from the cube - the cube's 3 normals, n, and the 9
            cross products of a cube axis with an edge; on an axis the cube reaches H (|x| + |y| + |z|) from its centre, and only a
            projection strictly beyond that separates (closed sets: touching counts).
  both      surface | solid

Loops over the triangles, vectorised over the voxels.  clip=True only restricts each triangle to the voxels its bounding box can reach
(for timing); the tests check that it changes nothing.
"""
import numpy as np

S, H = 1024, 512
MODES = ("solid", "surface", "both")


def _normal(a, b, c):
    e1, e2 = [b[q] - a[q] for q in range(3)], [c[q] - a[q] for q in range(3)]
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def _window(pts, dims, centres, clip):
    """index ranges (slices) of the voxels a triangle can touch: everything, or with clip its bounding box"""
    if not clip:
        return tuple(slice(0, d) for d in dims)
    out = []
    for q, d in enumerate(dims):
        lo, hi = min(p[q] for p in pts), max(p[q] for p in pts)
        if centres and q < 2:
            first, last = -((H - lo) // S), (hi - H) // S                  # ceil((lo - H) / S), floor((hi - H) / S)
        else:
            first, last = -((-lo) // S) - 1, hi // S                        # cubes [iS, (i+1)S] that meet [lo, hi]
        out.append(slice(max(first, 0), max(min(last, d - 1) + 1, max(first, 0))))
    return tuple(out)


def solid(verts, tris, dims, clip=False):
    """verts int [n, 3] snapped, tris int [m, 3] -> bool [d0, d1, d2]"""
    d0, d1, d2 = dims
    out = np.zeros(dims, bool)
    V = np.asarray(verts, np.int64).reshape(-1, 3).tolist()                 # Python integers: the scalar products cannot overflow
    for t in np.asarray(tris, np.int64).reshape(-1, 3).tolist():
        a, b, c = V[t[0]], V[t[1]], V[t[2]]
        n = _normal(a, b, c)
        if n[2] == 0:
            continue
        wi, wj, wk = _window((a, b, c), dims, True, clip)
        wk = slice(0, d2)
        Px = ((2 * np.arange(d0, dtype=np.int64) + 1) * H)[wi, None]
        Py = ((2 * np.arange(d1, dtype=np.int64) + 1) * H)[None, wj]
        zk = ((2 * np.arange(d2, dtype=np.int64) + 1) * H)[wk]
        bb, cc = (c, b) if n[2] < 0 else (b, c)
        covered = np.ones((Px.shape[0], Py.shape[1]), bool)
        for u, v in ((a, bb), (bb, cc), (cc, a)):
            dx, dy = v[0] - u[0], v[1] - u[1]
            E = dx * (Py - u[1]) - dy * (Px - u[0])
            owns = dy < 0 or (dy == 0 and dx < 0)
            covered &= (E > 0) | ((E == 0) & owns)
        sgn = 1 if n[2] > 0 else -1
        plane = (sgn * (n[0] * (Px - a[0]) + n[1] * (Py - a[1])))[:, :, None] + (sgn * n[2] * (zk - a[2]))[None, None, :]
        out[wi, wj, wk] ^= covered[:, :, None] & (plane > 0)
    return out


def surface(verts, tris, dims, clip=False):
    """verts int [n, 3] snapped, tris int [m, 3] -> bool [d0, d1, d2]"""
    out = np.zeros(dims, bool)
    V = np.asarray(verts, np.int64).reshape(-1, 3).tolist()
    for t in np.asarray(tris, np.int64).reshape(-1, 3).tolist():
        tri = (V[t[0]], V[t[1]], V[t[2]])
        n = _normal(*tri)
        if n == [0, 0, 0]:
            continue
        w = _window(tri, dims, False, clip)
        shape = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
        centre = [((2 * np.arange(d, dtype=np.int64) + 1) * H)[w[q]].reshape(shape[q]) for q, d in enumerate(dims)]
        p = [[v[q] - centre[q] for q in range(3)] for v in tri]             # vertices relative to every cube's centre
        axes = [(1, 0, 0), (0, 1, 0), (0, 0, 1), tuple(n)]
        for e in range(3):
            fx, fy, fz = (tri[(e + 1) % 3][q] - tri[e][q] for q in range(3))
            axes += [(0, -fz, fy), (fz, 0, -fx), (-fy, fx, 0)]
        separated = np.zeros([len(range(*s.indices(d))) for s, d in zip(w, dims)], bool)
        for ax in axes:
            proj = [ax[0] * pv[0] + ax[1] * pv[1] + ax[2] * pv[2] for pv in p]
            lo, hi = np.minimum(np.minimum(proj[0], proj[1]), proj[2]), np.maximum(np.maximum(proj[0], proj[1]), proj[2])
            r = H * (abs(ax[0]) + abs(ax[1]) + abs(ax[2]))
            separated |= (lo > r) | (hi < -r)
        out[w] |= ~separated
    return out


def voxelise(verts, tris, dims, mode="both", clip=False):
    if mode not in MODES:
        raise ValueError(mode)
    dims = tuple(int(d) for d in dims)
    out = np.zeros(dims, bool)
    if mode != "surface":
        out |= solid(verts, tris, dims, clip)
    if mode != "solid":
        out |= surface(verts, tris, dims, clip)
    return out


# ---- shared cases -------------------------------------------------------------------------------------------------------------------
def soup(dims, seed, n=200):
    """n random triangles, not closed -> (verts int64 [3n, 3], tris int64 [n, 3]).  Triangle 0 spans the whole grid; the others cycle
    through: vertices on the half-voxel lattice (ties), slivers thinner than a unit, triangles inside one voxel, vertices anywhere in
    the admitted range [-d S, 2 d S] (outside the grid), and triangles of a voxel or two."""
    rng = np.random.default_rng(seed)
    d = np.asarray(dims, np.int64)
    pts = np.zeros((n, 3, 3), np.int64)
    for t in range(n):
        kind = t % 5
        if t == 0:
            pts[t] = [[-H, -H, 3], [d[0] * S + 7, 5, d[2] * H + 1], [11, d[1] * S + H, d[2] * S - 9]]
        elif kind == 0:
            pts[t] = rng.integers(0, 2 * d + 1, (3, 3)) * H
        elif kind == 1:
            a, b = rng.integers(0, d * S + 1, (2, 3))
            c = (a + b) // 2
            c[rng.integers(0, 3)] += rng.integers(-1, 2)                    # at most one unit off the segment (a zero normal now and then)
            pts[t] = [a, b, c]
        elif kind == 2:
            pts[t] = rng.integers(0, d) * S + rng.integers(1, S, (3, 3))
        elif kind == 3:
            pts[t] = rng.integers(-d * S, 2 * d * S + 1, (3, 3))
        else:
            pts[t] = rng.integers(0, d * S + 1) + rng.integers(-S, S + 1, (3, 3))
    return pts.reshape(-1, 3), np.arange(3 * n, dtype=np.int64).reshape(n, 3)


def tie_cases():
    """name -> (verts int64, tris int64, dims): solids whose parity test runs into the tie rule"""
    cases = {}
    c = 9 * H                                                               # the centre of voxel 4 of an 8-grid
    octa = [[c, c, 1 * S + 7], [c, c, 7 * S - 7], [c - 5 * H, c, 4 * S + 3], [c, c - 5 * H, 4 * S + 3], [c + 5 * H, c, 4 * S + 3], [c, c + 5 * H, 4 * S + 3]]
    faces = [[0, 2 + q, 2 + (q + 1) % 4] for q in range(4)] + [[1, 2 + (q + 1) % 4, 2 + q] for q in range(4)]
    cases["octahedron_apex_on_a_centre_column"] = (np.asarray(octa, np.int64), np.asarray(faces, np.int64), (8, 8, 8))
    # a ridge along the column line x = 4.5 voxels: two roof planes share it, two floor triangles below close the solid sideways open
    roof = [[c, 1 * S, 6 * S], [c, 7 * S, 6 * S], [1 * S, 1 * S, 3 * S], [1 * S, 7 * S, 3 * S], [7 * S, 1 * S, 2 * S], [7 * S, 7 * S, 2 * S],
            [1 * S, 1 * S, S], [1 * S, 7 * S, S], [7 * S, 1 * S, S], [7 * S, 7 * S, S]]
    faces = [[0, 1, 3], [0, 3, 2], [0, 4, 5], [0, 5, 1], [6, 7, 9], [6, 9, 8]]
    cases["edge_along_a_column_line"] = (np.asarray(roof, np.int64), np.asarray(faces, np.int64), (8, 8, 8))
    # a box whose bottom and top lie exactly on centres (z = 1.5 and 3.5 voxels): by the rule it holds k = 2 and 3
    x0, x1, z0, z1 = S, 3 * S, 3 * H, 7 * H
    box = [[x, y, z] for x in (x0, x1) for y in (x0, x1) for z in (z0, z1)]
    quads = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]
    faces = [[q[0], q[i], q[i + 1]] for q in quads for i in (1, 2)]
    cases["centre_on_a_triangle_plane"] = (np.asarray(box, np.int64), np.asarray(faces, np.int64), (5, 5, 5))
    return cases
