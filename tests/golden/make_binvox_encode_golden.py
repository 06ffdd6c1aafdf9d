#!/usr/bin/env python3
"""Golden vectors for the binvox run-length WRITER, produced by the REFERENCE's own utils/binvox_rw.py (numpy only, importable
in the build container).  Each case is a file-order ([d0][d1][d2], 'xzy') boolean array written with the reference writer and
read back with the reference reader; the fixture stores the file bytes, the xyz array (bit-packed) and the dims.  The cases
are chosen for what the writer's (state, ctr) loop does at multiples of 255: it dumps (state, 255) and restarts the counter at
0, so a switch of value right after a dump writes a ZERO-COUNT pair, and a final run that ends on a multiple of 255 is not
flushed.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_binvox_encode_golden.py      (never runs on the GPU box)"""
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

spec = importlib.util.spec_from_file_location("ref_binvox_rw", "/root/reference/utils/binvox_rw.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)


def flat_case(dims, *ranges):
    z = np.zeros(int(np.prod(dims)), bool)
    for lo, hi in ranges:
        z[lo:hi] = True
    return z.reshape(dims)


def zero_count_pairs(raw):
    payload = np.frombuffer(raw[raw.index(b"data\n") + 5:], dtype=np.uint8)
    return len(payload) // 2, int((payload[1::2] == 0).sum())


cases = {
    "runs255_16": (flat_case((16, 16, 16), (255, 765), (1020, 1275), (1276, 1277)), [0.0, 0.0, 0.0], 1.0),
    "tail255_8": (flat_case((8, 8, 8), (512 - 255, 512)), [0.0, 0.0, 0.0], 1.0),
    "alt8": ((np.arange(512) % 2 == 1).reshape(8, 8, 8), [0.0, 0.0, 0.0], 1.0),
    "full32_holes": (flat_case((32, 32, 32), (1, 32767)), [0.0, 0.0, 0.0], 1.0),
    "long_exact": (flat_case((32, 32, 32), (765, 765 + 255 * 40)), [0.0, 0.0, 0.0], 1.0),
    "half32": (np.random.default_rng(11).random((32, 32, 32)) < 0.5, [0.0, 0.0, 0.0], 1.0),
    "noncubic": (np.random.default_rng(13).random((4, 6, 10)) < 0.4, [-0.5, 0.25, 0.0], 0.75),
}


def write(xzy, translate, scale):
    fp = io.BytesIO()
    ref.write(ref.Voxels(xzy, list(xzy.shape), translate, scale, "xzy"), fp)
    return fp.getvalue()


# sparse32: the first seed whose p = 0.03 draw holds a run of a multiple of 255 voxels followed by a switch (recorded in the fixture)
for SPARSE_SEED in range(100000):
    draw = np.random.default_rng(SPARSE_SEED).random((32, 32, 32)) < 0.03
    flat = draw.reshape(-1).astype(np.int8)
    edges = np.flatnonzero(np.diff(flat)) + 1
    lens = np.diff(np.concatenate([[0], edges]))                    # every run but the last
    if (lens % 255 == 0).any():
        break
cases["sparse32"] = (draw, [0.0, 0.0, 0.0], 1.0)

out, report = {"sparse32_seed": np.array(SPARSE_SEED)}, []
for name, (xzy, translate, scale) in cases.items():
    raw = write(xzy, translate, scale)
    back = ref.read_as_3d_array(io.BytesIO(raw), fix_coords=False)
    assert back.data.dtype == bool and np.array_equal(back.data, xzy), name
    assert back.dims == list(xzy.shape) and back.translate == translate and back.scale == scale, name
    xyz = ref.read_as_3d_array(io.BytesIO(raw)).data
    assert np.array_equal(xyz, np.transpose(xzy, (0, 2, 1))), name
    if len(set(xzy.shape)) == 1:                                   # cubic: the 'xyz' branch on the transposed array writes the same bytes
        fp = io.BytesIO()
        ref.write(ref.Voxels(xyz, list(xzy.shape), translate, scale, "xyz"), fp)
        assert fp.getvalue() == raw, name
    out[name + "_file"] = np.frombuffer(raw, dtype=np.uint8)
    out[name + "_xyz"] = np.packbits(xyz.reshape(-1))
    out[name + "_dims"] = np.array(xzy.shape)
    report.append((name, *zero_count_pairs(raw)))
zc = {name: z for name, _, z in report}
assert zc["runs255_16"] == 4 and zc["long_exact"] == 2 and zc["sparse32"] >= 1, zc
assert zc["tail255_8"] == 0 and out["tail255_8_file"][-6:].tolist() == [0, 255, 0, 2, 1, 255]
assert dict((n, p) for n, p, _ in report)["alt8"] == 512
np.savez_compressed(os.path.join(HERE, "binvox_encode_cases.npz"), **out)
for name, pairs, z in report:
    print(f"{name:14s} {pairs:6d} pairs, {z} with a zero count")
print("wrote", len(cases), "cases written and read back by the reference module; sparse32 seed", SPARSE_SEED)
