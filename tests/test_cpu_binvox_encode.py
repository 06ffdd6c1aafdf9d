"""The binvox writer (csrc/dataprep.hip sv_binvox_encode, data.binvox_header / encode_binvox_batch) without a GPU: the header declares
the entry and cites the reference writer, the ctypes table binds it, the argument refusals - host-side checks that run before any GPU
call - answer SV_ERR_INVALID with the entry's name, data.binvox_header reproduces the header bytes of every fixture, and the fixtures
(tests/golden/binvox_encode_cases.npz, written by the reference's own utils/binvox_rw.py) are intact.

rle_pairs() below restates the reference writer's (state, ctr) loop in closed form; it reproduces every fixture payload here and is
the expected value of the GPU tests (test_gpu_binvox_encode.py) for generated volumes."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import data as OD
from swinvox_amd import data as D
from swinvox_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "binvox_encode_cases.npz"))
CASES = ("runs255_16", "tail255_8", "alt8", "full32_holes", "long_exact", "half32", "sparse32", "noncubic")
ENTRY = "sv_binvox_encode"
SV_ERR_INVALID = -1


def golden(name):
    """(file bytes, xyz bool array, dims) of a fixture"""
    dims = [int(d) for d in G[name + "_dims"]]
    xyz = np.unpackbits(G[name + "_xyz"])[:int(np.prod(dims))].astype(bool).reshape(dims[0], dims[2], dims[1])
    return G[name + "_file"].tobytes(), xyz, dims


def payload_of(raw: bytes) -> bytes:
    return raw[D.parse_binvox_header(raw)[3]:]


def rle_pairs(flat) -> bytes:
    """utils/binvox_rw.py:272-292 in closed form, `flat` in file order: a run of n equal voxels that is not the last emits n // 255
    pairs (v, 255) and then (v, n % 255) even when that count is 0 (the writer restarts its counter at 0 after a dump at 255 and dumps
    it as it is on the next switch); the last run emits (v, n % 255) only when it is non-zero."""
    flat = np.asarray(flat).reshape(-1).astype(np.uint8)
    edges = np.flatnonzero(np.diff(flat)) + 1
    starts, ends = np.concatenate([[0], edges]), np.concatenate([edges, [flat.size]])
    out = bytearray()
    for r, (s, e) in enumerate(zip(starts, ends)):
        n, v = int(e - s), int(flat[s])
        out += bytes((v, 255)) * (n // 255)
        if r + 1 < len(starts) or n % 255 > 0:
            out += bytes((v, n % 255))
    return bytes(out)


def file_order(xyz):
    """xyz [..., a, b, c] -> the file's [..., a, c, b] order, flattened per volume"""
    return np.swapaxes(np.asarray(xyz), -1, -2).reshape(*np.asarray(xyz).shape[:-3], -1)


def test_header_declares_and_cites():
    hdr = open(os.path.join(ROOT, "include", "swinvox_hip.h")).read()
    m = re.search(r"(/\*(?:(?!\*/).)*\*/\s*)?\bint\s+" + ENTRY + r"\s*\([^;]*\)\s*;[ \t]*(/\*(?:(?!\*/).)*\*/)?", hdr, flags=re.S)
    assert m, f"{ENTRY} is not declared"
    comment = (m.group(1) or "") + (m.group(2) or "")
    assert "utils/binvox_rw.py:239" in comment and "zero" in comment.lower() and "non-cubic" in comment, comment


def test_exported_and_bound():
    assert ENTRY in hip.EXPORTED_SYMBOLS
    lib = hip.load()                          # dlopen only: no GPU call is made
    assert len(hip._argtypes(ENTRY)) == 12 and lib.sv_binvox_encode.argtypes[7] is ctypes.c_float
    assert lib.sv_binvox_encode.argtypes[9] is ctypes.c_longlong


# fake, suitably aligned device addresses: every call below is refused before anything could read them
VOL, PAIRS, NP = (0x10000 * (i + 1) for i in range(3))


def _args(**over):
    a = dict(vol=VOL, dtype=0, B=2, d0=4, d1=6, d2=10, fix=1, th=-1.0, pairs=PAIRS, cap=240, n_pairs=NP)
    a.update(over)
    return (a["vol"], a["dtype"], a["B"], a["d0"], a["d1"], a["d2"], a["fix"], a["th"], a["pairs"], a["cap"], a["n_pairs"], None)


@pytest.mark.parametrize("what,over", [
    ("vol null", dict(vol=None)),
    ("pairs null", dict(pairs=None)),
    ("n_pairs null", dict(n_pairs=None)),
    ("B = 0", dict(B=0)),
    ("B < 0", dict(B=-3)),
    ("d0 = 0", dict(d0=0)),
    ("d1 < 0", dict(d1=-1)),
    ("d2 = 0", dict(d2=0)),
    ("volume = 2^30", dict(d0=1024, d1=1024, d2=1024, cap=1 << 30)),
    ("volume past 2^31", dict(d0=2048, d1=2048, d2=1024, cap=1 << 32)),
    ("dtype 2", dict(dtype=2)),
    ("dtype -1", dict(dtype=-1)),
    ("threshold 1", dict(th=1.0)),
    ("threshold above 1", dict(th=1.5)),
    ("threshold 0", dict(th=0.0)),
    ("threshold NaN", dict(th=float("nan"))),
    ("threshold with uint8", dict(dtype=1, th=0.5)),
    ("capacity one short", dict(cap=239)),
    ("capacity 0", dict(cap=0)),
])
def test_refusals_before_any_gpu_call(what, over):
    lib = hip.load()
    rc = lib.sv_binvox_encode(*_args(**over))
    assert rc == SV_ERR_INVALID, (what, rc)
    assert ENTRY in lib.sv_last_error().decode(), (what, lib.sv_last_error())


def test_binvox_header_matches_every_fixture():
    for name in CASES:
        raw, _, dims = golden(name)
        _, translate, scale, pos = D.parse_binvox_header(raw)
        assert D.binvox_header(dims, translate, scale) == raw[:pos], name
        if name != "noncubic":
            assert D.binvox_header(dims) == raw[:pos], name
    assert D.binvox_header((4, 6, 10), (-0.5, 0.25, 0.0), 0.75) == b"#binvox 1\ndim 4 6 10\ntranslate -0.5 0.25 0.0\nscale 0.75\ndata\n"
    assert golden("noncubic")[0].startswith(b"#binvox 1\ndim 4 6 10\ntranslate -0.5 0.25 0.0\nscale 0.75\ndata\n")


def test_encode_rejects_cpu_tensors():
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        D.encode_binvox_batch(torch.zeros(1, 4, 4, 4))


@pytest.mark.parametrize("name", CASES)
def test_fixture_reads_back_and_restatement_reproduces_it(name):
    raw, xyz, dims = golden(name)
    got, d, _, _ = OD.read_binvox(raw)
    assert d == dims and np.array_equal(got, xyz)
    assert rle_pairs(file_order(xyz)) == payload_of(raw)


def test_named_cases_hold_their_zero_count_pairs():
    def pairs(name):
        p = np.frombuffer(payload_of(golden(name)[0]), dtype=np.uint8).reshape(-1, 2)
        return len(p), int((p[:, 1] == 0).sum()), p
    n, z, p = pairs("runs255_16")
    assert (n, z) == (23, 4) and p[:7].tolist() == [[0, 255], [0, 0], [1, 255], [1, 255], [1, 0], [0, 255], [0, 0]]
    n, z, _ = pairs("long_exact")
    assert (n, z) == (131, 2)
    n, z, p = pairs("tail255_8")
    assert (n, z) == (3, 0) and p.tolist() == [[0, 255], [0, 2], [1, 255]]       # a last run of exactly 255: no tail flush
    assert pairs("alt8")[:2] == (512, 0) and pairs("full32_holes")[:2] == (131, 0)
    assert pairs("sparse32")[1] >= 1 and pairs("half32")[1] == 0
    # what oracle.data.write_binvox leaves out: it is not the expected value of any encoder test
    raw, xyz, _ = golden("runs255_16")
    assert OD.write_binvox(xyz) != raw and np.array_equal(OD.read_binvox(OD.write_binvox(xyz))[0], xyz)
