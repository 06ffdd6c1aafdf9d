"""Characterization of the host path of Decoder, Merger, Refiner and Encoder (the conv / BatchNorm layer chains, the ResNet trunk, the Swin
neck, cross-view attention, the fusion head and the stream forks, joins and weight-gradient-stream launches): every case of
tests/golden/make_module_host_trace.py issues exactly the library calls - entry points, scalars, WHICH buffer goes to which pointer argument -
and the stream operations (on WHICH stream each launch is enqueued, relative to the waits and records) that the fixture recorded from the code
whose behaviour is kept.  CPU tensors, recorder in place of call / ptr, stand-ins for the torch stream names: no GPU call is made."""
import importlib.util
import json
import os

import pytest

from swinvox_amd import hip

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_module_host_trace", os.path.join(HERE, "golden", "make_module_host_trace.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

pytestmark = pytest.mark.skipif(not os.path.exists(hip.LIB_PATH), reason="the library is not built: its *_supported queries decide the paths")


@pytest.fixture(scope="module")
def traced():
    before = gen.snapshot()
    traces = gen.trace_all()
    assert before == gen.snapshot()             # every replaced function, switch, stream cache and environment variable is back
    assert gen.trace_all() == traces            # every case twice: nothing depends on addresses or on what an earlier case left behind
    return gen.split(traces)


@pytest.fixture(scope="module")
def golden():
    with open(gen.FIXTURE) as f:
        return json.load(f)


def test_tail_modules_issue_the_recorded_calls(traced, golden):
    tail, fx = traced[0], golden["tail"]
    assert gen.sha1(list(tail)) == fx["names"] and len(tail) == len(fx["cases"])
    for (name, trace), k in zip(tail.items(), fx["cases"]):
        for i, (got, exp) in enumerate(zip(trace, fx["traces"].get(str(k), []))):     # the traces kept in full: the first record that differs
            assert got == exp, f"{name}: record {i}"
        assert gen.sha1(trace) == fx["sha1"][k], f"{name}: {len(trace)} records, {[c[0] for c in trace]}"


def test_encoder_issues_the_recorded_calls_on_the_recorded_streams(traced, golden):
    enc, fx = traced[1], golden["encoder"]
    assert gen.sha1(list(enc)) == fx["names"] and len(enc) == len(fx["cases"])
    for (name, trace), k in zip(enc.items(), fx["cases"]):
        want = [fx["entries"][gen.ALPHABET.index(ch)] for ch in fx["sequences"][k]]
        for i, (got, exp) in enumerate(zip(trace, want)):                            # the first record whose head differs
            assert got[0] == exp, f"{name}: record {i} is {got}, the fixture has {exp} there"
        assert len(trace) == len(want), f"{name}: {len(trace)} records, the fixture has {len(want)}"
        assert gen.sha1(trace) == fx["sha1"][k], f"{name}: the same {len(trace)} record heads, but an argument, a buffer or a stream differs"


def test_fixture_covers_the_cases_and_the_path(traced, golden):
    tail, enc = traced
    t, e = golden["tail"], golden["encoder"]
    assert len(t["cases"]) == 16 + 24 + 32 and len(e["cases"]) == 27
    for fx in (t, e):
        assert len(set(fx["sha1"])) == len(fx["sha1"]) and sorted(set(fx["cases"])) == list(range(len(fx["sha1"])))
    assert all(gen.sha1(tr) == t["sha1"][int(k)] for k, tr in t["traces"].items())
    assert {c[0] for tr in t["traces"].values() for c in tr} == {c[0] for tr in tail.values() for c in tr}
    assert set(e["entries"]) == {c[0] for tr in enc.values() for c in tr}
    assert {"@wait_stream", "@wait_event", "@record", "@enter", "@exit", "@record_stream", "@hook", "sv_pack_weights", "sv_linear_mxfp8_wgrad",
            "sv_quant_rows_cols_mx_e4m3", "sv_bn_maxpool_bwd", "sv_bn_bwd2_signs", "sv_encoder_prep_bwd", "sv_stem_space_to_depth"} <= set(e["entries"])
    assert {"@enter", "@wait_stream", "sv_stencil3_fwd", "sv_stencil3_wgrad", "sv_bn_maxpool3d_bwd", "sv_maxpool3d_bwd", "sv_head_unpack_dx",
            "sv_decoder_head_bwd", "sv_merge_views_bwd"} <= {c[0] for tr in t["traces"].values() for c in tr}


def test_streams_of_a_case_are_numbered_by_first_appearance(traced):
    """the default Encoder case opens with the fork (the side stream, s0, waits for the main stream, s1); @enter / @exit nest and balance"""
    trace = traced[1]["encoder"]
    assert trace[[c[0][0] for c in trace].index("@")] == ["@wait_stream", "s0", "s1"]
    depth = 0
    for c in trace:
        depth += {"@enter": 1, "@exit": -1}.get(c[0], 0)
        assert depth >= 0
    assert depth == 0 and trace[-1][0] == "@wait_stream"           # the weight-gradient stream is joined last
