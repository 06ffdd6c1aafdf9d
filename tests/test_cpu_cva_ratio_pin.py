"""The oracle's CrossViewAttention at ATT_SPATIAL_DOWNSAMPLE_RATIO 4 and 7 (1x1 token grid) against the reference module: forward in
eval and train mode and every gradient, V in {1, 3}, (CROSS_ATT_REDUCTION_RATIO, CROSS_ATT_NUM_HEADS) in {(4, 4), (2, 2), (8, 8)},
recorded by tests/golden/make_cva_ratio_ge4_pin.py.  The GPU tests (tests/test_gpu_cva_ratio.py) check the HIP path against the
oracle, so this pin is what ties them to the reference."""
import json
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _pin():
    return json.load(open(os.path.join(GOLD, "cva_ratio_ge4_pin.json")))


def test_cva_ratio_ge4_oracle_matches_the_reference():
    pins = _pin()["pins"]
    expected = {f"cva_ds{r}_red{red}_h{h}_V{V}_{mode}_fwd_bwd_maxdiff"
                for r in (4, 7) for red, h in ((4, 4), (2, 2), (8, 8)) for V in (1, 3) for mode in ("eval", "train")}
    assert set(pins) == expected
    for k, v in pins.items():
        assert 0.0 <= v <= 1e-6, (k, v)


def test_cva_ratio_8_fails_in_both():
    assert _pin()["ratio8_raises"] == {"oracle": True, "reference": True}


def test_oracle_runs_every_built_ratio():
    """The oracle is general in the ratio: ratios 4 ... 7 all give a 1x1 grid and run forward + backward on CPU."""
    import torch
    import oracle as O
    for r in (4, 5, 6, 7):
        cfg = O.default_cfg()
        cfg.NETWORK.ATT_SPATIAL_DOWNSAMPLE_RATIO = r
        m = O.CrossViewAttention(cfg, 512)
        assert tuple(m.downsample_qkv.weight.shape) == (512, 1, r, r)
        x = torch.randn(1, 2, 512, 7, 7, requires_grad=True)
        y = m(x)
        y.sum().backward()
        assert y.shape == x.shape and bool(torch.isfinite(x.grad).all())
