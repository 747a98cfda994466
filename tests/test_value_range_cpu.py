"""The value-range tests without a GPU (tests/value_range_cases.py): the epilogue inputs cover what they claim to cover, the BN rows
fold to exactly the intended scale and shift, the oracle's own float32 conv_block stays inside the bound the kernels are held to
(so the bound is attainable by float32 arithmetic), and the wide-range weight set of tests/helpers.widen_activations drives the
backbone's pre-activations beyond +-20 while every stored activation stays finite in float16."""
import numpy as np
import pytest

import value_range_cases as V
from helpers import quantize, widen_activations

ACTS = ("mish", "leaky", "linear")


def _case(dtype, cout, hw, k):
    from yolo4hip.weights import ConvWeights
    c = V.epilogue_case(dtype, cout, hw, k)
    cw = ConvWeights(w=c["w"], bn=c["bn"])
    scale, shift = cw.scale_shift()
    return c, cw, scale, shift


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("cout,hw,k", [(64, (16, 16), 1), (128, (24, 16), 3)])
def test_epilogue_inputs_cover_the_value_range(dtype, cout, hw, k):
    c, cw, scale, shift = _case(dtype, cout, hw, k)
    # the operands are what they claim to be: x and the residual representable in the dtype, the fold exact (the sign of -0 included)
    assert np.array_equal(quantize(c["x"], dtype), c["x"]) and np.array_equal(quantize(c["res"], dtype), c["res"])
    assert np.array_equal(scale.view(np.int32), c["bn"][1].view(np.int32))
    assert np.array_equal(shift.view(np.int32), c["bn"][0].view(np.int32))
    assert (scale < 0).sum() >= cout // 4 and (scale > 0).sum() >= cout // 4
    assert np.array_equal(np.einsum("oikl->oi", c["w"]), np.eye(cout, dtype=np.float32)) and np.count_nonzero(c["w"]) == cout
    # channels with a shift: x * scale is exact in float32 (a multiply-then-add and an FMA round alike)
    prod = c["x"].astype(np.float64) * scale.astype(np.float64)
    assert np.array_equal(prod[..., shift != 0], prod[..., shift != 0].astype(np.float32).astype(np.float64))
    z = V.preact64(c["x"], scale, shift)
    assert np.isfinite(z).all()
    cov = V.coverage(z, dtype)
    print(dtype, cout, cov)
    assert cov.pop("dense_bins_of_0.05_on_[-25,25]_hit") >= 1000            # every 0.05-wide bin of [-25, 25]
    assert cov.pop("decades") == (4 if dtype == "f16" else 29)              # 30 .. 3e4, or 30 .. 1e30
    assert all(v >= 1 for v in cov.values()), {k_: v for k_, v in cov.items() if v < 1}
    a = np.abs(z)
    assert a.max() == (65520.0 + 64.0 if dtype == "f16" else float(np.float32(1e30)))   # nothing beyond the intended top


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("cout,hw,k", [(64, (16, 16), 1), (128, (24, 16), 3)])
def test_oracle_float32_conv_block_is_inside_the_epilogue_bound(dtype, cout, hw, k):
    from oracle.forward import conv_block
    c, cw, scale, shift = _case(dtype, cout, hw, k)
    z = V.preact64(c["x"], scale, shift)
    for act in ACTS:
        want = V.act64(z, act)
        for res in (None, c["res"]):
            got = conv_block(c["x"], cw, k, 1, None if act == "linear" else act, res)
            ok, dist = V.check_epilogue(got, z, want, res, "f32")
            print(dtype, cout, act, "residual" if res is not None else "plain", f"c = {dist:.2f}")
            assert ok.all(), (act, int((~ok).sum()), z[~ok][:4], got[~ok][:4], want[~ok][:4])


def test_bound_helpers():
    # half a spacing of the storage types, at normal, subnormal and power-of-two magnitudes
    assert V.storage_half_spacing(np.array([1.0, 1.5, 2.0, 65504.0, 2.0 ** -20]), "f16").tolist() == \
        [2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 16.0, 2.0 ** -25]
    assert V.storage_half_spacing(np.array([1.0, 3.0e30]), "bf16").tolist() == [2.0 ** -8, 2.0 ** (101 - 8)]
    assert not V.storage_half_spacing(np.array([7.0]), "f32").any()
    # beyond the float16 range only the signed infinity or the signed largest value pass; inside it the bound decides
    z = np.array([7.0e4, -7.0e4, 7.0e4, 7.0e4, 7.0e4, 100.0, 100.0])
    got = np.array([np.inf, -65504.0, -np.inf, 65472.0, np.nan, 100.03125, 100.125])
    ok, _ = V.check_epilogue(got, z, z, None, "f16")
    assert ok.tolist() == [True, True, False, False, False, True, False]
    ok, _ = V.check_epilogue(np.array([np.inf, np.nan, 1.0e30]), np.full(3, 1.0e30), np.full(3, 1.0e30), None, "f32")
    assert ok.tolist() == [False, False, True]
    assert np.array_equal(V.act64(np.array([-800.0, 0.0, 800.0]), "mish"), [-0.0, 0.0, 800.0])


@pytest.fixture(scope="module")
def wide_net():
    """The wide-range net at 96 x 96, 3 classes, 5 images: float32 pre-activations, and the 16-bit storage emulations' taps."""
    from oracle.forward import yolo_model_forward
    from yolo4hip import weights as W
    from yolo4hip.plan import build_plan
    size, ncls, n, seed = 96, 3, 5, 5
    base = W.synth_weights(build_plan(size, ncls), seed)
    wide = widen_activations(base, seed)
    imgs = W.synth_images(n, size, seed)
    pre = {}
    heads, _ = yolo_model_forward(imgs, wide, ncls, collect=range(110), pre=pre)
    stored = {st: yolo_model_forward(imgs, wide, ncls, collect=range(110), storage=st) for st in ("bf16", "f16")}
    return base, wide, pre, heads, stored


def test_widen_activations_changes_only_gamma_and_beta(wide_net):
    base, wide, _, _, _ = wide_net
    assert len(base) == len(wide) == 110
    negative = 0
    for i, (a, b) in enumerate(zip(base, wide)):
        assert a.w is b.w
        if a.bn is None:
            assert b is a
            continue
        assert np.array_equal(a.bn[2:], b.bn[2:]) and not np.array_equal(a.bn[:2], b.bn[:2]), i
        negative += int((b.bn[1] < 0).sum())
        assert (b.bn[1] < 0).any() == (i not in (92, 100, 108)), i
    assert negative > 1000
    again = widen_activations(base, 5)
    assert all(np.array_equal(x.bn, y.bn) for x, y in zip(wide, again) if x.bn is not None)


def test_wide_net_reaches_beyond_20_and_stays_finite_in_float16(wide_net):
    _, _, pre, heads, stored = wide_net
    # The pre-activations the fused kernels' epilogues see: each listed conv's own, and those of the conv that feeds it
    # (0..37 covers both readings of "at the inputs of convs 1, 2..7, 11..14, 20..36")
    assert set(V.WIDE_INPUT_CONVS) | {i - 1 for i in V.WIDE_INPUT_CONVS} <= set(range(38))
    for i in range(38):
        z = pre[i]
        hi, lo = float((z > 20.0).mean()), float((z < -20.0).mean())
        assert hi >= 0.01 and lo >= 0.01, (i, hi, lo)
    for i in (60, 80, 91, 99, 107):                                          # ... and the neck's
        assert (pre[i] > 20.0).mean() >= 0.01 and (pre[i] < -20.0).mean() >= 0.01, i
    assert all(np.isfinite(h).all() for h in heads)
    for st, (h16, taps) in stored.items():
        top = max(float(np.abs(t).max()) for t in taps.values())
        print(st, "largest stored activation", top, "largest head logit", max(float(np.abs(h).max()) for h in h16))
        assert top < V.WIDE_MAX_STORED, (st, top)
        assert len(taps) > 110 and all(np.isfinite(t).all() for t in taps.values())
        assert all(np.isfinite(h).all() and np.abs(h).max() < 100.0 for h in h16)
