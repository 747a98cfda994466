"""The kernels on the value range of a trained or fine-tuned net, not the order-1 values of the synthetic one (inputs, references and
the derivation of every bound: tests/value_range_cases.py; their CPU side: tests/test_value_range_cpu.py).

1. test_epilogue_*: act(fma(x, scale, shift)) (+ residual) of y4_conv2d, element by element against float64, for every dtype,
   activation, store type and tile family -- identity weights make each accumulator an input element.
2. test_fused_kernels_*: the stem / chain / stage / residual-block fusions against the unfused engine, bit for bit, on a weight set
   whose pre-activations reach beyond +-20 (helpers.widen_activations); the unfused engine's taps against the oracle's conv_block.
3. test_decode_nms_*: decode + NMS at saturating logits, through test_gpu_decode_nms._compare.
4. test_block_and_head_grad_on_wide_heads: y4_block_grad / y4_head_grad with the wide heads of loss_cases at the smallest training
   grid of test_gpu_fit_geometry.py, by that file's budget rule.  (The wide loss and loss-gradient fixtures run through the
   parametrised tests of test_gpu_loss.py and test_gpu_fit.py.)

Measured distances of part 1 go to profiles/value_range/epilogue_measured.json: c in c * 2^-24 * max(1, |z|, |want|)."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

import loss_cases as LC
import value_range_cases as V
from helpers import GOLDEN, ROOT, quantize, run_conv_gpu, widen_activations
from test_gpu_conv import TOL

pytestmark = pytest.mark.gpu

# schedule code of y4_conv_tile_desc -> family
FAMILY = {2: "plain", 3: "ring", 4: "ring", 5: "ring", 6: "ring", 7: "ring", 8: "staggered_groups", 9: "pipelined", 10: "producer_consumer",
          12: "staggered", 20: "halo", 21: "halo2", 32: "mfma32"}
HALO = ("halo", "halo2")
# what must have run, per dtype (float32 is built for the plain and ring tiles only; "staggered" runs where it fits, unasserted)
REQUIRED = {"f32": {"builtin", "plain", "ring"},
            "bf16": {"builtin", "plain", "ring", "staggered_groups", "pipelined", "producer_consumer", "halo", "halo2", "mfma32"}}
REQUIRED["f16"] = REQUIRED["bf16"]


def _note(key, value):
    path = os.path.join(ROOT, "profiles", "value_range", "epilogue_measured.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    try:
        with open(path) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
    doc[key] = value
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


@functools.lru_cache(maxsize=None)
def _case(dtype, cout, hw, k):
    from yolo4hip.weights import ConvWeights
    c = V.epilogue_case(dtype, cout, hw, k)
    cw = ConvWeights(w=c["w"], bn=c["bn"])
    scale, shift = cw.scale_shift()                      # exactly the float32 numbers run_conv_gpu hands the kernel
    return c, cw, V.preact64(c["x"], scale, shift)


def _families():
    from yolo4hip import ext
    lib = ext.load()
    fam = {"builtin": [0]}
    for tile in range(1, lib.y4_conv_tile_count() + 1):
        cfg = (C.c_int32 * 6)()
        ext.check(lib.y4_conv_tile_desc(tile, cfg))
        fam.setdefault(FAMILY[cfg[5]], []).append(tile)
    return fam


def _run_matrix(dtype, act, tile, cout, hw, k):
    """out_f32 x residual of one (tile, shape) -> [(label, ok array, c, z, got, want)] or None if the tile refuses the shape"""
    from yolo4hip import ext
    c, cw, z = _case(dtype, cout, hw, k)
    want_act = V.act64(z, act)
    out = []
    for out_f32 in (0, 1):
        for res in (None, c["res"]):
            try:
                got, _ = run_conv_gpu(c["x"], cw, k, 1, act, dtype, residual=res, out_f32=bool(out_f32), tile=tile)
            except ext.Y4Error as e:
                assert e.code == -22                     # the tile does not fit this shape / dtype: refused, not computed wrongly
                if not out:
                    return None
                continue
            store = "f32" if out_f32 else dtype
            ok, dist = V.check_epilogue(got, z, want_act, res, store)
            want = want_act if res is None else want_act + res
            out.append((f"out_f32={out_f32} residual={res is not None}", ok, dist, z, got, want))
    return out


@pytest.mark.parametrize("act", ["mish", "leaky", "linear"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_epilogue_element_by_element(dtype, act):
    """Every tile family's epilogue on the value range of value_range_cases.channel_table, within the derived bound."""
    ran, worst, failures = {}, {}, []
    for fam, tiles in _families().items():
        shapes = [(3, (24, 16))] if fam in HALO else [(1, (16, 16)), (3, (16, 16))]     # (24 x 16: the smallest map the 384- and 192-pixel bands fill)
        for k, hw in shapes:
            done = False
            for tile in tiles if fam != "ring" else sorted(tiles, key=lambda t: t not in (43, 14)):
                for cout in (64, 128, 256):
                    rows = _run_matrix(dtype, act, tile, cout, hw, k)
                    if rows is None:
                        continue
                    for label, ok, dist, z, got, want in rows:
                        ran[fam] = ran.get(fam, 0) + 1
                        worst[fam] = max(worst.get(fam, 0.0), dist)
                        print(f"{dtype} {act} {fam} tile {tile} {k}x{k} cout {cout} {label}: c = {dist:.3f}, {int((~ok).sum())} outside")
                        if not ok.all():
                            i = tuple(np.argwhere(~ok)[0])
                            failures.append(f"{fam} tile {tile} {k}x{k} cout {cout} {label}: {int((~ok).sum())} of {ok.size} outside the bound "
                                            f"(c = {dist:.2f}), first z = {z[i]!r}: got {got[i]!r}, want {want[i]!r}")
                    done = True
                    break
                if done:
                    break
    _note(f"{dtype}_{act}", {"c_per_family": worst, "launches": ran})
    print(dtype, act, "worst c per family:", worst)
    assert not failures, "\n".join(failures)
    assert REQUIRED[dtype] <= set(ran), (REQUIRED[dtype] - set(ran), ran)
    # four store / residual combinations of a 1x1 and a 3x3 conv per family; the halo families are 3x3 kernels with a 16-bit store
    # only (conv_igemm.hip refuses out_f32 for them with -22): with and without residual
    assert all(ran[f] >= (2 if f in HALO else 8) for f in REQUIRED[dtype]), ran


# ---- 2. the fused kernels on a wide-range net
def _wide_engine(size, ncls, n, dtype, seed):
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    ws = widen_activations(W.synth_weights(build_plan(size, ncls), seed), seed)
    eng = Engine(ncls, make_config(size), max_batch=n, dtype=dtype)
    eng.load_weight_blob(W.flatten(ws))
    return ws, W.synth_images(n, size, seed), eng


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype.itemsize == 4 else np.int64) if a.dtype.kind == "f" else a


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("size,n", [(96, 5), (160, 3)])
def test_fused_kernels_bit_identical_on_a_wide_range_net(dtype, size, n):
    """Stem, chain, stage and residual-block fusion (masks 1, 2, 3), one at a time and all together, against the unfused engine: heads,
    the taps each schedule still materialises and the detections as integer bit patterns -- the property of test_gpu_forward.py, on
    pre-activations of which a tenth lie beyond +-20 (asserted without a GPU in test_value_range_cpu.py)."""
    from oracle.forward import conv_block
    from yolo4hip import ext
    from yolo4hip.weights import ConvWeights
    ws, imgs, eng = _wide_engine(size, 3, n, dtype, seed=5)
    heads = eng.forward_heads(imgs)
    assert all(np.isfinite(h).all() for h in heads)
    every = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 19, 21, 23, 29, 35, 36, 37, 43, 57, 58, 89, 91, 93, 94)
    ref = {i: eng.conv_output(i, n) for i in every}
    assert all(np.isfinite(t).all() for t in ref.values())
    assert max(float(np.abs(t).max()) for t in ref.values()) > 60.0          # the widened net, not the synthetic one
    base = eng.predict(imgs, with_indices=True)

    # the unfused engine against the oracle, one conv() unit behind its own previous tap (test_gpu_conv.py's per-element tolerance)
    atol, rtol = TOL[dtype]

    def unit(i, x, k, stride, act, res=None):
        cwq = ConvWeights(w=quantize(ws[i].w, dtype), bn=ws[i].bn)
        want = conv_block(x, cwq, k, stride, act, res)
        err = np.abs(ref[i] - want)
        print(f"conv {i} vs oracle: max err {err.max():.3e}, max |want| {np.abs(want).max():.1f}")
        assert np.all(err <= atol + rtol * np.abs(want)), f"conv {i}: max err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}"
    unit(1, ref[0], 3, 2, "leaky")
    unit(7, np.concatenate([ref[6], ref[2]], axis=-1), 1, 1, "mish")         # the first stage's concat [post conv, route] (custom_layers.py:68)
    unit(12, ref[11], 3, 1, "mish", ref[10])                                  # 3x3 + Add of the first 64-channel block: the trunk is conv 10
    unit(16, np.concatenate([ref[15], ref[9]], axis=-1), 1, 1, "mish")

    def check(taps, what):
        for a, b in zip(heads, eng.forward_heads(imgs)):
            assert np.array_equal(_bits(a), _bits(b)), what
        seen = 0
        for i in taps:
            try:
                got = eng.conv_output(i, n)
            except ext.Y4Error:
                continue                                                     # inside a fused kernel under this schedule: not materialised
            assert np.array_equal(_bits(ref[i]), _bits(got)), (what, i)
            seen += 1
        for a, b in zip(base, eng.predict(imgs, with_indices=True)):
            assert np.array_equal(_bits(a), _bits(b)), what
        return seen

    eng.set_stem_fusion(True)
    assert check((1,), "stem") == 1
    eng.set_stem_fusion(False)
    assert eng.set_chain_fusion(True) == 26
    assert check((2, 3, 4, 7, 9, 10, 11, 12, 13, 16, 19, 21, 35, 36, 37, 43, 57, 58, 89, 91, 93, 94), "chain") == 22
    eng.set_chain_fusion(False)
    assert eng.set_stage_fusion(True) and eng.stage_fusion_active()
    assert check((1, 7, 8, 16, 37), "stage") == 5
    assert not eng.set_stage_fusion(False)
    for mask in (1, 2, 3):
        assert eng.set_res_fusion(True) == 10
        eng.set_res_fusion_mask(mask)
        assert eng.res_fusion_mask() == mask
        assert check((10, 12, 14, 16, 19, 21, 23, 29, 35, 36, 37), f"res mask {mask}") == 11
    eng.set_stem_fusion(True)
    eng.set_chain_fusion(True)
    eng.set_stage_fusion(True)
    assert check(every, "all") >= 8
    eng.close()


# ---- 3. decode and NMS at saturating logits
def _saturating_heads(rng, n, size, ncls, conf=(-40.0, 40.0)):
    """Objectness and class logits uniform over `conf` (beyond +-17 a float32 sigmoid is exactly 0 or 1), xy logits over +-30, tw / th
    over [-12, 8]: boxes from 6e-6 to 3000 anchors wide, all finite."""
    heads = []
    nf = 5 + ncls
    for s in (8, 16, 32):
        g = size // s
        h = np.empty((n, g, g, 3, nf), np.float32)
        h[..., 0:2] = rng.uniform(-30.0, 30.0, size=h[..., 0:2].shape)
        h[..., 2:4] = rng.uniform(-12.0, 8.0, size=h[..., 2:4].shape)
        h[..., 4:] = rng.uniform(conf[0], conf[1], size=h[..., 4:].shape)
        heads.append(h.reshape(n, g, g, 3 * nf))
    return heads


@pytest.mark.parametrize("size,ncls,n", [(96, 4, 2), (160, 3, 3)])
def test_decode_nms_at_saturating_logits(size, ncls, n):
    from test_gpu_decode_nms import _compare, _engine
    cfg, eng = _engine(size, ncls, n)
    rng = np.random.default_rng(size)
    # many scores are exactly 1.0f: the ties are ordered by box index, then class (the oracle's stable order)
    heads = _saturating_heads(rng, n, size, ncls)
    got, ref = _compare(eng, cfg, heads, size, ncls)
    assert np.isfinite(got[0]).all() and (got[1][:, :20] == 1.0).all() and got[3].min() > 20
    # every candidate saturates: all scores are 1.0f, the order is the box index's alone
    heads = _saturating_heads(rng, n, size, ncls, conf=(20.0, 40.0))
    got, ref = _compare(eng, cfg, heads, size, ncls)
    v = int(got[3].min())
    assert v > 0 and all((got[1][b, :got[3][b]] == 1.0).all() for b in range(n))
    # ... and none does: nothing passes, whatever the boxes
    heads = _saturating_heads(rng, n, size, ncls, conf=(-40.0, -20.0))
    got, ref = _compare(eng, cfg, heads, size, ncls)
    assert not got[3].any() and not got[0].any()
    eng.close()


# ---- 4. the block and head gradients on the wide heads
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_block_and_head_grad_on_wide_heads(dtype):
    """After a real forward at (96, 352) -- the smallest grid of test_gpu_fit_geometry.py -- the raw heads are replaced by the wide heads
    of loss_cases (logits to +-40, xy to +-20, wh +-8 about the label) for the case's own labels: dK and the head gradient by that
    file's rule, rel_to_max <= max(4 x d_ref, 1e-6) against float64, whole and tap by tap."""
    import lossgrad_oracle as GO
    from test_gpu_fit_blocks import HEAD_IN
    from test_gpu_fit_geometry import CASES, _block_oracle, _boxes, _forward, _hold_dk, _hold_dw
    from yolo4hip.data import preprocess_true_boxes, records_from_boxes
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    from make_lossgrad_fixtures import check_ties
    hw = (96, 352)
    ncls, n, seed = CASES[hw][:3]
    boxes = _boxes(hw, ncls, n, seed)
    records, _ = records_from_boxes(boxes, hw, LC.ANCHORS, ncls)
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    heads = LC.make_heads(hw, ncls, n, 1, records, wide=True)                # seed 1: the first that passes the generators' tie rules
    assert not check_ties(dict(heads=heads, ncls=ncls, hw=hw), labels, xywh)
    assert max(float(np.abs(h).max()) for h in heads) > 39.0
    c = _forward(hw, dtype, 2)
    eng, w = c["eng"], c["w"]
    assert eng.set_heads(heads) == n
    g64 = GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw, img_weight=w)
    tag = f"wide_heads_96x352_{dtype}"
    dk = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    _hold_dk("block_grad_" + tag, eng, dk.cpu().numpy(), _block_oracle(c, dtype, g64))
    dw = eng.head_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    _hold_dw("head_grad_" + tag, eng, dw.cpu().numpy(), g64, [c["ref"].conv_output(i, n) for i in HEAD_IN])
    eng.close()
    c["ref"].close()
