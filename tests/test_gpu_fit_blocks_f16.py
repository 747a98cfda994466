"""fit(trainable='head_blocks') on an f16 model: y4_block_grad_scaled (csrc/block_train.hip: the loss scale S applied to dZ before
its rounding to fp16, 1 / S to the float32 sum, the overflow word), y4_block_adam on an f16 handle, and the loss-scale policy in
Yolov4.fit -- against the float64 restatement of tests/blockgrad_oracle.py, and against itself.

Budget of every comparison with a float64 value: the rule of tests/test_gpu_fit.py, rel_to_max <= max(4 x d_ref, 1e-6), d_ref from
the oracle alone: the distance of the float64 oracle with dZ rounded as (dZ * S -> np.float16 -> / S) from the unrounded one.  It
is evaluated twice, once keeping fp16's subnormals and once flushing them to zero, and the LARGER distance is d_ref: what the
device does with subnormals is asserted nowhere.  S is chosen from the oracle alone: per scale the power of two that puts the
oracle's max |dZ| * S in [2^12, 2^13), and the smallest of the three serves the call.  At that S the two evaluations agree to four
digits.  Every distance goes to profiles/fit/parity_measured.json beside its budget.

A scale that is too large is an arithmetic overflow to inf in a buffer of fixed size; the kernel reports it in the overflow word."""
import os

import numpy as np
import pytest

import blockgrad_oracle as BO
import loss_cases as LC
import lossgrad_oracle as GO
from helpers import CLASS_DIR
from test_gpu_fit import _bits, _engine, _facade, _note, _within
from test_gpu_fit_blocks import BLOCK_IN, HEAD_IN, RATE, _adam32, _layer_params, _unpack_k
from test_gpu_fit_geometry import CHANNELS, _boxes, _scratch_bytes, geometries, grids, reached
from test_loss_cpu import _write_dataset

pytestmark = pytest.mark.gpu
WEIGHTS = np.array([0.4, 0.1, 0.3, 0.2], np.float32)
# hw -> classes, images, seed, boxes, [(scale, path of blockgrad_oracle.wgrad_branches)] the case is there for
CASES = {
    (160, 160): (3, 4, 9, LC.make_boxes, []),
    (96, 160): (3, 4, 14, LC.make_boxes, []),
    (96, 416): (80, 2, 22, _boxes, [(0, "R2_fall_back"), (0, "Wp_above_W"), (1, "R4"), (2, "odd_W_pair")]),
    (96, 608): (3, 3, 23, _boxes, [(0, "R2_wide_start"), (0, "lds_above_64k"), (1, "R4_last_strip_partial")]),
}
SHIFT = 24           # test 2: the image weights are multiplied by 2^-SHIFT (verified on the CPU oracle with storage='f16': d_ref at
#                      scale 1 is 0.33 .. 0.45 with subnormals kept and 1.0 with them flushed, against 8.4e-5 .. 1.7e-4 at S_good)


def round_f16(scale, keep_subnormals):
    """round_dz of blockgrad_oracle.block_grad: dZ * scale -> fp16 (nearest even) -> / scale, subnormal results kept or flushed"""
    def rnd(dz):
        with np.errstate(over="ignore"):
            y = (np.asarray(dz, np.float64) * scale).astype(np.float16)
        if not keep_subnormals:
            y = np.where(np.abs(y) < np.float16(2.0 ** -14), np.float16(0), y)
        return y.astype(np.float64) / scale
    return rnd


def scale_for(max_dz, lo_exp):
    """the power of two S with max_dz * S in [2^lo_exp, 2^(lo_exp + 1))"""
    return 2.0 ** (lo_exp - int(np.floor(np.log2(max_dz))))


def _forward(hw):
    """Two f16 engines after a forward of the case's batch: the one under test (aliased workspace, fused chains, level 2) and the
    non-aliased unfused one that supplies U and A.  -> dict; oracle(w) evaluates the float64 side for image weights w."""
    import torch
    from yolo4hip.data import preprocess_true_boxes
    ncls, n, seed, make, _ = CASES[hw]
    eng, flat = _engine(hw, ncls, n, "f16", alias_workspace=True, retain_head_inputs=2)
    ref, _ = _engine(hw, ncls, n, "f16")
    assert eng.set_chain_fusion(True) > 0
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + tuple(hw) + (3,)).astype(np.float32)).to(eng.device)
    boxes = make(hw, ncls, n, seed)
    eng.forward_device(imgs)
    ref.forward_device(imgs)
    heads = [h.cpu().numpy() for h in eng.heads_device(n)]
    for a, b in zip(heads, ref.heads_device(n)):
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    U = [ref.conv_output(c, n) for c in BLOCK_IN]
    A = [ref.conv_output(c, n) for c in HEAD_IN]
    ref.close()
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    params = []
    for wh, _, _, bn in _layer_params(eng, flat, "f16"):
        params.append((wh.astype(np.float16).astype(np.float64), BO.bn_scale(bn[1], bn[3])))      # Wh as the f16 handle packs it

    def oracle(w):
        """-> per scale (g64, dZ64, dK64)"""
        g64 = GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw, img_weight=w)
        out = []
        for s, (wh, sc) in enumerate(params):
            dz = BO.block_dz(g64[s], wh, A[s], sc)
            out.append((g64[s], dz, BO.block_wgrad(dz, U[s])))
        return out

    def rounded(orc, scale):
        """-> per scale (dK64, [dK with dZ rounded at `scale`, subnormals kept; the same, flushed])"""
        return [(dk64, [BO.block_grad(g, wh, A[s], U[s], sc, round_dz=round_f16(scale, keep)) for keep in (True, False)])
                for s, ((g, _, dk64), (wh, sc)) in enumerate(zip(orc, params))]
    return dict(eng=eng, flat=flat, imgs=imgs, boxes_dev=torch.from_numpy(boxes).to(eng.device), ncls=ncls, n=n, w=WEIGHTS[:n].copy(),
                oracle=oracle, rounded=rounded, torch=torch, hw=hw)


def _d_ref(others, want):
    return max(GO.rel_to_max(o, want) for o in others)


def _hold_dk(tag, eng, dk, oracle):
    """dK of the three scales against the oracle, as a whole and tap by tap (the rule of test_gpu_fit_geometry._hold_dk), d_ref
    the larger of the two subnormal treatments"""
    for s, (got, (want, others)) in enumerate(zip(_unpack_k(eng, dk), oracle)):
        assert got.shape == want.shape and np.abs(want).max() > 0
        _within(f"{tag}_scale{s}_dK", got, want, _d_ref(others, want))
        for kh in range(3):
            for kw in range(3):
                t = want[:, :, kh, kw]
                assert np.abs(t).max() > 0
                _within(f"{tag}_scale{s}_dK_tap{kh}{kw}", got[:, :, kh, kw], t, _d_ref([o[:, :, kh, kw] for o in others], t))


def _word(t):
    return int(t.cpu().numpy()[0])


@pytest.fixture(scope="module")
def small():
    """(96, 160) after a forward, its oracle at the call's S_good, and the device gradient at S_good: shared by tests 1, 2, 3"""
    c = _forward((96, 160))
    orc = c["oracle"](c["w"])
    c["max_dz"] = [float(np.abs(dz).max()) for _, dz, _ in orc]
    c["s_good"] = min(scale_for(m, 12) for m in c["max_dz"])
    c["at_good"] = c["rounded"](orc, c["s_good"])
    c["dk_good"], c["word_good"] = c["eng"].block_grad_device(c["n"], boxes_dev=c["boxes_dev"], img_weight=c["w"], loss_scale=c["s_good"])
    yield c
    c["eng"].close()


# ---- 1. the scaled gradient after a real forward
@pytest.mark.parametrize("hw", list(CASES), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_block_grad_scaled_f16_after_a_forward(hw, request):
    shared = hw == (96, 160)
    c = request.getfixturevalue("small") if shared else _forward(hw)
    eng, n, w, torch = c["eng"], c["n"], c["w"], c["torch"]
    geo, hit = geometries(hw, "bf16", n), reached(hw, "bf16", n)            # the geometry of fp16 is the bf16 one
    print("reaches:", hit)
    assert set(CASES[hw][4]) <= set(hit), (CASES[hw][4], hit)
    for m in sorted({1, n - 1, n}):
        assert _scratch_bytes(eng, m) == BO.scratch_bytes("bf16", m, grids(hw), CHANNELS), m
    if shared:
        s_good, oracle, dk, word = c["s_good"], c["at_good"], c["dk_good"], c["word_good"]
        max_dz = c["max_dz"]
    else:
        orc = c["oracle"](w)
        max_dz = [float(np.abs(dz).max()) for _, dz, _ in orc]
        s_good = min(scale_for(m, 12) for m in max_dz)
        oracle = c["rounded"](orc, s_good)
        dk, word = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=s_good)
    tag = f"block_grad_scaled_{hw[0]}x{hw[1]}_c{c['ncls']}_f16"
    _note(tag + "_scale", {"max_abs_dZ": max_dz, "log2_S": float(np.log2(s_good)), "lds_bytes": [g["lds_bytes"] for g in geo],
                           "d_ref_kept_vs_flushed": [[GO.rel_to_max(o, want) for o in others] for want, others in oracle]})
    assert 2.0 ** 12 <= max(max_dz) * s_good < 2.0 ** 13
    assert word.dtype == torch.int32 and _word(word) == 0
    _hold_dk(tag, eng, dk.cpu().numpy(), oracle)
    again, word2 = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=s_good)
    assert np.array_equal(_bits([dk])[0], _bits([again])[0]) and _word(word2) == 0

    # two accumulated calls of unequal size into one overflow word: one image, then the rest
    def chunked():
        acc = torch.empty_like(dk)
        flag = torch.zeros((1,), dtype=torch.int32, device=eng.device)
        w_dev = torch.from_numpy(w).to(eng.device)
        for i0, i1 in ((0, 1), (1, n)):
            eng.forward_device(c["imgs"][i0:i1])
            _, back = eng.block_grad_device(i1 - i0, boxes_dev=c["boxes_dev"][i0:i1], img_weight=w_dev[i0:i1], dk=acc, accumulate=i0 > 0,
                                            loss_scale=s_good, overflow=flag)
            assert back is flag
        assert _word(flag) == 0
        return acc.cpu().numpy()
    two = chunked()
    assert np.array_equal(two.view(np.int32), chunked().view(np.int32))
    _hold_dk(tag + "_chunks", eng, two, oracle)
    eng.forward_device(c["imgs"])                                           # (the shared engine holds the whole batch again)
    if not shared:
        eng.close()


# ---- 2. the scale is applied before the rounding
def test_the_scale_is_applied_before_the_rounding(small):
    c = small
    eng, n = c["eng"], c["n"]
    eng.forward_device(c["imgs"])
    w = (c["w"] * np.float32(2.0 ** -SHIFT)).astype(np.float32)
    orc = c["oracle"](w)
    max_dz = [float(np.abs(dz).max()) for _, dz, _ in orc]
    s_good = min(scale_for(m, 12) for m in max_dz)
    good, one = c["rounded"](orc, s_good), c["rounded"](orc, 1.0)
    # a condition on the inputs, from the oracle alone: at scale 1 the rounding destroys the gradient under either treatment
    for s in range(3):
        for keep in (0, 1):
            d1, dg = GO.rel_to_max(one[s][1][keep], one[s][0]), GO.rel_to_max(good[s][1][keep], good[s][0])
            print(f"scale {s} subnormals {'kept' if keep == 0 else 'flushed'}: d_ref(S=1) {d1}, d_ref(S_good) {dg}")
            assert d1 >= 10.0 * dg, (s, keep, d1, dg)
    _note("block_grad_scaled_shift", {"shift_log2": -SHIFT, "max_abs_dZ": max_dz, "log2_S_good": float(np.log2(s_good)),
                                      "d_ref_S1_kept_vs_flushed": [[GO.rel_to_max(o, want) for o in others] for want, others in one]})
    dk, word = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=s_good)
    assert _word(word) == 0
    # a kernel that drops the scale, or applies it after the rounding, lands near d_ref(S=1)
    _hold_dk(f"block_grad_scaled_96x160_c3_f16_shift{SHIFT}", eng, dk.cpu().numpy(), good)


# ---- 3. a scale that is too large is reported
def test_overflow_is_flagged_not_hidden(small):
    c = small
    eng, n, w, torch = c["eng"], c["n"], c["w"], c["torch"]
    eng.forward_device(c["imgs"])
    s_over = scale_for(max(c["max_dz"]), 18)
    assert max(c["max_dz"]) * s_over >= 2.0 ** 18 > 65504.0
    _, word = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=s_over)
    assert _word(word) & 1
    dk, word = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=c["s_good"])
    assert _word(word) == 0
    assert np.array_equal(_bits([dk])[0], _bits([c["dk_good"]])[0])
    held = torch.ones((1,), dtype=torch.int32, device=eng.device)
    dk, back = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=c["s_good"], overflow=held)
    assert back is held and _word(held) == 1                                # ORed into, never cleared
    assert np.array_equal(_bits([dk])[0], _bits([c["dk_good"]])[0])


# ---- 4. refusals
def _scaled_raw(eng, n, triple, w, scale, word, dk, accumulate=False):
    """y4_block_grad_scaled through ctypes, so that the word may be null -> the return code"""
    from yolo4hip import ext
    rec, cnt, xywh = triple
    scratch = eng._group_scratch("blocks", n)
    with eng.torch.cuda.device(eng.device):
        return eng.lib.y4_block_grad_scaled(eng.handle, n, ext.ptr(rec), ext.ptr(cnt), ext.ptr(xywh), eng._loss_max_boxes(), 0.5,
                                            ext.ptr(w), float(scale), ext.ptr(word), ext.ptr(scratch), scratch.numel(), ext.ptr(dk),
                                            dk.numel(), 1 if accumulate else 0, ext.stream_ptr())


def test_scaled_entry_refusals(small):
    from yolo4hip import ext
    c = small
    eng, n, torch = c["eng"], c["n"], c["torch"]
    eng.forward_device(c["imgs"])
    triple = eng.assign_device(c["boxes_dev"])
    w = torch.from_numpy(c["w"]).to(eng.device)
    dk = torch.empty((eng.block_floats(),), dtype=torch.float32, device=eng.device)
    word = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    for bad in (3.0, 1000.0, 0.0, -2.0, float("inf"), float("nan")):
        assert _scaled_raw(eng, n, triple, w, bad, word, dk) == -22, bad
        assert b"power of two" in eng.lib.y4_last_error()
    assert _scaled_raw(eng, n, triple, w, 256.0, None, dk) == -22 and b"overflow word" in eng.lib.y4_last_error()
    assert _word(word) == 0
    with pytest.raises(ext.Y4Error) as err:                                 # the unscaled entry still refuses f16, and says where to go
        eng.block_grad_device(n, records=triple, img_weight=w)
    assert err.value.code == -22 and "f16" in str(err.value) and "y4_block_grad_scaled" in str(err.value)
    assert _scaled_raw(eng, n, triple, w, 256.0, word, dk) == 0 and _word(word) == 0
    # level 1
    one, _ = _engine((96, 160), 3, n, "f16", alias_workspace=True, retain_head_inputs=1)
    one.forward_device(c["imgs"])
    with pytest.raises(ext.Y4Error) as err:
        one.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w, loss_scale=256.0)
    assert err.value.code == -1 and "retention level" in str(err.value)
    one.close()
    # the width limit is the bf16 one: 200 cells answer, 204 do not (queries only)
    for width, ok in ((1600, True), (1632, False)):
        hw = (96, width)
        wide, _ = _engine(hw, 3, 1, "f16", alias_workspace=True, retain_head_inputs=2)
        if ok:
            assert _scratch_bytes(wide, 1) == BO.scratch_bytes("bf16", 1, grids(hw), CHANNELS)
        else:
            assert BO.scratch_bytes("bf16", 1, grids(hw), CHANNELS) is None
            with pytest.raises(ext.Y4Error) as err:
                _scratch_bytes(wide, 1)
            assert err.value.code == -22 and "grid row of 204 cells" in str(err.value)
        wide.close()


# ---- 5. a power-of-two scale is exact where the operand type has the range
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_power_of_two_scale_changes_no_bit_on_f32_and_bf16(dtype):
    import torch
    hw, ncls, n = (96, 160), 3, 4
    eng, _ = _engine(hw, ncls, n, dtype, alias_workspace=True, retain_head_inputs=2)
    if dtype != "f32":
        assert eng.set_chain_fusion(True) > 0
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + hw + (3,)).astype(np.float32)).to(eng.device)
    boxes_dev = torch.from_numpy(LC.make_boxes(hw, ncls, n, seed=14)).to(eng.device)
    w = torch.from_numpy(WEIGHTS).to(eng.device)

    def run(scale, word):
        """the whole batch in one call, and two accumulated chunks -> (bits, bits)"""
        out = []
        for parts in (((0, n),), ((0, 1), (1, n))):
            dk = torch.empty((eng.block_floats(),), dtype=torch.float32, device=eng.device)
            for i0, i1 in parts:
                eng.forward_device(imgs[i0:i1])
                triple = eng.assign_device(boxes_dev[i0:i1])
                if scale is None:
                    eng.block_grad_device(i1 - i0, records=triple, img_weight=w[i0:i1], dk=dk, accumulate=i0 > 0)
                else:
                    assert _scaled_raw(eng, i1 - i0, triple, w[i0:i1], scale, word, dk, i0 > 0) == 0, eng.lib.y4_last_error()
            out.append(_bits([dk])[0])
        return out
    plain = run(None, None)
    assert np.abs(plain[0].view(np.float32)).max() > 0
    word = torch.zeros((1,), dtype=torch.int32, device=eng.device)
    for scale, flag in ((1.0, None), (1.0, word), (2.0 ** 10, None), (2.0 ** 10, word)):
        for a, b in zip(plain, run(scale, flag)):
            diff = int((a != b).sum())
            print(f"{dtype} scale {scale} word {'given' if flag is not None else 'null'}: {diff} of {a.size} elements differ")
            assert diff == 0
    assert _word(word) == 0
    eng.close()


# ---- 6. Adam and the re-pack on an f16 handle
def test_block_adam_steps_and_repack_f16():
    import torch
    hw, ncls, n, dtype = (160, 160), 3, 2, "f16"
    eng, flat = _engine(hw, ncls, n, dtype)
    state = eng.block_state(flat)
    count = eng.block_floats()
    assert count == sum(k for _, k in eng.block_records()) == state["w"].numel()
    rng = np.random.default_rng(8)
    w, m, v = state["w"].cpu().numpy().copy(), np.zeros(count, np.float32), np.zeros(count, np.float32)
    for t in range(1, 4):
        g = (rng.normal(size=count) * 10.0 ** rng.integers(-3, 1, size=count)).astype(np.float32)
        eng.block_adam_step(state, torch.from_numpy(g).to(eng.device), lr=1e-3)
        w, m, v = _adam32(w, m, v, g, t, 1e-3)
    assert state["t"] == 3
    for name, want in (("w", w), ("m", m), ("v", v)):
        got = state[name].cpu().numpy()
        diff = int((got.view(np.int32) != want.view(np.int32)).sum())
        print(f"adam {dtype} {name}: {diff} of {count} elements differ from the NumPy float32 restatement")
        assert diff == 0, (name, diff)
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + hw + (3,)).astype(np.float32)).to(eng.device)
    new_flat = eng.block_weights_to_flat(state, flat.copy())
    changed = np.flatnonzero(new_flat != flat)
    inside = np.zeros(flat.size, bool)
    for o, k in eng.block_records():
        inside[o:o + k] = True
    assert changed.size and inside[changed].all()
    fresh, _ = _engine(hw, ncls, n, dtype)
    fresh.load_weight_blob(new_flat)
    assert np.array_equal(eng.wts.cpu().numpy(), fresh.wts.cpu().numpy())
    eng.forward_device(imgs)
    fresh.forward_device(imgs)
    for a, b in zip(_bits(eng.heads_device(n)), _bits(fresh.heads_device(n))):
        assert np.array_equal(a, b)
    eng.close()
    fresh.close()


# ---- 7. fit with a static scale
# The static scale of the end-to-end run: the largest power of two S for which the run at 16 S still skips no step, so that a
# gradient sixteen times as large as any of these twelve steps' still fits fp16.  Measured once on an MI355X with this file's _fit
# (profiles/fit/parity_measured.json, "fit_head_blocks_f16_scale_sweep"): 2^6 .. 2^11 skip nothing, 2^12 skips one step per epoch,
# 2^13 and above skip all twelve.  16 S = 2^11, S = 2^7.
STATIC_SCALE = 2.0 ** 7


def _fit(tmp_path, trainable, epochs=4, loss_scale=None, images=7):
    from yolo4hip.data import DataGenerator
    m = _facade((160, 160), "f16", max_batch=2)                             # batches of 3 through max_batch 2: two chunks
    sizes = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64), (128, 96), (160, 120)][:images]
    lines = _write_dataset(tmp_path, sizes, [3, 0, 5, 8, 1, 4, 2][:images])
    gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=False, config=m.config)
    before_flat = m._flat.copy()
    np.random.seed(11)
    kw = {} if loss_scale is None else {"loss_scale": loss_scale}
    hist = m.fit(gen, epochs, trainable=trainable, learning_rate=RATE, **kw)
    return m, gen, before_flat, hist


def test_fit_head_blocks_f16_static_scale(tmp_path):
    for d in "abc":
        (tmp_path / d).mkdir()
    m, gen, before_flat, hist = _fit(tmp_path / "a", "head_blocks", loss_scale=STATIC_SCALE)
    m2, _, _, hist2 = _fit(tmp_path / "b", "head_blocks", loss_scale=STATIC_SCALE)
    mh, _, _, hist_h = _fit(tmp_path / "c", "heads")
    loss = hist.history["loss"]
    print(f"fit head_blocks f16 at scale {STATIC_SCALE}: history {hist.history}; heads only {hist_h.history['loss']}")
    _note("fit_head_blocks_f16", {"history": loss, "heads_only_history": hist_h.history["loss"], "loss_scale": STATIC_SCALE})
    assert len(loss) == 4 and np.isfinite(loss).all()
    assert all(b < a for a, b in zip(loss, loss[1:]))                        # the training loss falls over the epochs
    assert loss[-1] < hist_h.history["loss"][-1]                             # and further than with the heads alone
    assert hist.history["skipped_steps"] == [0, 0, 0, 0] and hist.history["loss_scale"] == [STATIC_SCALE] * 4
    assert set(hist_h.history) == {"loss"}                                   # the two keys only where a scale is in use
    assert hist.history == hist2.history
    assert np.array_equal(m._flat.view(np.int32), m2._flat.view(np.int32))
    # only the six trained records moved; the BatchNormalization vectors of convs 92 / 100 / 108 did not
    inside = np.zeros(m._flat.size, bool)
    for o, k in m.engine.head_records() + m.engine.block_records():
        inside[o:o + k] = True
    changed = m._flat.view(np.int32) != before_flat.view(np.int32)
    assert not changed[~inside].any()
    for o, k in m.engine.block_records():
        assert changed[o:o + k].any()
    lt = m.engine.layer_table()
    for c in m.engine.BLOCK_CONVS:
        o = lt[c]["weight_offset"]
        assert not changed[o:o + 4 * lt[c]["cout"]].any()
    # a checkpoint reproduces predict bit for bit
    imgs = np.random.default_rng(6).uniform(0, 1, size=(2, 160, 160, 3)).astype(np.float32)
    heads = m.yolo_model.predict(imgs)
    path = str(tmp_path / "trained.ckpt")
    m.save_model(path)
    fresh = _facade((160, 160), "f16", max_batch=2)
    fresh.load_model(path)
    assert np.array_equal(fresh._flat.view(np.int32), m._flat.view(np.int32))
    for a, b in zip(heads, fresh.yolo_model.predict(imgs)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for a, b in zip(m.engine.predict(imgs, iou_threshold=0.413, score_threshold=0.3), fresh.inference_model.predict(imgs)):
        assert np.array_equal(a, b)
    # a later fit starts from the trained weights
    again = m.fit(gen, 1, trainable="head_blocks", learning_rate=RATE, loss_scale=STATIC_SCALE)
    assert again.history["loss"][0] < loss[0]
    # what has nothing to scale refuses the argument; no scale on f16 is refused as before, with the way out
    with pytest.raises(ValueError, match="nothing to scale"):
        m.fit(gen, 1, trainable="heads", loss_scale=STATIC_SCALE)
    with pytest.raises(ValueError, match="power of two"):
        m.fit(gen, 1, trainable="head_blocks", loss_scale=100)
    with pytest.raises(NotImplementedError, match="loss_scale='dynamic'"):
        m.fit(None, 1, trainable="head_blocks")
    for mm in (m, m2, mh, fresh):
        mm.engine.close()


# ---- 8. the dynamic scale
def _replay(flags, scale, interval, lo=1.0, hi=2.0 ** 24):
    """Keras' rule, restated: the scale after each step of a run with these overflow flags"""
    out, good = [], 0
    for f in flags:
        if f:
            scale, good = max(scale / 2, lo), 0
        else:
            good += 1
            if good == interval:
                scale, good = min(scale * 2, hi), 0
        out.append(scale)
    return out


def test_fit_dynamic_scale_skips_halves_and_grows(tmp_path):
    from yolo4hip.loss_scale import LossScale
    for d in "abc":
        (tmp_path / d).mkdir()
    # one batch per epoch: an epoch's 'skipped_steps' is that step's overflow flag, its 'loss_scale' the scale after it
    m, gen, before, hist = _fit(tmp_path / "a", "head_blocks", epochs=1, loss_scale=LossScale(initial=2 ** 24, growth_interval=2), images=3)
    assert len(gen) == 1
    assert hist.history["skipped_steps"] == [1] and hist.history["loss_scale"] == [2.0 ** 23]
    assert np.array_equal(m._flat.view(np.int32), before.view(np.int32))    # nothing moved, the heads included
    assert np.isfinite(hist.history["loss"]).all()
    m.engine.close()
    epochs = 24
    runs = []
    for d in "bc":
        policy = LossScale(initial=2 ** 24, growth_interval=2)
        m, _, before, hist = _fit(tmp_path / d, "head_blocks", epochs=epochs, loss_scale=policy, images=3)
        runs.append((m._flat.copy(), hist.history))
        assert policy.scale == hist.history["loss_scale"][-1] and policy.skipped == sum(hist.history["skipped_steps"])
        m.engine.close()
    flat, h = runs[0]
    flags, scales = h["skipped_steps"], h["loss_scale"]
    print("overflow flags:", flags, "log2 scale:", [float(np.log2(s)) for s in scales], "loss:", h["loss"])
    _note("fit_head_blocks_f16_dynamic", {"overflow_flags": flags, "log2_scale": [float(np.log2(s)) for s in scales], "history": h["loss"]})
    assert set(flags) <= {0, 1} and scales == _replay(flags, 2.0 ** 24, 2)
    steps = list(zip([2.0 ** 24] + scales, scales))
    assert any(b == a / 2 for a, b in steps) and any(b == a * 2 for a, b in steps)
    assert np.isfinite(h["loss"]).all() and (flat.view(np.int32) != before.view(np.int32)).any()
    assert h == runs[1][1] and np.array_equal(flat.view(np.int32), runs[1][0].view(np.int32))
