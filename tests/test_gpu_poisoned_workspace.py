"""Forward, detection tail and gradients on a POISONED workspace.

y4_bind_workspace zeroes the whole activation workspace and every other GPU test replays a few calls with n == max_batch on it, so
two classes of defect pass the rest of the suite: a read of bytes that no kernel of the call wrote (a tail tile past n * h * w, a
spatial tile past an image edge, candidate slots past the count, a split-K partial sum of another launch) meets zeros or the same
finite values as last time, and a store past what the call owns (image slot n, alignment slack, a neighbouring buffer) lands where
nothing looks.  Here every region the library does not itself keep zero (y4_workspace_map: ACT, TAIL, SCRATCH; never ZERO) is filled
before the call, with two patterns because each alone is blind (helpers.POISON_NAN, helpers.POISON_FINITE; the candidate keys with
an index-safe poison derived from their codec, helpers.key_poison), and

  * every tensor the call leaves -- conv taps where the layout has them, the heads, the five detection outputs -- equals the same
    call's on a fresh bind, bit for bit (`first_tap_difference` names the first layer that differs);
  * with aliasing off, the image slots >= n of every ACT row and per-image TAIL row, and every gap, still hold the poison;
  * the packed weights are unchanged.

No tolerance anywhere.  (96, 96) and (96, 160) are the smallest shapes at which the fused kernels and a halo band run.  Every test
prints how many bytes it poisoned and how many unowned bytes it held."""
import numpy as np
import pytest

import layer_local as LL
from helpers import (POISON_FINITE, POISON_NAN, PoisonedEmpty, first_tap_difference, fresh_bind, key_poison, poison, tap_snapshot,
                     unowned_bytes_intact)

pytestmark = pytest.mark.gpu

NCLS, MAX_BATCH = 3, 5
PATTERNS = (POISON_NAN, POISON_FINITE)
ALL = ("act", "tail", "scratch")
SHAPES = [(96, 96), (96, 160)]
_INPUTS, _FUSED_PLAIN = {}, {}


def _inputs(hw, seed=0):
    from yolo4hip import weights as W
    from yolo4hip.plan import build_plan
    if (hw, seed) not in _INPUTS:
        plan = build_plan(hw, NCLS)
        _INPUTS[(hw, seed)] = (W.flatten(W.synth_weights(plan, seed)), W.synth_images(MAX_BATCH, hw, seed))
    return _INPUTS[(hw, seed)]


def _engine(hw, dtype, max_batch=MAX_BATCH, **kw):
    import torch
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    blob, imgs = _inputs(hw)
    eng = Engine(NCLS, make_config(hw), max_batch=max_batch, dtype=dtype, **kw)
    eng.load_weight_blob(blob)
    return eng, torch.from_numpy(imgs).to(eng.device)


def _all_fusions_on(eng, hw):
    """stem (square only), chain, stage and residual fusion, asserted through the getters and the launch count"""
    from yolo4hip import ext
    square = hw[0] == hw[1]
    if square:
        eng.set_stem_fusion(True)
    else:
        with pytest.raises(ext.Y4Error):
            eng.set_stem_fusion(True)
    assert eng.set_chain_fusion(True) == 26
    assert eng.set_stage_fusion(True) and eng.stage_fusion_active()
    assert eng.set_res_fusion(True) == 10 and eng.res_fusion_mask() == 3
    assert eng.conv_launches_per_step() == (75 if square else 76)      # 104 unfused (tests/test_lib_abi.py: FRESH_LAUNCHES)


def _has_unowned_act_slots(eng, n):
    return any(r["kind"] == "act" and r["bytes"] > n * r["image_bytes"] for r in eng.workspace_map())


def _snapshot(eng, n):
    """`tap_snapshot` without the convs a fused kernel keeps on chip under the engine's switches (y4_conv_output_view): y4_get_conv_output
    refuses conv 0, the stage's and the residual blocks' inner convs itself, but copies the view of a conv INSIDE A RUN as it is --
    bytes of an earlier call, or the poison (found by this file: conv 8, the first such tap, came back as the poison)."""
    snap = tap_snapshot(eng, n)
    return {k: v for k, v in snap.items() if not k.startswith("conv") or eng.conv_output_view(int(k[4:]))[3]}


def _fresh(eng, imgs, n):
    fresh_bind(eng)
    eng.forward_device(imgs[:n])
    return _snapshot(eng, n)


def _poisoned_forwards(eng, imgs, tag, ns=(5, 3, 1), fresh=None):
    """The shared body: per n the call on a fresh bind, then per pattern and n the call on a poisoned workspace.
    -> {n: fresh snapshot}"""
    import torch
    wts = eng.wts.clone()
    fresh = fresh or {n: _fresh(eng, imgs, n) for n in ns}
    poisoned = checked = 0
    for byte in PATTERNS:
        for n in ns:
            poisoned += poison(eng, ALL, byte)
            eng.forward_device(imgs[:n])
            diff = first_tap_difference(fresh[n], _snapshot(eng, n), eng)
            assert diff is None, f"{tag}, poison {byte:#x}, n = {n} of {eng.max_batch}: differs from the fresh bind -- {diff}"
            if not eng.alias_workspace:
                if n < eng.max_batch:
                    assert _has_unowned_act_slots(eng, n)
                nb, bad = unowned_bytes_intact(eng, n, byte)
                checked += nb
                assert bad is None, f"{tag}, poison {byte:#x}, n = {n} of {eng.max_batch}: {bad}"
    assert torch.equal(wts, eng.wts), f"{tag}: the packed weights changed"
    print(f"{tag}: {poisoned} bytes poisoned over {len(PATTERNS) * len(ns)} calls, {checked} unowned bytes held their poison")
    return fresh


def _tail_only(snap):
    return {k: v for k, v in snap.items() if not k.startswith("conv")}


# ---- 1. float32, plain layout, no fusion
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_f32_plain(hw):
    eng, imgs = _engine(hw, "f32")
    fresh = _poisoned_forwards(eng, imgs, f"f32 plain {hw}")
    assert sum(k.startswith("conv") for k in fresh[5]) >= 107          # unfused: every conv is a tap
    eng.close()


def test_control_a_read_of_unowned_slots_shows():
    """The poison lies where a stray read meets it, and the comparison sees such a read: after a forward of 3 images a decode of 5
    reads the raw heads of slots 3 and 4, which no kernel of this forward wrote.  Images 0 .. 2 come out as on the fresh bind under
    both patterns; images 3 and 4 come out differently under the finite pattern (logits of 5e4 are candidates where zeros are not)
    -- and NOT under the NaN pattern, which every `score > threshold` drops: why there are two."""
    import torch
    eng, imgs = _engine((96, 96), "f32")
    fresh_bind(eng)
    eng.forward_device(imgs[:3])
    want = [o.clone() for o in eng.decode_nms_device(5)]
    differs = {}
    for byte in PATTERNS:
        poison(eng, ALL, byte)
        eng.forward_device(imgs[:3])
        got = eng.decode_nms_device(5)
        torch.cuda.synchronize()
        assert all(torch.equal(a[:3], b[:3]) for a, b in zip(want, got)), hex(byte)
        differs[byte] = not all(torch.equal(a[3:], b[3:]) for a, b in zip(want, got))
    assert differs == {POISON_NAN: False, POISON_FINITE: True}, differs
    eng.close()


# ---- 2. 16-bit, plain layout, every fusion on
def _fused_plain(hw, dtype):
    if (hw, dtype) not in _FUSED_PLAIN:
        eng, imgs = _engine(hw, dtype)
        _all_fusions_on(eng, hw)
        fresh = _poisoned_forwards(eng, imgs, f"{dtype} plain fused {hw}")
        eng.close()
        _FUSED_PLAIN[(hw, dtype)] = {n: _tail_only(s) for n, s in fresh.items()}
    return _FUSED_PLAIN[(hw, dtype)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_16bit_plain_fused(hw, dtype):
    _FUSED_PLAIN.pop((hw, dtype), None)
    _fused_plain(hw, dtype)


# ---- 3. 16-bit, aliased layout (what the benchmark and fit run on), same fusions; and equal to case 2
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_16bit_aliased_fused(hw, dtype):
    plain = _fused_plain(hw, dtype)
    eng, imgs = _engine(hw, dtype, alias_workspace=True)
    _all_fusions_on(eng, hw)
    rows = [r for r in eng.workspace_map() if r["kind"] == "act"]
    assert any(a["offset"] < b["offset"] + b["bytes"] and b["offset"] < a["offset"] + a["bytes"]
               for i, a in enumerate(rows) for b in rows[i + 1:]), "no two activation buffers share memory"
    fresh = _poisoned_forwards(eng, imgs, f"{dtype} aliased fused {hw}")
    for n, snap in fresh.items():
        diff = first_tap_difference(plain[n], snap)
        assert diff is None, f"{dtype} {hw} n = {n}: the aliased layout differs from the plain one -- {diff}"
    eng.close()


# ---- 4. sub-batching
@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
@pytest.mark.parametrize("images", [1, 2])
def test_bf16_subbatch(images, fused):
    hw = (96, 96)
    eng, imgs = _engine(hw, "bf16")
    if fused:
        _all_fusions_on(eng, hw)
    eng.set_subbatch(images, 16)
    _poisoned_forwards(eng, imgs, f"bf16 subbatch({images}, 16) {'fused' if fused else 'unfused'}")
    eng.close()


# ---- 5. small batches: the default schedule and a forced 2-way split-K (its partial sums live in the SCRATCH row)
SPLITK_2WAY = 110          # the id tests/test_gpu_forward.py::test_splitk_latency_schedule_vs_oracle forces


@pytest.mark.parametrize("dtype,splitk", [("bf16", False), ("f32", True), ("bf16", True)])
def test_small_batch_and_split_k(dtype, splitk):
    hw = (96, 96)
    eng, imgs = _engine(hw, dtype, max_batch=2)
    if splitk:
        eng.set_splitk(True)
        forced = LL.force_family(eng, imgs[:2], [SPLITK_2WAY])
        assert SPLITK_2WAY in forced, forced
        print(f"split-K id {SPLITK_2WAY} forced on {sum(t == SPLITK_2WAY for t in forced)} convs")
    _poisoned_forwards(eng, imgs, f"{dtype} max_batch 2{' split-K' if splitk else ''}", ns=(1, 2))
    counters = next(r for r in eng.workspace_map() if r["name"] == "splitk_counters")
    assert not bool(eng.act[counters["offset"]:counters["offset"] + counters["bytes"]].any()), "split-K tile counters not back at zero"
    eng.close()


# ---- 6. every tile family the suite forces elsewhere (conv_tiles.h schedule codes), n = 3 of 5
FAMILIES = {"ring3to7": (3, 4, 5, 6, 7), "code8": (8,), "code9": (9,), "code10": (10,), "staggered": (12,), "halo": (20,),
            "halo2": (21,), "mfma32x32x16": (32,)}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_bf16_forced_tile_family(family):
    hw = (96, 96)
    eng, imgs = _engine(hw, "bf16")
    forced = LL.force_family(eng, imgs[:3], LL.tiles_of(eng.lib, FAMILIES[family]))
    accepted = {i: t for i, t in enumerate(forced) if t}
    assert accepted, f"no conv accepted a {family} tile"
    print(f"{family}: forced on {len(accepted)} convs")
    _poisoned_forwards(eng, imgs, f"bf16 {family}", ns=(3,))
    eng.close()


# ---- 7. shrink and grow
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_shrink_and_grow(dtype):
    """dense n = 5, poison, n = 1 with OTHER images, n = 5 again: the workspace of a stream's ragged last batch and of the batch
    after it.  (bf16: every fusion on.)"""
    import torch
    hw = (96, 96)
    eng, imgs = _engine(hw, dtype)
    if dtype != "f32":
        _all_fusions_on(eng, hw)
    other = torch.flip(imgs[3:4], dims=(1, 2)).contiguous()
    one = _fresh(eng, other, 1)
    five = _fresh(eng, imgs, 5)
    for byte in PATTERNS:
        nbytes = poison(eng, ALL, byte)
        eng.forward_device(other)
        diff = first_tap_difference(one, _snapshot(eng, 1), eng)
        assert diff is None, f"{dtype}, poison {byte:#x}: n = 1 behind a dense batch -- {diff}"
        checked, bad = unowned_bytes_intact(eng, 1, byte)
        assert bad is None, f"{dtype}, poison {byte:#x}: n = 1 behind a dense batch -- {bad}"
        eng.forward_device(imgs)
        diff = first_tap_difference(five, _snapshot(eng, 5), eng)
        assert diff is None, f"{dtype}, poison {byte:#x}: n = 5 behind n = 1 -- {diff}"
        print(f"shrink and grow {dtype} {byte:#x}: {nbytes} bytes poisoned, {checked} unowned bytes held their poison")
    eng.close()


# ---- 8. the detection tail alone
def _set_mode(eng, mode):
    if mode == "diou":
        eng.set_nms_rule("diou", 0.6)
    elif mode == "agnostic":
        eng.set_nms_rule("iou", agnostic=True)
    elif mode in ("soft_gaussian", "soft_linear"):
        eng.set_nms_soft(mode[5:])
    elif mode == "matrix":
        eng.set_nms_matrix("gaussian")
    elif mode == "merge":
        eng.set_nms_merge(True)
    else:
        assert mode in ("hard", "gathered"), mode


def _gathered(eng, n, byte=None):
    """decode -> gather (one group per image, identity map) -> NMS; byte: the engine's gather scratch is poisoned behind its
    counters (which y4_gather_begin has just zeroed): keys index-safe (ids < max_slots * nbox * C = group_cap), boxes with `byte`"""
    import torch
    cap = eng.num_boxes * eng.num_classes
    state = eng.gather_begin(n, 1, cap)
    nbytes = 0
    if byte is not None:
        up = lambda x: (x + 255) // 256 * 256
        scratch = state[1]
        keys_off = up(n * 256)
        boxes_off = keys_off + up(n * cap * 8)
        assert scratch.numel() == boxes_off + up(n * eng.num_boxes * 16), "the gather scratch's layout is not the one restated here"
        scratch[keys_off:boxes_off].view(torch.int64).copy_(key_poison((boxes_off - keys_off) // 8, cap, scratch.device))
        scratch[boxes_off:].fill_(byte)
        nbytes = scratch.numel() - keys_off
    dev = eng.device
    eng.decode_gather(state, n, torch.arange(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                      torch.tensor([[1.0, 0.0, 1.0, 0.0]] * n, dtype=torch.float32, device=dev))
    outs, cnt = eng.nms_gathered(state)
    torch.cuda.synchronize()
    return list(outs) + [cnt], nbytes


@pytest.mark.parametrize("mode", ["hard", "diou", "agnostic", "soft_gaussian", "soft_linear", "matrix", "merge", "gathered"])
def test_detection_tail_alone(mode):
    """The dense 96^2 heads of decode_nms_cases (two dense images, three sparse) through decode + NMS with TAIL and SCRATCH
    poisoned, under every NMS mode: the bits of the unpoisoned call."""
    import torch
    import decode_nms_cases as DC
    heads = [h[:MAX_BATCH] for h in DC.dense_case(NCLS)[0]]
    cfg, eng = DC._engine(DC.SIZE_DENSE, NCLS, MAX_BATCH)
    _set_mode(eng, mode)

    def run(n, byte=None):
        if mode == "gathered":
            return _gathered(eng, n, byte)
        outs = list(eng.decode_nms_device(n))
        torch.cuda.synchronize()
        return outs, 0

    want = {}
    for n in (MAX_BATCH, 2):
        fresh_bind(eng)
        eng.set_heads([h[:n] for h in heads])
        want[n], _ = run(n)
        assert int(want[n][3].min()) > 0 and int(want[n][3].max()) == 100, want[n][3]
    poisoned = checked = 0
    for byte in PATTERNS:
        for n in (MAX_BATCH, 2):
            eng.set_heads([h[:n] for h in heads])
            poisoned += poison(eng, ("tail", "scratch"), byte)
            got, extra = run(n, byte)
            poisoned += extra
            for name, a, b in zip(("boxes", "scores", "classes", "valid", "kept", "cand_count"), want[n], got):
                assert torch.equal(a, b), f"{mode}, poison {byte:#x}, n = {n}: {name} differs from the unpoisoned call"
            nb, bad = unowned_bytes_intact(eng, n, byte, kinds=("tail",))
            checked += nb
            assert bad is None, f"{mode}, poison {byte:#x}, n = {n}: {bad}"
    print(f"detection tail {mode}: {poisoned} bytes poisoned, {checked} unowned bytes held their poison")
    eng.close()


# ---- 9. training: loss and gradients on poisoned scratch, the tail of a forward on a poisoned arena
@pytest.mark.parametrize("dtype,alias", [("f32", False), ("bf16", False), ("bf16", True), ("f16", True)])
def test_training_calls(dtype, alias):
    import torch
    import loss_cases as LC
    hw, n = (96, 96), 3
    eng, imgs = _engine(hw, dtype, alias_workspace=alias, retain_head_inputs=2)
    scale = {"loss_scale": 1024.0} if dtype == "f16" else {}
    boxes = torch.from_numpy(LC.make_boxes(hw, NCLS, n, seed=5)).to(eng.device)
    records = eng.assign_device(boxes)
    assert int(records[1].min()) >= 0 and int(records[1].max()) > 0          # (image 0 has no box; -1 would be a box off the grid)

    def calls():
        loss = eng.loss_device(n, records=records)
        dw = eng.head_grad_device(n, records=records)
        dk = eng.block_grad_device(n, records=records, **scale)
        if scale:
            assert int(dk[1]) == 0, "dZ overflowed"
            dk = dk[0]
        torch.cuda.synchronize()
        return {"loss": loss, "head_grad": dw, "block_grad": dk}

    eng.forward_device(imgs[:n])
    heads = [h.clone() for h in eng.heads_device(n)]
    cache = eng.alloc_feature_cache(n)
    eng.store_features(cache, np.arange(n))
    want = calls()
    assert all(bool(torch.isfinite(v).all()) and bool(v.any()) for v in want.values())
    poisoned = 0
    for byte in PATTERNS:
        poisoned += poison(eng, ("scratch",), byte)
        eng._block_scratch.fill_(byte)
        poisoned += eng._block_scratch.numel()
        with PoisonedEmpty(eng, byte) as p:
            got = calls()
        poisoned += p.bytes
        for name in want:
            assert torch.equal(want[name], got[name]), f"{dtype} alias {alias}, poison {byte:#x}: {name} differs from the unpoisoned call"
        # the cached features into an arena poisoned before the load, then only the convs behind them
        poisoned += poison(eng, ALL, byte)
        eng.load_features(cache, np.arange(n))
        eng.forward_tail_device(n)
        for k, (a, b) in enumerate(zip(heads, eng.heads_device(n))):
            assert torch.equal(a, b), f"{dtype} alias {alias}, poison {byte:#x}: head {k} of forward_tail_device differs from forward_device's"
        again = calls()
        for name in want:
            assert torch.equal(want[name], again[name]), f"{dtype} alias {alias}, poison {byte:#x}: {name} behind forward_tail_device differs"
        if not alias:
            nb, bad = unowned_bytes_intact(eng, n, byte)
            assert bad is None, f"{dtype}, poison {byte:#x}: {bad}"
    print(f"training {dtype} alias {alias}: {poisoned} bytes poisoned")
    eng.close()
