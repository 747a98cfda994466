"""Tiled inference on the device: y4_window_u8_ragged against the ragged resize on contiguous copies, the gathered decode + NMS
(y4_decode_gather, y4_nms_gathered) against the tiled oracle (tests/tiled_oracle.py) on the cases of tests/tiled_cases.py, the
handle's state, determinism, the capacity contract, and Engine.predict_tiled / the facade end to end."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import decode_nms_cases as DC
import nms_rule_cases as RC
import tiled_cases as TC
import tiled_oracle as TO
from helpers import CLASS_DIR

pytestmark = pytest.mark.gpu

NBOX = 3 * sum((TC.SIZE // s) ** 2 for s in (8, 16, 32))             # 567 boxes of a 96^2 row
IDENT = (1.0, 0.0, 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def _eng(ncls):
    """The 96^2 engine of decode_nms_cases with max_batch = 4 (kept for the module: decode / NMS read no weights)."""
    return DC._engine(TC.SIZE, ncls, TC.CHUNK)


def _gathered(eng, heads, group, slot, maps, n_groups, max_slots, group_cap, rule=("iou", 1.0, False), iou=-1.0, score=-1.0):
    """set_heads per chunk of CHUNK rows -> decode_gather -> nms_gathered: -> (the five outputs as numpy, cand_count)."""
    import torch
    eng.set_nms_rule(*rule)
    try:
        state = eng.gather_begin(n_groups, max_slots, group_cap)
        g = torch.from_numpy(np.ascontiguousarray(group, np.int32)).to(eng.device)
        s = torch.from_numpy(np.ascontiguousarray(slot, np.int32)).to(eng.device)
        m = torch.from_numpy(np.ascontiguousarray(maps, np.float32).reshape(-1, 4)).to(eng.device)
        for r0 in range(0, len(group), TC.CHUNK):
            n = eng.set_heads([h[r0:r0 + TC.CHUNK] for h in heads])
            eng.decode_gather(state, n, g[r0:r0 + n], s[r0:r0 + n], m[r0:r0 + n], score)
        outs, cnt = eng.nms_gathered(state, None, None, iou)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in outs], cnt.cpu().numpy()
    finally:
        eng.set_nms_rule("iou")


def _case(ncls, seed, rule, group_cap=1 << 15):
    _, group, slot, maps, per_group = TC.geometry()
    _, eng = _eng(ncls)
    return _gathered(eng, TC.heads(ncls, seed), group, slot, maps, len(per_group), max(per_group), group_cap, TC.RULES[rule])


# ------------------------------------------------------------------------------------------------ 1. the window kernel
def _window_table(img_hw):
    """(y0, x0, wh, ww, rect) of the windows test 1 cuts from its 131 x 173 image, on a 96^2 canvas."""
    from yolo4hip import prepost
    h, w = img_hw
    full = (96, 96, 0, 0)
    return [(3, 5, 96, 96, full), (8, 11, 96, 96, full),                     # 1:1 at an odd x0: the source offset is not 4-byte aligned
            (h - 96, w - 96, 96, 96, full), (100, 140, h - 100, w - 140, full),   # touching the last row and column: 1:1, stretched
            (0, 0, 96, 96, full), (0, 0, h, w, full),
            (20, 31, 50, 70, full),                                          # a 50 x 70 window stretched ...
            (20, 31, 50, 70, prepost.letterbox_rect(50, 70, 96, 96)),        # ... and letterboxed, with pads
            (20, 31, 70, 50, prepost.letterbox_rect(70, 50, 96, 96)),
            (60, 61, 1, 1, full), (h - 1, w - 1, 1, 1, (31, 17, 40, 9))]     # a 1 x 1 window


def _desc_tensor(eng, desc):
    import torch
    return torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(eng.device)


def test_window_kernel_equals_the_ragged_resize_of_contiguous_copies():
    import torch
    from yolo4hip import ext
    _, eng = _eng(3)
    rng = np.random.default_rng(131173)
    img = rng.integers(0, 256, (131, 173, 3), dtype=np.uint8)
    table = _window_table(img.shape[:2])
    n, H, W = len(table), TC.SIZE, TC.SIZE
    # the reference: y4_resize_u8_ragged on np.ascontiguousarray(img[y0:y0+h, x0:x0+w]) with the same rectangle
    crops = [np.ascontiguousarray(img[y0:y0 + wh, x0:x0 + ww]) for y0, x0, wh, ww, _ in table]
    rdesc = (ext.y4_image_desc * n)()
    off = 0
    for d, c, (_, _, wh, ww, rect) in zip(rdesc, crops, table):
        d.offset, d.h, d.w = off, wh, ww
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
        off += c.size
    rsrc = torch.from_numpy(np.concatenate([c.reshape(-1) for c in crops])).to(eng.device)
    ref = eng.resize_u8_ragged(rsrc, _desc_tensor(eng, rdesc), n, torch.empty((n, H, W, 3), dtype=torch.uint8, device=eng.device), 77)
    ref = ref.cpu().numpy()
    # (a) every descriptor points into ONE shared source; (b) descriptor k points into its own image, equal to `img` inside window
    # k and inverted everywhere else: a tap that reads beyond the window's edge changes the result
    srcs = [img]
    for y0, x0, wh, ww, _ in table:
        other = 255 - img
        other[y0:y0 + wh, x0:x0 + ww] = img[y0:y0 + wh, x0:x0 + ww]
        srcs.append(other)
    src = torch.from_numpy(np.concatenate([s.reshape(-1) for s in srcs])).to(eng.device)
    pitch = img.shape[1] * 3
    for own in (False, True):
        wdesc = (ext.y4_window_desc * n)()
        for k, (d, (y0, x0, wh, ww, rect)) in enumerate(zip(wdesc, table)):
            d.offset = (img.size * (k + 1) if own else 0) + y0 * pitch + x0 * 3
            d.pitch, d.h, d.w = pitch, wh, ww
            d.out_h, d.out_w, d.pad_top, d.pad_left = rect
        assert any(d.offset % 4 for d in wdesc[:2])                    # a source offset that is not 4-byte aligned
        got = eng.window_u8_ragged(src, _desc_tensor(eng, wdesc), n, torch.zeros((n, H, W, 3), dtype=torch.uint8, device=eng.device), 77)
        got = got.cpu().numpy()
        for k in range(n):
            assert np.array_equal(got[k], ref[k]), (own, k, table[k], int((got[k] != ref[k]).sum()))
        # an output that is not 4-byte aligned takes the one-pixel-per-thread store: the same bytes
        flat = torch.zeros(n * H * W * 3 + 4, dtype=torch.uint8, device=eng.device)
        eng.window_u8_ragged(src, _desc_tensor(eng, wdesc), n, flat[1:], 77)
        assert np.array_equal(flat[1:1 + n * H * W * 3].cpu().numpy().reshape(n, H, W, 3), ref) and int(flat[0]) == 0
    # the 1:1 windows are plain copies
    assert np.array_equal(ref[0], img[3:99, 5:101])
    lib = eng.lib
    out = torch.empty((1, H, W, 3), dtype=torch.uint8, device=eng.device)
    assert lib.y4_window_u8_ragged(None, ext.ptr(src), 1, ext.ptr(out), H, W, 0, None) == -22
    assert lib.y4_window_u8_ragged(ext.ptr(src), ext.ptr(src), 1, ext.ptr(out), H, W, 256, None) == -22
    assert lib.y4_window_u8_ragged(ext.ptr(src), ext.ptr(src), 0, ext.ptr(out), H, W, 0, None) == -22


def test_whole_image_windows_equal_the_ragged_resize_of_the_same_table():
    """A window that is its whole image (pitch == 3 * w, the image's own offset) is the packed case: y4_window_u8_ragged writes the
    bytes y4_resize_u8_ragged writes for the same offsets, sizes and rectangles.  Up- and down-scaled, 1 x N, N x 1, one image of
    the canvas's size, stretched and letterboxed."""
    import torch
    from yolo4hip import ext, prepost
    _, eng = _eng(3)
    H = W = TC.SIZE
    rng = np.random.default_rng(9600)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((131, 173), (40, 31), (1, 77), (77, 1), (H, W), (200, 55))]
    rects = [(H, W, 0, 0)] * len(imgs) + [prepost.letterbox_rect(a.shape[0], a.shape[1], H, W) for a in imgs]
    imgs = imgs + imgs
    n = len(imgs)
    src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(eng.device)
    rdesc, wdesc = (ext.y4_image_desc * n)(), (ext.y4_window_desc * n)()
    off = 0
    for r, w_, a, rect in zip(rdesc, wdesc, imgs, rects):
        r.offset, r.h, r.w = off, a.shape[0], a.shape[1]
        w_.offset, w_.pitch, w_.h, w_.w = off, 3 * a.shape[1], a.shape[0], a.shape[1]
        r.out_h, r.out_w, r.pad_top, r.pad_left = rect
        w_.out_h, w_.out_w, w_.pad_top, w_.pad_left = rect
        off += a.size
    want = eng.resize_u8_ragged(src, _desc_tensor(eng, rdesc), n, torch.zeros((n, H, W, 3), dtype=torch.uint8, device=eng.device), 77)
    got = eng.window_u8_ragged(src, _desc_tensor(eng, wdesc), n, torch.ones((n, H, W, 3), dtype=torch.uint8, device=eng.device), 77)
    want, got = want.cpu().numpy(), got.cpu().numpy()
    for k in range(n):
        assert np.array_equal(got[k], want[k]), (k, imgs[k].shape, rects[k], int((got[k] != want[k]).sum()))
    assert np.array_equal(want[4], imgs[4])                                  # the image of the canvas's size is a plain copy


# ------------------------------------------------------------------------------------------------ 2. gather + NMS vs the oracle
@pytest.mark.parametrize("ncls,seed,rule", sorted(TC.MARGINS))
def test_gathered_nms_equals_the_oracle(ncls, seed, rule):
    ref = TC.reference(ncls, seed, rule)
    assert ref[5] >= 1e-5
    got, cnt = _case(ncls, seed, rule)
    DC.assert_same_detections(got, ref[:5])               # decisions identical (kept_idx = slot * nbox + box), boxes 1e-5, scores 1e-6
    assert cnt.tolist() == ref[6].tolist()                # the candidate counts, exactly
    v = int(got[3][0])
    assert set((got[4][0][:v] // NBOX).tolist()) == set(range(13))


# ------------------------------------------------------------------------------------------------ 3. witnesses
def _pair_heads(cls_a, cls_b, lc_a=2.0, lc_b=1.0):
    """Row 0: the witness box of nms_rule_cases on stride-8 cell (5, 7); row 1: the same box on cell (5, 3)."""
    return DC._heads_with(TC.SIZE, 3, 2, [(0, 0, 5, 7, 0, cls_a, 8.0, lc_a, RC.T_PAIR), (1, 0, 5, 3, 0, cls_b, 8.0, lc_b, RC.T_PAIR)])


SHIFT5 = np.float32(5 * 8 / TC.SIZE)         # five cells: row 1's box lands on cell (5, 8), next to row 0's: IoU 12/28 = 0.4286 > 0.413
TOGETHER = np.array([IDENT, (1.0, SHIFT5, 1.0, 0.0)], np.float32)
APART = np.array([IDENT, IDENT], np.float32)
BOX_A, BOX_B = 3 * (5 * 12 + 7), 3 * (5 * 12 + 3)


def _witness(heads, maps, rule=("iou", 1.0, False), slots=(0, 1)):
    cfg, eng = _eng(3)
    got, cnt = _gathered(eng, heads, [0, 0], slots, maps, 1, 2, 64, rule)
    order = np.argsort(slots)
    ref = TO.gathered_nms([([h[order] for h in heads], np.asarray(maps)[order])], 3, cfg, TC.SIZE, TC.IOU_THR, TC.SCORE_THR, *rule)
    DC.assert_same_detections(got, ref[:5])
    assert cnt.tolist() == [2]
    return got


def test_boxes_of_two_slots_meet_in_the_photo():
    """Same class: the boxes do not touch in tile coordinates (32 px apart, 20 px wide) and overlap with IoU 0.4286 after their
    maps: one survives; under maps that leave them apart both do."""
    got = _witness(_pair_heads(1, 1), TOGETHER)
    assert got[3].tolist() == [1] and got[4][0][0] == BOX_A
    got = _witness(_pair_heads(1, 1), APART)
    assert got[3].tolist() == [2] and got[4][0][:2].tolist() == [BOX_A, NBOX + BOX_B]
    # DIoU-NMS keeps both (0.4286 - 0.1736 < 0.413): the measure, too, is taken on the mapped boxes
    assert _witness(_pair_heads(1, 1), TOGETHER, ("diou", 0.6, False))[3].tolist() == [2]


def test_two_classes_across_slots_and_the_agnostic_rule():
    assert _witness(_pair_heads(1, 2), TOGETHER)[3].tolist() == [2]
    got = _witness(_pair_heads(1, 2), TOGETHER, ("iou", 1.0, True))
    assert got[3].tolist() == [1] and got[4][0][0] == BOX_A and got[2][0][0] == 1.0


def test_equal_scores_are_ordered_by_slot():
    """Bit-equal scores in two slots, boxes that coincide: the slot-0 box is kept, whichever row carries slot 0."""
    heads = DC._heads_with(TC.SIZE, 3, 2, [(0, 0, 5, 7, 0, 1, 8.0, 2.0, RC.T_PAIR), (1, 0, 5, 7, 0, 1, 8.0, 2.0, RC.T_PAIR)])
    for slots in ((0, 1), (1, 0)):
        got = _witness(heads, APART, slots=slots)
        assert got[3].tolist() == [1] and got[4][0][0] == BOX_A            # = 0 * nbox + box, not nbox + box


# ------------------------------------------------------------------------------------------------ 4. anchor to y4_decode_nms
@pytest.mark.parametrize("ncls", [3, 80])
def test_one_group_per_row_is_decode_nms(ncls):
    import torch
    _, eng = _eng(ncls)
    heads = [h[:TC.CHUNK] for h in TC.heads(ncls, 0)]
    n = eng.set_heads(heads)
    plain = [o.cpu().numpy() for o in eng.decode_nms_device(n)]
    got, cnt = _gathered(eng, heads, np.arange(n), np.zeros(n), np.tile(np.float32(IDENT), (n, 1)), n, 1, NBOX * ncls)
    torch.cuda.synchronize()
    for a, b in zip(got, plain):
        assert np.array_equal(a, b)
    assert plain[3].sum() > 0 and (cnt > 0).all()


# ------------------------------------------------------------------------------------------------ 5. the handle's state
def test_gathered_and_plain_calls_alternate_on_one_handle():
    cfg, eng = _eng(3)
    ref = TC.reference(3, 1, "iou")
    plain_heads = [h[3:6] for h in TC.heads(3, 2)]
    plain_ref = DC.reference(plain_heads, 3, cfg, TC.SIZE)
    got, cnt = _case(3, 1, "iou")                                         # gathered ...
    DC.assert_same_detections(got, ref[:5])
    DC._compare(eng, cfg, plain_heads, TC.SIZE, 3, ref=plain_ref)         # ... then plain, on fewer rows than the last chunk
    got, cnt = _case(3, 1, "iou")                                         # ... then gathered again
    DC.assert_same_detections(got, ref[:5])
    assert cnt.tolist() == ref[6].tolist()
    DC._compare(eng, cfg, [h[:4] for h in TC.heads(3, 2)], TC.SIZE, 3)
    # a gathered sequence that is abandoned before its NMS leaves nothing behind on the handle either
    _, group, slot, maps, per_group = TC.geometry()
    import torch
    state = eng.gather_begin(2, 13, 1 << 15)
    n = eng.set_heads([h[:4] for h in TC.heads(3, 1)])
    dev = [torch.from_numpy(np.ascontiguousarray(a[:4])).to(eng.device) for a in (group, slot, maps)]
    eng.decode_gather(state, n, *dev)
    DC._compare(eng, cfg, plain_heads, TC.SIZE, 3, ref=plain_ref)


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_gathered_outputs_are_the_same_bits_on_every_run():
    a, ca = _case(80, 0, "iou")
    b, cb = _case(80, 0, "iou")
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))
    assert np.array_equal(ca, cb)


# ------------------------------------------------------------------------------------------------ 7. capacity and refusals
def test_capacity_is_reported_and_nothing_is_out_of_range():
    ref = TC.reference(3, 0, "iou")
    got, cnt = _case(3, 0, "iou", group_cap=64)                           # returns Y4_OK (ext.check raises otherwise)
    assert cnt.tolist() == ref[6].tolist() and (cnt > 64).all()            # the true counts, above the capacity
    b, s, c, v, k = got
    assert ((0 <= v) & (v <= 100)).all() and b.min() >= 0.0 and b.max() <= 1.0
    for g in range(2):
        assert ((0 <= k[g, :v[g]]) & (k[g, :v[g]] < 13 * NBOX)).all() and (k[g, v[g]:] == -1).all()
    again, cnt = _case(3, 0, "iou")                                        # the scratch of the next sequence is unharmed
    DC.assert_same_detections(again, ref[:5])


def test_refusals_come_before_any_launch():
    import torch
    from yolo4hip import ext
    _, eng = _eng(80)
    lib, h = eng.lib, eng.handle
    nbytes = C.c_size_t()
    too_many = (1 << 31) // (NBOX * 80) + 1                                # max_slots * nbox * C >= 2^31
    assert lib.y4_gather_scratch_bytes(h, 1, too_many, 64, C.byref(nbytes)) == -22
    assert lib.y4_gather_scratch_bytes(h, 1, too_many - 1, 64, C.byref(nbytes)) == 0
    for bad in ((0, 1, 64), (1, 0, 64), (1, 1, 0)):
        assert lib.y4_gather_scratch_bytes(h, *bad, C.byref(nbytes)) == -22
    assert lib.y4_gather_scratch_bytes(h, 2, 13, 64, None) == -22
    assert lib.y4_gather_scratch_bytes(h, 2, 13, 1 << 15, C.byref(nbytes)) == 0
    assert nbytes.value >= 2 * 256 + 2 * (1 << 15) * 8 + 2 * 13 * NBOX * 16
    scratch = torch.zeros(nbytes.value, dtype=torch.uint8, device=eng.device)
    tab = torch.zeros(16, dtype=torch.int32, device=eng.device)
    maps = torch.zeros(16, dtype=torch.float32, device=eng.device)
    outs = eng.alloc_outputs(2)
    cnt = torch.zeros(2, dtype=torch.int32, device=eng.device)
    sp, p = ext.ptr(scratch), ext.ptr
    assert lib.y4_gather_begin(h, 2, 13, 1 << 15, None, None) == -22
    assert lib.y4_gather_begin(h, 2, too_many, 1 << 15, sp, None) == -22
    assert lib.y4_gather_begin(h, 2, 13, 1 << 15, C.c_void_p(scratch.data_ptr() + 8), None) == -22
    eng.set_heads([hd[:4] for hd in TC.heads(80, 0)])
    for args in ((None, p(tab), p(maps)), (p(tab), None, p(maps)), (p(tab), p(tab), None)):
        assert lib.y4_decode_gather(h, 4, -1.0, *args, 2, 13, 1 << 15, sp, None) == -22
    assert lib.y4_decode_gather(h, 4, -1.0, p(tab), p(tab), p(maps), 2, 13, 1 << 15, None, None) == -22
    assert lib.y4_decode_gather(h, 4, -1.0, p(tab), p(tab), p(maps), 2, too_many, 1 << 15, sp, None) == -22
    assert lib.y4_decode_gather(h, 5, -1.0, p(tab), p(tab), p(maps), 2, 13, 1 << 15, sp, None) == -22      # n > max_batch
    assert lib.y4_decode_gather(None, 4, -1.0, p(tab), p(tab), p(maps), 2, 13, 1 << 15, sp, None) == -22
    b, s, c, v, k = (p(o) for o in outs)
    assert lib.y4_nms_gathered(h, 2, 13, 1 << 15, -1.0, None, p(cnt), b, s, c, v, k, None) == -22
    assert lib.y4_nms_gathered(h, 2, 13, 1 << 15, -1.0, sp, None, b, s, c, v, k, None) == -22
    assert lib.y4_nms_gathered(h, 2, 13, 1 << 15, -1.0, sp, p(cnt), None, s, c, v, k, None) == -22
    assert lib.y4_nms_gathered(h, 2, 13, 1 << 15, -1.0, sp, p(cnt), b, s, c, None, k, None) == -22
    assert lib.y4_nms_gathered(h, 2, too_many, 1 << 15, -1.0, sp, p(cnt), b, s, c, v, k, None) == -22
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0 and int(scratch.view(torch.int32).abs().sum()) == 0      # nothing was written
    ref = TC.reference(80, 1, "iou")                                       # and the handle works as before
    got, cc = _case(80, 1, "iou")
    DC.assert_same_detections(got, ref[:5])


# ------------------------------------------------------------------------------------------------ 8. engine and facade
FACADE_SIZE, FACADE_SCORE = 160, 0.05


@functools.lru_cache(maxsize=None)
def _model():
    """The tiny synthetic net of tests/test_gpu_api.py (bccd classes, 160^2, fp32, max_batch 4) with the score threshold lowered
    so that the untrained net keeps boxes."""
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg = dict(make_config(FACADE_SIZE))
    cfg["score_threshold"] = FACADE_SCORE
    return cfg, Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), cfg, dtype="f32", max_batch=4)


def _photo(h, w, seed):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_facade_one_window_is_inference_model_predict():
    """(a) a photo of exactly the network size, full_image=False, overlap at its default: one 1:1 window -> the bits of
    inference_model.predict."""
    from yolo4hip import tiling
    _, m = _model()
    img = _photo(FACADE_SIZE, FACADE_SIZE, 1)
    rows = tiling.tile_rows(FACADE_SIZE, FACADE_SIZE, (FACADE_SIZE, FACADE_SIZE), full_image=False)
    assert [r[0] for r in rows] == [(0, 0, FACADE_SIZE, FACADE_SIZE)] and rows[0][1] == (FACADE_SIZE, FACADE_SIZE, 0, 0)
    ref = m.inference_model.predict(img[None])
    assert int(ref[3].sum()) > 0
    got = m.predict_tiled([img], full_image=False)
    assert len(got) == 4
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[0].flags.writeable


def test_facade_tiled_photo_equals_the_oracle_on_its_own_heads():
    """(b) a 200 x 260 photo: 2 x 2 windows + the full image = 5 rows, two forward chunks.  The oracle is fed with the heads
    Engine.forward_heads gives for the same window bytes in the same chunking."""
    from yolo4hip import prepost, tiling
    cfg, m = _model()
    eng = m.engine
    S = FACADE_SIZE
    photo = _photo(200, 260, 2)
    rows = tiling.tile_rows(200, 260, (S, S), None, 0.2, True, False)
    assert [r[0] for r in rows] == [(0, 0, S, S), (0, 100, S, S), (40, 0, S, S), (40, 100, S, S), (0, 0, 200, 260)]
    canvases = np.stack([photo[y0:y0 + wh, x0:x0 + ww] if (wh, ww) == (S, S) else prepost.resize_bilinear(photo[y0:y0 + wh, x0:x0 + ww], (S, S))
                         for (y0, x0, wh, ww), _, _ in rows])
    heads = eng.forward_heads(canvases)                                   # chunks of max_batch = 4 rows, as predict_tiled
    maps = np.stack([r[2] for r in rows])
    ref = TO.gathered_nms([(heads, maps)], m.num_classes, cfg, S, cfg["iou_threshold"], FACADE_SCORE)
    got = eng.predict_tiled([photo], with_indices=True)
    facade = m.predict_tiled(photo)
    for a, b in zip(facade, got[:4]):
        assert np.array_equal(a, b)
    print(f"tiled facade: oracle min_margin {ref[5]:.3g}, valid {int(ref[3][0])}, candidates {int(ref[6][0])}")
    assert int(ref[3][0]) > 0
    if ref[5] >= 1e-5:
        DC.assert_same_detections(got, ref[:5])
    else:
        # a pair within 1e-5 of the threshold may fall either way (the README's parity rule): the kept sets may then differ in
        # near-ties only, at most 3 % of the positions
        a = set(zip(got[4][0][:got[3][0]].tolist(), got[2][0][:got[3][0]].tolist()))
        b = set(zip(ref[4][0][:ref[3][0]].tolist(), ref[2][0][:ref[3][0]].tolist()))
        assert len(a ^ b) <= 0.03 * max(len(b), 1)
    slots = set((got[4][0][:got[3][0]] // eng.num_boxes).tolist())
    assert slots <= set(range(5))
    # capacity: with every (box, class) a candidate, 64 keys cannot hold a photo
    with pytest.raises(RuntimeError, match="tile_candidates"):
        eng.predict_tiled([photo], tile_candidates=64, score_threshold=0.0)
    again = eng.predict_tiled([photo], with_indices=True)                 # and the engine is as usable as before
    for a, b in zip(again, got):
        assert np.array_equal(a, b)


def test_facade_predict_img_tiled_dataframe(capsys):
    """(c) the DataFrame of predict_img, pixel coordinates inside the photo."""
    _, m = _model()
    photo = _photo(200, 260, 2)
    plain = m.predict_img(photo, plot_img=False)
    det = m.predict_img_tiled(photo, plot_img=False)
    assert list(det.columns) == list(plain.columns) == ["x1", "y1", "x2", "y2", "class_name", "score", "w", "h"]
    assert len(det) > 0
    assert (det[["x1", "x2"]].values >= 0).all() and (det[["x1", "x2"]].values <= 260).all()
    assert (det[["y1", "y2"]].values >= 0).all() and (det[["y1", "y2"]].values <= 200).all()
    assert set(det["class_name"]) <= set(m.class_names)
    out, det2 = m.predict_img_tiled(photo, plot_img=False, return_output=True, tile=128, overlap=0.5, full_image=False)
    assert out.shape == photo.shape and list(det2.columns) == list(det.columns)
    assert "img shape:" in capsys.readouterr().out


def test_facade_refuses_images_that_are_not_uint8():
    """(d)"""
    _, m = _model()
    for bad in (np.zeros((200, 260, 3), np.float32), [np.zeros((200, 260, 3), np.float64)], np.zeros((200, 260), np.uint8)[..., None], []):
        with pytest.raises(ValueError):
            m.predict_tiled(bad)
    with pytest.raises(ValueError):
        m.predict_tiled(_photo(200, 260, 2), overlap=1.0)
