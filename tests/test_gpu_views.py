"""Test-time augmentation on the device: y4_view_u8_ragged against np.flip of y4_window_u8_ragged, y4_decode_gather_views against
y4_decode_gather on positive maps and against the oracle (tests/views_oracle.py) on the cases of tests/views_cases.py, the mirror
witnesses, labels that follow pixels through the pieces of `Engine.predict_tta_device` (tests/marker_photos.py), and
`Engine.predict_tta` / `predict_tiled(views=...)` / `Yolov4.evaluate_map(views=...)` end to end."""
import ctypes as C

import numpy as np
import pytest

import decode_nms_cases as DC
import marker_photos as MP
import nms_rule_cases as RC
import test_gpu_labels_follow_pixels as GL
import test_gpu_nms_merge as GM
import test_gpu_tiled as GT
import test_labels_follow_pixels_cpu as LC
import tiled_cases as TC
import views_cases as VC
import views_oracle as VO

pytestmark = pytest.mark.gpu

NBOX = VC.NBOX
IDENT = (1.0, 0.0, 1.0, 0.0)
FLIP_AXES = {0: (), 1: (1,), 2: (0,), 3: (0, 1)}


def _flip(a, bits):
    return np.flip(a, axis=FLIP_AXES[bits]) if bits else a


# ------------------------------------------------------------------------------------------------ 1. the view kernel
def _view_table(img_hw, H, W):
    """(y0, x0, wh, ww, rect) rows of one 131 x 173 photo on an H x W canvas: windows at odd offsets, the whole photo, stretched and
    letterboxed, rectangles scaled about their centre by tiling.view_rect, a 1 x 1 window; every row reads the one photo."""
    from yolo4hip import prepost, tiling
    h, w = img_hw
    full = (H, W, 0, 0)
    th, tw = min(H, h), min(W, w)
    lb = prepost.letterbox_rect(h, w, H, W)
    return [(3, 5, th, tw, full), (8, 11, th, tw, prepost.letterbox_rect(th, tw, H, W)), (h - th, w - tw, th, tw, tiling.view_rect(full, 0.83)),
            (0, 0, h, w, full), (0, 0, h, w, lb), (0, 0, h, w, tiling.view_rect(lb, 0.67)), (0, 0, h, w, tiling.view_rect(full, 0.5)),
            (20, 31, 50, 70, tiling.view_rect(prepost.letterbox_rect(50, 70, H, W), 0.83)), (60, 61, 1, 1, full),
            (h - 1, w - 1, 1, 1, (max(1, H // 3), max(1, W // 5), H // 2, W // 3))]


@pytest.mark.parametrize("hw", [(96, 96), (96, 128), (5, 7)])
def test_view_kernel_is_np_flip_of_the_window_kernel(hw):
    """Flips 0..3 on every row and one table that mixes them; aligned outputs and outputs off by one byte.  5 x 7 takes the
    one-pixel-per-thread store (H * W % 4 != 0)."""
    import torch
    from yolo4hip import ext
    _, eng = GT._eng(3)
    H, W = hw
    lib, dev = eng.lib, eng.device
    img = np.random.default_rng(131173).integers(0, 256, (131, 173, 3), dtype=np.uint8)
    table = _view_table(img.shape[:2], H, W)
    n, pitch = len(table), img.shape[1] * 3
    src = torch.from_numpy(img.reshape(-1)).to(dev)
    wdesc = (ext.y4_window_desc * n)()
    for d, (y0, x0, wh, ww, rect) in zip(wdesc, table):
        d.offset, d.pitch, d.h, d.w = y0 * pitch + x0 * 3, pitch, wh, ww
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
    ref = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=dev)
    ext.check(lib.y4_window_u8_ragged(ext.ptr(src), ext.ptr(GT._desc_tensor(eng, wdesc)), n, ext.ptr(ref), H, W, 77, None))
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    assert (ref == 77).any() and (ref != 77).any()
    for flips in ([0] * n, [1] * n, [2] * n, [3] * n, [(3 * k + 1) % 4 for k in range(n)]):
        vdesc = (ext.y4_view_desc * n)()
        for d, (y0, x0, wh, ww, rect), f in zip(vdesc, table, flips):
            d.offset, d.pitch, d.h, d.w = y0 * pitch + x0 * 3, pitch, wh, ww
            d.out_h, d.out_w, d.pad_top, d.pad_left = rect
            d.flip = f
            d.reserved[0], d.reserved[1] = -1, 0x7fffffff                       # not read
        dd = GT._desc_tensor(eng, vdesc)
        want = np.stack([_flip(ref[k], f) for k, f in enumerate(flips)])
        flat = torch.zeros(n * H * W * 3 + 8, dtype=torch.uint8, device=dev)
        for shift in (4, 1):                                                    # 4-byte aligned, and off by one byte
            flat.zero_()
            ext.check(lib.y4_view_u8_ragged(ext.ptr(src), ext.ptr(dd), n, C.c_void_p(flat.data_ptr() + shift), H, W, 77, None))
            torch.cuda.synchronize()
            got = flat.cpu().numpy()
            assert not got[:shift].any() and not got[shift + n * H * W * 3:].any()
            got = got[shift:shift + n * H * W * 3].reshape(n, H, W, 3)
            for k in range(n):
                assert np.array_equal(got[k], want[k]), (hw, flips[k], shift, k, table[k], int((got[k] != want[k]).sum()))
    if hw == (96, 96):                                                           # the engine's method, at the engine's size
        got = eng.view_u8_ragged(src, dd, n, torch.zeros((n, H, W, 3), dtype=torch.uint8, device=dev), 77).cpu().numpy()
        assert np.array_equal(got, want)


def test_view_kernel_refusals_come_before_any_launch():
    import torch
    from yolo4hip import ext
    _, eng = GT._eng(3)
    lib = eng.lib
    H = W = 96
    src = torch.zeros(4096, dtype=torch.uint8, device=eng.device)
    out = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=eng.device)
    s, o = ext.ptr(src), ext.ptr(out)
    assert lib.y4_view_u8_ragged(None, s, 1, o, H, W, 0, None) == -22
    assert lib.y4_view_u8_ragged(s, None, 1, o, H, W, 0, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 1, None, H, W, 0, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 1, o, H, W, 256, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 1, o, H, W, -1, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 0, o, H, W, 0, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 65536, o, H, W, 0, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 1, o, 0, W, 0, None) == -22
    assert lib.y4_view_u8_ragged(s, s, 3, o, 16384, 16384, 0, None) == -22      # an output of 2^31 bytes or more
    assert b"view_u8_ragged" in lib.y4_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0


# ------------------------------------------------------------------------------------------------ the gathered sequence
def _gathered(eng, heads, group, slot, maps, n_groups, max_slots, group_cap, rule, merge=False, oriented=True):
    """set_heads per chunk -> decode_gather (oriented: y4_decode_gather_views) -> nms_gathered (merged when `merge`): -> (the five
    outputs, cand_count, the scratch's tables as test_gpu_nms_merge._tables reads them)."""
    import torch
    eng.set_nms_rule(*rule)
    eng.set_nms_merge(merge)
    try:
        state = eng.gather_begin(n_groups, max_slots, group_cap)
        g = torch.from_numpy(np.ascontiguousarray(group, np.int32)).to(eng.device)
        s = torch.from_numpy(np.ascontiguousarray(slot, np.int32)).to(eng.device)
        m = torch.from_numpy(np.ascontiguousarray(maps, np.float32).reshape(-1, 4)).to(eng.device)
        for r0 in range(0, len(group), VC.CHUNK):
            n = eng.set_heads([h[r0:r0 + VC.CHUNK] for h in heads])
            eng.decode_gather(state, n, g[r0:r0 + n], s[r0:r0 + n], m[r0:r0 + n], oriented=oriented)
        outs, cnt = eng.nms_gathered(state)
        torch.cuda.synchronize()
        cnt = cnt.cpu().numpy()
        tables = GM._tables(state, max_slots * NBOX, eng.num_classes, np.minimum(cnt, group_cap))
        return [o.cpu().numpy() for o in outs], cnt, tables
    finally:
        eng.set_nms_rule("iou")
        eng.set_nms_merge(False)


def _decoded(eng, heads):
    """The device's own decode of every row, unmapped: boxes [R, nbox, 4] (zero where no candidate lives), scores [R, nbox, C]."""
    bs, ss = [], []
    for r0 in range(0, len(heads[0]), VC.CHUNK):
        b, s = GM._device_tables(eng, [h[r0:r0 + VC.CHUNK] for h in heads])
        bs.append(b); ss.append(s)
    return np.concatenate(bs), np.concatenate(ss)


# ------------------------------------------------------------------------------------------------ 2. positive maps
@pytest.mark.parametrize("ncls,seed,rule", sorted(TC.MARGINS))
def test_oriented_gather_on_positive_maps_writes_the_bits_of_the_plain_gather(ncls, seed, rule):
    _, group, slot, maps, per_group = TC.geometry()
    assert (maps[:, [0, 2]] > 0).all()
    _, eng = GT._eng(ncls)
    args = (eng, TC.heads(ncls, seed), group, slot, maps, len(per_group), max(per_group), 1 << 15, TC.RULES[rule])
    plain, cnt, (tb, ts, _) = _gathered(*args, oriented=False)
    views, cnt2, (tb2, ts2, _) = _gathered(*args, oriented=True)
    GM._same_bits(views, plain, "oriented against plain")
    assert cnt.tolist() == cnt2.tolist() and int(plain[3].sum()) > 0
    GM._same_bits([tb2, ts2], [tb, ts], "the group tables")


# ------------------------------------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize("ncls,geo,rule", sorted(VC.CASES))
def test_oriented_gather_equals_the_oracle(ncls, geo, rule):
    """Merge off: the decisions of the CPU oracle (decoded on the CPU: boxes to 1e-5, the project's bar).  Bit for bit: the group
    tables are views_oracle.map_boxes_oriented of the device's own decode, and the outputs with merge off and on are the NMS and
    merge oracles on those tables."""
    seed = VC.CASES[(ncls, geo, rule)][0]
    rows, group, slot, maps, per_group = VC.geometry(geo)
    _, eng = GT._eng(ncls)
    r = VC.RULES[rule]
    ref = VC.reference(ncls, geo, rule)
    assert ref[5] >= 1e-5
    heads = VC.heads(ncls, geo, seed)
    args = (eng, heads, group, slot, maps, len(per_group), max(per_group), 1 << 15, r)
    plain, cnt, _ = _gathered(*args, merge=False)
    merged, cnt2, (tb, ts, _) = _gathered(*args, merge=True)
    DC.assert_same_detections(plain, ref[:5])
    assert cnt.tolist() == cnt2.tolist() == ref[6].tolist()
    GM._same_bits(merged[1:], plain[1:], "merge on against merge off")
    # the stored boxes: corners in order, and the oriented map of the device's decode bit for bit
    live = ts.any(axis=-1)
    assert (tb[..., 0] <= tb[..., 2])[live].all() and (tb[..., 1] <= tb[..., 3])[live].all()
    db, ds = _decoded(eng, heads)
    flipped_kept = 0
    for g in range(len(per_group)):
        sel = np.nonzero(group == g)[0]
        want = np.zeros_like(tb[g])
        for i in sel:
            t = int(slot[i])
            want[t * NBOX:(t + 1) * NBOX] = VO.map_boxes_oriented(db[i], maps[i])
        want[~live[g]] = 0
        GM._same_bits([tb[g]], [want], f"group {g}: the table against the oriented map of the device's decode")
        o = VO.merged(tb[g:g + 1], ts[g:g + 1], VC.IOU_THR, VC.SCORE_THR, *r)
        print(f"geometry {geo} photo {g}: {int(cnt[g])} candidates, NMS margin {o[5]:.3e}, membership margin {o[6]:.3e}")
        assert o[5] >= 1e-5 and o[6] >= 1e-5
        GM._same_bits([a[g:g + 1] for a in plain], (o[7],) + tuple(o[1:5]), f"merge off, photo {g}")
        GM._same_bits([a[g:g + 1] for a in merged], o[:5], f"merge on, photo {g}")
        v = int(plain[3][g])
        flipped_kept += sum(1 for i in plain[4][g][:v] if (maps[sel][int(i) // NBOX][[0, 2]] < 0).any())
    assert flipped_kept == VC.CASES[(ncls, geo, rule)][3] >= 1
    assert (merged[0] != plain[0]).any(axis=2).sum() >= 1


# ------------------------------------------------------------------------------------------------ 4. witnesses
SHIFT2 = 2.0 / VC.SIZE


def _mirror_heads(axis, lc_b=1.0):
    """Row 0: the witness box of nms_rule_cases (20 x 20 pixels) on a stride-8 cell, (5, 7) for 'lr' and (3, 7) for 'ud'; row 1: the
    same box on the mirrored cell, (5, 4) and (8, 7) (the 96^2 grid has 12 cells a side; the box sits at its cell's centre, so the
    two are 24 and 40 pixels apart on the canvas).  -> (heads, box index of row 0's, box index of row 1's)."""
    y0, x0 = (5, 7) if axis == "lr" else (3, 7)
    gy, gx = (y0, 11 - x0) if axis == "lr" else (11 - y0, x0)
    heads = DC._heads_with(VC.SIZE, 3, 2, [(0, 0, y0, x0, 0, 1, 8.0, 2.0, RC.T_PAIR), (1, 0, gy, gx, 0, 1, 8.0, lc_b, RC.T_PAIR)])
    return heads, 3 * (y0 * 12 + x0), 3 * (gy * 12 + gx)


@pytest.mark.parametrize("axis", ["lr", "ud"])
def test_a_box_and_its_mirror_image_meet_in_the_photo(axis):
    """Slot 1 sees the mirrored canvas; its map mirrors back, two pixels off so that the pair is two boxes and not one.  With the
    mirrored map the two meet (IoU 0.82) and come back once; with slot 1's map left unflipped both survive.  Every stored box
    has its corners in order; y4_decode_gather under the same map stores them crossed, and the merged box collapses."""
    cfg, eng = GT._eng(3)
    heads, box_a, box_b = _mirror_heads(axis)
    mirror = (-1.0, 1.0 + SHIFT2, 1.0, 0.0) if axis == "lr" else (1.0, 0.0, -1.0, 1.0 + SHIFT2)
    maps = np.array([IDENT, mirror], np.float32)
    rule = ("iou", 1.0, False)
    args = (eng, heads, [0, 0], [0, 1], maps, 1, 2, 64, rule)
    plain, cnt, (tb, ts, _) = _gathered(*args)
    assert cnt.tolist() == [2] and plain[3].tolist() == [1] and plain[4][0][0] == box_a
    ref = VO.gathered_nms([(heads, maps)], 3, cfg, VC.SIZE, VC.IOU_THR, VC.SCORE_THR)
    DC.assert_same_detections(plain, ref[:5])
    a, b = tb[0, box_a], tb[0, NBOX + box_b]
    assert a[0] < a[2] and a[1] < a[3] and b[0] < b[2] and b[1] < b[3]
    k = 0 if axis == "lr" else 1
    assert abs(b[k] - a[k] - SHIFT2) < 1e-6 and abs(b[k + 2] - a[k + 2] - SHIFT2) < 1e-6 and abs(b[1 - k] - a[1 - k]) < 1e-6
    # merge on: the oracle's score-weighted mean bit for bit, between the two members, nearer to the better one
    merged, _, _ = _gathered(*args, merge=True)
    o = VO.merged(tb, ts, VC.IOU_THR, VC.SCORE_THR)
    assert o[6] >= 1e-5
    GM._same_bits(plain, (o[7],) + tuple(o[1:5]), "merge off")
    GM._same_bits(merged, o[:5], "merge on")
    m = merged[0][0][0]
    assert a[k] < m[k] < b[k] and a[k + 2] < m[k + 2] < b[k + 2] and m[k] - a[k] < b[k] - m[k]
    # slot 1's map left unflipped: the boxes are apart on the canvas, both survive
    apart, _, _ = _gathered(eng, heads, [0, 0], [0, 1], np.array([IDENT, IDENT], np.float32), 1, 2, 64, rule)
    assert apart[3].tolist() == [2] and apart[4][0][:2].tolist() == [box_a, NBOX + box_b]
    # the plain gather under the mirrored map stores crossed corners.  The pair measure orders corners itself (nms_measure.h), so
    # the pair still meets -- but the merge averages the four stored floats as they are: the low corner of one member with the
    # high corner of the other, a sliver instead of a box.  That is what the swap is for.
    crossed, _, (tc, _, _) = _gathered(*args, merge=True, oriented=False)
    c = tc[0, NBOX + box_b]
    assert c[k] > c[k + 2] and crossed[3].tolist() == [1]
    mc = crossed[0][0][0]
    assert mc[k + 2] - mc[k] < 0.5 * (a[k + 2] - a[k]) < 0.6 * (m[k + 2] - m[k])


# ------------------------------------------------------------------------------------------------ 5. labels follow pixels
TTA_VIEWS = {"default": None, "ud_lrud": ((1.0, "ud"), (0.5, "lrud"))}


def _tta_rows(photos, hw, letterbox, views, drop_flip_of=None):
    """The rows `Engine.predict_tta_device` makes: per photo the full-image row under every view.  drop_flip_of: a flip-bit mask
    removed from the MAP (not the canvas) of every row that has it -- the negative control."""
    from yolo4hip import tiling
    photo, slot, rows = [], [], []
    for p, a in enumerate(photos):
        h, w = a.shape[:2]
        base = tiling.tile_rows(h, w, hw, None, 0.0, True, letterbox)[-1:]
        for t, (win, rect, bits, m) in enumerate(tiling.view_rows(base, views, (h, w), hw)):
            if drop_flip_of and bits & drop_flip_of:
                m = tiling.view_map(h, w, hw[0], hw[1], win, rect, bits & ~drop_flip_of)
            photo.append(p); slot.append(t); rows.append((win, rect, bits, m))
    return photo, slot, rows


def _tta_pieces(eng, cfg, photos, truth, hw, letterbox, views, drop_flip_of=None):
    """The pieces `Engine._rows_device` calls, in its order, with `set_heads` (a detector that boxes every marker on the canvas the
    DEVICE wrote) in place of the forward -> (outputs as numpy, rows, photo of each row)."""
    import torch
    from yolo4hip import ext
    H, W = hw
    photo, slot, rows = _tta_rows(photos, hw, letterbox, views, drop_flip_of)
    R, P, max_slots = len(rows), len(photos), max(slot) + 1
    desc = (ext.y4_view_desc * R)()
    for d, (_, rect, bits, _) in zip(desc, rows):
        d.out_h, d.out_w, d.pad_top, d.pad_left = rect
        d.flip = bits
    extra = np.concatenate([np.asarray([r[3] for r in rows], np.float32).reshape(-1).view(np.int32), np.asarray(photo, np.int32),
                            np.asarray(slot, np.int32)])
    dev, desc_bytes, head = eng._upload_ragged(photos, desc, extra, rows=photo, windows=[r[0] for r in rows])
    tab = dev[desc_bytes:head].view(torch.int32)
    row_map, row_group, row_slot = tab[:4 * R].view(torch.float32).view(R, 4), tab[4 * R:5 * R], tab[5 * R:6 * R]
    state = eng.gather_begin(P, max_slots, max_slots * eng.num_boxes * eng.num_classes)
    step = C.sizeof(ext.y4_view_desc)
    canvas = torch.empty((eng.max_batch, H, W, 3), dtype=torch.uint8, device=eng.device)
    src = C.c_void_p(dev.data_ptr() + head)
    for r0 in range(0, R, eng.max_batch):
        n = min(eng.max_batch, R - r0)
        eng._canvas_launch(eng.lib.y4_view_u8_ragged, src, (C.c_void_p(dev.data_ptr() + r0 * step),), n, canvas, MP.PAD)
        got = canvas[:n].cpu().numpy()
        for i in range(n):
            win, rect, bits, _ = rows[r0 + i]
            assert np.array_equal(got[i], VO.view_host(photos[photo[r0 + i]], win, rect, bits, hw)), (r0 + i, rect, bits)

        def own(i, p, j, r0=r0):                        # a marker of another photo on this row's canvas is an error
            assert p == photo[r0 + i], (r0 + i, p, photo[r0 + i])
            return True

        heads, _, found = MP.detect_markers(got, lambda p: truth[p], hw, 3, cfg["anchors"], cfg["xyscale"], accept=own)
        assert all(len(f) == len(truth[photo[r0 + i]]) for i, f in enumerate(found))      # every view shows every marker
        assert eng.set_heads(heads) == n
        eng.decode_gather(state, n, row_group[r0:r0 + n], row_slot[r0:r0 + n], row_map[r0:r0 + n], oriented=True)
    outs, cnt = eng.nms_gathered(state)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs], rows, photo


def _every_marker_once(outs, rows, photo, photos, truth, nbox, what):
    boxes, scores, classes, valid, kept = outs
    for p, a in enumerate(photos):
        h, w = a.shape[:2]
        mine = [i for i in range(len(rows)) if photo[i] == p]
        hit = []
        for k in range(int(valid[p])):
            box = boxes[p, k].astype(np.float64) * (w, h, w, h)
            j = int(np.argmax([MP.iou(list(box), [float(v) for v in t[:4]]) for t in truth[p]]))
            win, rect, _, _ = rows[mine[int(kept[p, k]) // nbox]]
            assert int(classes[p, k]) == int(truth[p][j][4]), (what, p, k, box, truth[p][j])
            MP.detection_sits_on_marker(box, truth[p][j], rect[1] / win[3], rect[0] / win[2], f"{what} photo {p} box {k}")
            hit.append(j)
        assert sorted(hit) == list(range(len(truth[p]))), (what, p, hit)         # every marker exactly once


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("name", sorted(TTA_VIEWS))
@pytest.mark.parametrize("hw", LC.EVAL_CANVASES)
def test_tta_rows_return_every_marker_once(tmp_path_factory, hw, name, letterbox):
    """One upload of photos, view descriptors and maps; per chunk of max_batch rows y4_view_u8_ragged -> (stand-in) ->
    y4_decode_gather_views; then nms_gathered.  The control: one flip bit dropped from the maps and not from the canvases must fail."""
    from yolo4hip import tiling
    cfg, eng = GL._engine(hw)
    ds = LC.eval_dataset(tmp_path_factory.mktemp("tta_markers"))
    photos, truth = ds["photos"], ds["truth"]
    views = tiling.DEFAULT_VIEWS if TTA_VIEWS[name] is None else TTA_VIEWS[name]
    outs, rows, photo = _tta_pieces(eng, cfg, photos, truth, hw, letterbox, views)
    assert len(rows) == len(photos) * len(views) and len(rows) % GL.MAX_BATCH == (1 if len(views) == 3 else 0)
    what = f"tta {hw} {name} lb={letterbox}"
    _every_marker_once(outs, rows, photo, photos, truth, eng.num_boxes, what)
    for drop in [b for b in (1, 2) if any(r[2] & b for r in rows)]:
        bad, rows2, _ = _tta_pieces(eng, cfg, photos, truth, hw, letterbox, views, drop_flip_of=drop)
        with pytest.raises(AssertionError):
            _every_marker_once(bad, rows2, photo, photos, truth, eng.num_boxes, what + f" flip bit {drop} dropped from the map")


# ------------------------------------------------------------------------------------------------ 6. engine and facade
def _view_canvases(photo, rows, hw):
    return np.stack([VO.view_host(photo, win, rect, bits, hw) for win, rect, bits, _ in rows])


def _against_oracle(m, cfg, got, canvases, maps, what):
    """`got` (with indices) against the oracle on Engine.forward_heads of the host's canvases, in the device's chunking."""
    heads = m.engine.forward_heads(canvases)
    ref = VO.gathered_nms([(heads, maps)], m.num_classes, cfg, GT.FACADE_SIZE, cfg["iou_threshold"], GT.FACADE_SCORE)
    print(f"{what}: oracle min_margin {ref[5]:.3g}, valid {int(ref[3][0])}, candidates {int(ref[6][0])}")
    assert int(ref[3][0]) > 0
    if ref[5] >= 1e-5:
        DC.assert_same_detections(got, ref[:5])
    else:                                                 # near-ties may fall either way: at most 3 % of the positions
        a = set(zip(got[4][0][:got[3][0]].tolist(), got[2][0][:got[3][0]].tolist()))
        b = set(zip(ref[4][0][:ref[3][0]].tolist(), ref[2][0][:ref[3][0]].tolist()))
        assert len(a ^ b) <= 0.03 * max(len(b), 1)
    return ref


def test_facade_identity_view_is_the_plain_path(monkeypatch):
    """(a) views = ((1.0, ''),): inference_model.predict on a photo of the network size; predict_img's letterbox path on 200 x 260."""
    _, m = GT._model()
    S = GT.FACADE_SIZE
    img = GT._photo(S, S, 1)
    ref = m.inference_model.predict(img[None])
    assert int(ref[3].sum()) > 0
    got = m.predict_tta(img, views=((1.0, ""),))
    assert len(got) == 4
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[0].flags.writeable
    monkeypatch.setattr(m, "_letterbox", True)
    photo = GT._photo(200, 260, 2)
    ref = m._predict_mapped(*m._letterboxed([photo]))
    assert int(ref[3].sum()) > 0
    got = m.predict_tta([photo], views=[(1.0, "")])
    for a, b in zip(got, ref):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def test_facade_tta_equals_the_oracle_on_its_own_heads():
    """(b), (e), (f): a 200 x 260 photo under the default views, three rows in one chunk."""
    from yolo4hip import tiling
    cfg, m = GT._model()
    eng = m.engine
    S = GT.FACADE_SIZE
    photo = GT._photo(200, 260, 2)
    rows = tiling.view_rows(tiling.tile_rows(200, 260, (S, S), None, 0.0, True, False)[-1:], tiling.DEFAULT_VIEWS, (200, 260), (S, S))
    got = eng.predict_tta([photo], with_indices=True)
    facade = m.predict_tta(photo)
    for a, b in zip(facade, got[:4]):
        assert np.array_equal(a, b)
    _against_oracle(m, cfg, got, _view_canvases(photo, rows, (S, S)), np.stack([r[3] for r in rows]), "tta facade")
    assert set((got[4][0][:got[3][0]] // eng.num_boxes).tolist()) <= {0, 1, 2}
    again = eng.predict_tta([photo], with_indices=True)                     # (e) the same bits on every run
    for a, b in zip(again, got):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    with pytest.raises(RuntimeError, match="tile_candidates"):               # (f)
        eng.predict_tta([photo], tile_candidates=64, score_threshold=0.0)
    with pytest.raises(RuntimeError, match="tile_candidates"):
        m.predict_tta(photo, tile_candidates=1)
    again = eng.predict_tta([photo], with_indices=True)
    for a, b in zip(again, got):
        assert np.array_equal(a, b)


def test_facade_tiled_views_equal_the_oracle_and_none_is_unchanged():
    """(c) 5 rows x 3 views over four chunks; views=None returns what views=((1.0, ''),) returns."""
    from yolo4hip import tiling
    cfg, m = GT._model()
    eng = m.engine
    S = GT.FACADE_SIZE
    photo = GT._photo(200, 260, 2)
    base = tiling.tile_rows(200, 260, (S, S), None, 0.2, True, False)
    rows = tiling.view_rows(base, tiling.DEFAULT_VIEWS, (200, 260), (S, S))
    assert len(base) == 5 and len(rows) == 15
    got = eng.predict_tiled([photo], with_indices=True, views=tiling.DEFAULT_VIEWS)
    for a, b in zip(m.predict_tiled(photo, views=tiling.DEFAULT_VIEWS), got[:4]):
        assert np.array_equal(a, b)
    _against_oracle(m, cfg, got, _view_canvases(photo, rows, (S, S)), np.stack([r[3] for r in rows]), "tiled views facade")
    assert set((got[4][0][:got[3][0]] // eng.num_boxes).tolist()) <= set(range(15))
    none = eng.predict_tiled([photo], with_indices=True)
    ident = eng.predict_tiled([photo], with_indices=True, views=((1.0, ""),))
    for a, b in zip(none, ident):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert int(none[3][0]) > 0


def test_facade_predict_img_tta_dataframe(capsys):
    """(d)"""
    _, m = GT._model()
    photo = GT._photo(200, 260, 2)
    plain = m.predict_img(photo, plot_img=False)
    det = m.predict_img_tta(photo, plot_img=False)
    assert list(det.columns) == list(plain.columns) == ["x1", "y1", "x2", "y2", "class_name", "score", "w", "h"]
    assert len(det) > 0
    assert (det[["x1", "x2"]].values >= 0).all() and (det[["x1", "x2"]].values <= 260).all()
    assert (det[["y1", "y2"]].values >= 0).all() and (det[["y1", "y2"]].values <= 200).all()
    assert set(det["class_name"]) <= set(m.class_names)
    out, det2 = m.predict_img_tta(photo, plot_img=False, return_output=True, views=((1.0, "lrud"), (0.5, "")))
    assert out.shape == photo.shape and list(det2.columns) == list(det.columns)
    det3 = m.predict_img_tiled(photo, plot_img=False, views=((1.0, ""), (1.0, "ud")))
    assert list(det3.columns) == list(det.columns)
    assert "img shape:" in capsys.readouterr().out


def test_facade_refuses_bad_images_and_bad_views():
    """(g)"""
    _, m = GT._model()
    photo = GT._photo(200, 260, 2)
    for bad in (np.zeros((200, 260, 3), np.float32), [np.zeros((200, 260, 3), np.float64)], np.zeros((200, 260), np.uint8)[..., None], []):
        with pytest.raises(ValueError):
            m.predict_tta(bad)
    for bad in ([], [(1.0, "")] * 2, [(0.0, "")], [(1.5, "lr")], [(float("nan"), "")], [(1.0, "flip")],
                [(1 - 0.05 * k, "") for k in range(17)]):
        for call in (m.predict_tta, m.predict_tiled, m.engine.predict_tta):
            with pytest.raises(ValueError):
                call(photo, views=bad)
        with pytest.raises(ValueError):
            m.predict_img_tta(photo, plot_img=False, views=bad)
    assert int(m.predict_tta(photo)[3][0]) >= 0                               # the engine is usable afterwards


# ------------------------------------------------------------------------------------------------ 7. evaluate_map
def _view_order(n_photos, bs, step, n_views):
    """(photo, view) of every canvas `evaluate_map(views=...)` sends through the forward, in order: batches of bs photos in
    chunks of `step` photos, a photo's views side by side."""
    order = []
    for start in range(0, n_photos, bs):
        for i0 in range(start, min(start + bs, n_photos), step):
            chunk = range(i0, min(i0 + step, start + bs, n_photos))
            order += [(p, v) for p in chunk for v in range(n_views)]
    return order


def _views_stand_in(m, eval_ds, seen, order, rotate_from=None):
    """test_gpu_labels_follow_pixels._stand_in for views: every marker on the canvas the device wrote becomes a head cell.
    rotate_from: {(photo, view): canvas} of an earlier run -- photo p is then served photo p + 1's canvas under the same view."""
    eng = m.engine
    hw = tuple(m.img_size[:2])
    P = len(eval_ds["photos"])

    def forward(imgs_dev):
        canvases = imgs_dev.cpu().numpy()
        assert canvases.dtype == np.uint8
        k0 = len(seen)
        seen.extend(canvases)
        if rotate_from is not None:
            canvases = [rotate_from[((order[k0 + i][0] + 1) % P, order[k0 + i][1])] for i in range(len(canvases))]
        heads, _, _ = MP.detect_markers(canvases, lambda p: eval_ds["truth"][p], hw, 3, m.config["anchors"], m.config["xyscale"])
        assert eng.set_heads(heads) == len(canvases)

    return forward


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("hw", LC.EVAL_CANVASES)
def test_evaluate_map_with_views(tmp_path_factory, hw, letterbox, monkeypatch):
    from yolo4hip import tiling
    m = GL._model(hw)
    monkeypatch.setattr(m, "_letterbox", letterbox)
    eval_ds = LC.eval_dataset(tmp_path_factory.mktemp("eval_views"))
    gen = LC.generator(eval_ds, hw, 3)
    P = len(eval_ds["photos"])
    # the identity view is evaluate_map itself: on the network's own forward, and on the detector that boxes every marker
    assert m.evaluate_map(gen, views=((1.0, ""),)) == m.evaluate_map(gen)
    seen = []
    monkeypatch.setattr(m.engine, "forward_device", GL._stand_in(m, eval_ds, seen))
    plain = m.evaluate_map(gen, bs=3, iou_thresholds=(0.5, 0.75))
    assert m.evaluate_map(gen, bs=3, iou_thresholds=(0.5, 0.75), views=((1.0, ""),)) == plain and plain["mAP"] == 1.0
    # the default views: every canvas is the host restatement's, and every marker comes back once, as a true positive
    views = tiling.DEFAULT_VIEWS
    order = _view_order(P, 3, GL.MAX_BATCH, len(views))
    seen = []
    monkeypatch.setattr(m.engine, "forward_device", _views_stand_in(m, eval_ds, seen, order))
    res = m.evaluate_map(gen, bs=3, iou_thresholds=(0.5, 0.75), views=views)
    assert len(seen) == len(order) == P * len(views)
    for canvas, (p, v) in zip(seen, order):
        photo = eval_ds["photos"][p]
        h, w = photo.shape[:2]
        (win, rect, bits, _), = tiling.view_rows(tiling.tile_rows(h, w, hw, None, 0.0, True, letterbox)[-1:], views[v:v + 1], (h, w), hw)
        assert np.array_equal(canvas, VO.view_host(photo, win, rect, bits, hw)), (p, v)
    n_gt = sum(len(t) for t in eval_ds["truth"])
    print(f"evaluate_map views {hw} letterbox={letterbox}:", {k: res[k] for k in ("mAP", "tp", "fp", "n_gt")}, res["per_threshold"])
    assert sum(res["n_det"].values()) == n_gt and res["mAP"] == 1.0
    for thr in (0.5, 0.75):
        assert res["per_threshold"][thr]["mAP"] == 1.0 and sum(res["per_threshold"][thr]["fp"].values()) == 0
    # the negative control: every photo is served its neighbour's canvas, view by view
    again = []
    monkeypatch.setattr(m.engine, "forward_device",
                        _views_stand_in(m, eval_ds, again, order, rotate_from={pv: c for pv, c in zip(order, seen)}))
    bad = m.evaluate_map(gen, bs=3, iou_thresholds=(0.5, 0.75), views=views)
    print("rotated by one image:", bad["mAP"])
    assert bad["mAP"] < 0.5
    # capacity: one candidate key cannot hold an image
    monkeypatch.setattr(m.engine, "forward_device", _views_stand_in(m, eval_ds, [], order))
    with pytest.raises(RuntimeError, match="tile_candidates"):
        m.evaluate_map(gen, views=views, tile_candidates=1)
