"""Tiled inference without a GPU: the host geometry (yolo4hip/tiling.py), the tiled oracle (tests/tiled_oracle.py) and the
witnesses of the cases the GPU tests run (tests/tiled_cases.py)."""
import numpy as np
import pytest

import decode_nms_cases as DC
import nms_rule_oracle as NR
import tiled_cases as TC
import tiled_oracle as TO

SIDES = [(1, 96), (95, 96), (96, 96), (97, 96), (200, 96), (260, 96), (120, 96), (1000, 96), (4000, 608), (3000, 608), (31, 7), (64, 1)]
OVERLAPS = [0.0, 0.2, 0.25, 0.5, 0.9, 0.999]


@pytest.mark.parametrize("L,t", SIDES)
@pytest.mark.parametrize("overlap", OVERLAPS)
def test_windows_cover_the_side_and_end_flush(L, t, overlap):
    from yolo4hip.tiling import window_starts
    starts = window_starts(L, t, overlap)
    if L <= t:
        assert starts == [0]
        return
    assert starts[0] == 0 and starts[-1] == L - t                      # the last window is flush with the edge
    assert all(0 <= s and s + t <= L for s in starts)                  # all inside
    assert all(b > a for a, b in zip(starts, starts[1:]))
    covered = np.zeros(L, bool)
    for s in starts:
        covered[s:s + t] = True
    assert covered.all()
    need = int(np.floor(t * overlap))
    assert all(a + t - b >= need for a, b in zip(starts, starts[1:]))   # neighbours share at least floor(t * overlap) pixels


def test_issue_geometry():
    from yolo4hip.tiling import tile_windows, window_starts
    assert window_starts(200, 96, 0.25) == [0, 72, 104] and window_starts(260, 96, 0.25) == [0, 72, 144, 164]
    assert window_starts(120, 96, 0.25) == [0, 24] and window_starts(96, 96, 0.25) == [0]
    wins = tile_windows(200, 260, (96, 96), 0.25)
    assert len(wins) == 12 and wins[0] == (0, 0, 96, 96) and wins[1] == (0, 72, 96, 96) and wins[-1] == (104, 164, 96, 96)
    _, group, slot, _, per_group = TC.geometry()
    assert per_group == [13, 3] and group.tolist() == [0] * 13 + [1] * 3 and slot.tolist() == list(range(13)) + [0, 1, 2]


def test_small_image_gives_one_window():
    from yolo4hip.tiling import tile_rows, tile_windows
    assert tile_windows(50, 70, (96, 96), 0.2) == [(0, 0, 50, 70)]
    assert tile_windows(96, 96, (96, 96), 0.2) == [(0, 0, 96, 96)]
    assert tile_windows(50, 200, (96, 96), 0.0) == [(0, 0, 50, 96), (0, 96, 50, 96), (0, 104, 50, 96)]
    rows = tile_rows(96, 96, (96, 96), None, 0.2, full_image=False, letterbox=False)
    assert len(rows) == 1 and rows[0][0] == (0, 0, 96, 96) and rows[0][1] == (96, 96, 0, 0)
    assert rows[0][2].tolist() == [1.0, 0.0, 1.0, 0.0]                 # a 1:1 window of a network-size photo: the identity, exactly


@pytest.mark.parametrize("overlap", [-0.1, 1.0, 1.5, float("nan")])
def test_bad_overlap_raises(overlap):
    from yolo4hip.tiling import tile_rows, window_starts
    with pytest.raises(ValueError):
        window_starts(200, 96, overlap)
    with pytest.raises(ValueError):
        tile_rows(200, 260, (96, 96), None, overlap)


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("h,w,canvas,tile", [(200, 260, (96, 96), None), (96, 120, (96, 96), None), (131, 173, (96, 160), (50, 70)),
                                             (3000, 4000, (608, 608), None), (300, 90, (96, 96), (128, 64))])
def test_map_sends_the_rectangle_to_the_window(h, w, canvas, tile, letterbox):
    """The composed map takes the corners of a row's canvas rectangle (canvas-normalised) to the corners of its window
    (photo-normalised) within 1e-6, and the full-image row's map is prepost.box_map."""
    from yolo4hip import prepost
    from yolo4hip.tiling import tile_rows
    H, W = canvas
    rows = tile_rows(h, w, canvas, tile, 0.2, full_image=True, letterbox=letterbox)
    for (y0, x0, wh, ww), (out_h, out_w, top, left), m in rows:
        assert m.dtype == np.float32 and m.shape == (4,)
        assert 0 <= y0 and y0 + wh <= h and 0 <= x0 and x0 + ww <= w
        assert 0 <= top and top + out_h <= H and 0 <= left and left + out_w <= W
        if letterbox:
            assert (out_h, out_w, top, left) == prepost.letterbox_rect(wh, ww, H, W)
        else:
            assert (out_h, out_w, top, left) == (H, W, 0, 0)
        m = m.astype(np.float64)
        for xc, xp in ((left / W, x0 / w), ((left + out_w) / W, (x0 + ww) / w)):
            assert abs(xc * m[0] + m[1] - xp) < 1e-6
        for yc, yp in ((top / H, y0 / h), ((top + out_h) / H, (y0 + wh) / h)):
            assert abs(yc * m[2] + m[3] - yp) < 1e-6
    win, rect, m = rows[-1]
    assert win == (0, 0, h, w)
    assert np.array_equal(m, prepost.box_map(h, w, H, W, rect))
    assert len(tile_rows(h, w, canvas, tile, 0.2, full_image=False, letterbox=letterbox)) == len(rows) - 1


def test_oracle_of_one_row_is_the_rule_oracle():
    """One group, one slot, the identity map: the tiled oracle is combined_nms_rule on that row."""
    from yolo4hip.config import make_config
    cfg = make_config(TC.SIZE)
    hd = [h[5:6] for h in TC.heads(3, 0)]
    ident = np.array([[1.0, 0.0, 1.0, 0.0]], np.float32)
    b, s = DC.boxes_and_scores(hd, 3, cfg, TC.SIZE)
    for kind, beta, agn in TC.RULES.values():
        got = TO.gathered_nms([(hd, ident)], 3, cfg, TC.SIZE, TC.IOU_THR, TC.SCORE_THR, kind, beta, agn)
        ref = NR.combined_nms_rule(b, s, 100, 100, TC.IOU_THR, TC.SCORE_THR, kind, beta, agn)
        for a, r in zip(got[:5], ref[:5]):
            assert np.array_equal(a, r)
        assert got[5] == ref[5] and got[6].tolist() == [int((s > np.float32(TC.SCORE_THR)).sum())]


def test_oracle_maps_before_the_measure():
    """Two rows whose boxes coincide only after their maps: the tiled oracle suppresses one, and keeps both under maps that
    leave them apart."""
    from yolo4hip.config import make_config
    import nms_rule_cases as RC
    cfg = make_config(TC.SIZE)
    hd = DC._heads_with(TC.SIZE, 3, 2, [(0, 0, 5, 7, 0, 1, 8.0, 2.0, RC.T_PAIR), (1, 0, 5, 3, 0, 1, 8.0, 1.0, RC.T_PAIR)])
    shift = 5 * 8 / TC.SIZE                    # five stride-8 cells: cell 3 -> cell 8, next to cell 7 (IoU 12/28 = 0.4286)
    together = np.array([[1, 0, 1, 0], [1, shift, 1, 0]], np.float32)
    apart = np.array([[1, 0, 1, 0], [1, 0, 1, 0]], np.float32)
    assert TO.gathered_nms([(hd, together)], 3, cfg, TC.SIZE, TC.IOU_THR, TC.SCORE_THR)[3].tolist() == [1]
    assert TO.gathered_nms([(hd, apart)], 3, cfg, TC.SIZE, TC.IOU_THR, TC.SCORE_THR)[3].tolist() == [2]


@pytest.mark.parametrize("ncls,seed,rule", sorted(TC.MARGINS))
def test_recorded_margins_hold(ncls, seed, rule):
    ref = TC.reference(ncls, seed, rule)
    margin = TC.MARGINS[(ncls, seed, rule)]
    assert ref[5] >= 1e-5 and ref[5] >= TC.MIN_MARGIN and abs(ref[5] - margin) <= 0.01 * margin
    nbox = 3 * sum((TC.SIZE // s) ** 2 for s in (8, 16, 32))
    assert ref[3].tolist() == [100, 100]                               # the oracle keeps 100 boxes per group ...
    assert TC.kept_slots(ref, 0, nbox) == set(range(13))               # ... group 0's from all 13 slots
    big, small = {3: ((3900, 4150), (800, 950)), 80: ((12200, 12450), (2700, 2950))}[ncls]      # candidates per group
    assert big[0] <= ref[6][0] <= big[1] and small[0] <= ref[6][1] <= small[1]
    assert ref[6][0] > DC.NMS_THREADS and (ncls == 3 or ref[6][0] > DC.SORT_CAP + DC.NMS_THREADS)


def test_abi_of_the_new_entry_points_host_only():
    """The descriptor's layout, and y4_gather_scratch_bytes -- pure host work -- with its refusals, without a GPU."""
    import ctypes as C
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    assert C.sizeof(ext.y4_window_desc) == 40 and ext.y4_window_desc.pitch.offset == 8 and ext.y4_window_desc.h.offset == 12
    lib = ext.load()
    h = C.c_void_p()
    ext.check(lib.y4_create(C.byref(_cfg_struct(make_config(96), 80, 4, "bf16")), C.byref(h)))
    nbox, nbytes = 3 * (144 + 36 + 9), C.c_size_t()
    up = lambda x: (x + 255) // 256 * 256
    for groups, slots, cap in ((1, 1, 1), (2, 13, 1 << 15), (3, 5, 1000)):
        ext.check(lib.y4_gather_scratch_bytes(h, groups, slots, cap, C.byref(nbytes)))
        assert nbytes.value == up(groups * 256) + up(groups * cap * 8) + up(groups * slots * nbox * 16)
    limit = (1 << 31) // (nbox * 80)                                   # the largest max_slots with slots * nbox * C < 2^31
    assert lib.y4_gather_scratch_bytes(h, 1, limit, 64, C.byref(nbytes)) == 0
    assert lib.y4_gather_scratch_bytes(h, 1, limit + 1, 64, C.byref(nbytes)) == -22 and b"2^31" in lib.y4_last_error()
    for bad in ((0, 1, 64), (1, 0, 64), (1, 1, 0), (-1, 1, 64)):
        assert lib.y4_gather_scratch_bytes(h, *bad, C.byref(nbytes)) == -22
    assert lib.y4_gather_scratch_bytes(h, 1, 1, 64, None) == -22
    assert lib.y4_gather_scratch_bytes(None, 1, 1, 64, C.byref(nbytes)) == -22
    assert lib.y4_decode_gather(h, 1, -1.0, None, None, None, 1, 1, 64, None, None) != 0      # workspace not bound: refused
    assert lib.y4_window_u8_ragged(None, None, 1, None, 96, 96, 128, None) == -22
    lib.y4_destroy(h)
