"""Merge-NMS on the device (y4_decode_nms_merged, y4_nms_gathered_merged; box_merge.hip) against tests/merge_oracle.py on the
cases of tests/merge_cases.py (margins and witnesses asserted without a GPU in tests/test_nms_merge_cpu.py).

Every comparison with the oracle is BIT FOR BIT on all five outputs.  The oracle runs on the candidate list and the box table the
device's own decode stage produced -- read back from the scratch of a gathered decode, where nms_kernel and box_merge_kernel read
them -- so every bit of a result is the NMS and merge kernels' to get right (the device's expf differs from NumPy's in the last
bit of some boxes, which is why the project compares decodes with bars, tests/test_gpu_nms_rule.py).  On those tables the oracle's
smallest membership margin is asserted to be >= 1e-5 again."""
import functools
import os
import shutil

import numpy as np
import pytest

import decode_nms_cases as DC
import merge_cases as MC
import merge_oracle as MO
import nms_rule_cases as RC
import tiled_cases as TC
from helpers import CLASS_DIR, GOLDEN

pytestmark = pytest.mark.gpu

IDENT = (1.0, 0.0, 1.0, 0.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(got, want, what=""):
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), \
            (what, "output", k, int((_bits(g) != _bits(w)).sum()), "words differ of", g.size)


def _tables(state, rows_nbox, ncls, counts=None):
    """The groups' candidate lists and box tables as the kernels read them, from the scratch of a gathered decode (counters, one
    per 256-byte line | keys [G][cap] | boxes [G][rows_nbox][4], each part on a 256-byte boundary: runtime.hip, GatherLayout).
    counts: the groups' candidate counts when an NMS has consumed the counters already.
    -> (boxes [G, rows_nbox, 4] (zero where no candidate lives), scores [G, rows_nbox, C] (zero likewise), counts)."""
    (G, _, cap), scratch = state
    raw = scratch.cpu().numpy()
    up = lambda x: (x + 255) // 256 * 256                      # noqa: E731
    keys_off = up(G * 64 * 4)
    boxes_off = keys_off + up(G * cap * 8)
    assert raw.size == boxes_off + up(G * rows_nbox * 16)
    if counts is None:
        counts = raw[:G * 256].view(np.uint32).reshape(G, 64)[:, 0].astype(np.int64)
    assert (np.asarray(counts) <= cap).all()
    boxes = np.zeros((G, rows_nbox, 4), np.float32)
    scores = np.zeros((G, rows_nbox, ncls), np.float32)
    for g in range(G):
        keys = raw[keys_off + g * cap * 8:keys_off + (g * cap + int(counts[g])) * 8].view(np.uint64)
        ids = ~(keys & np.uint64(0xffffffff)).astype(np.uint32)
        bi, ci = (ids // np.uint32(ncls)).astype(np.int64), (ids % np.uint32(ncls)).astype(np.int64)
        assert len(set(ids.tolist())) == len(ids)
        scores[g, bi, ci] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
        table = raw[boxes_off + g * rows_nbox * 16:boxes_off + (g + 1) * rows_nbox * 16].view(np.float32).reshape(rows_nbox, 4)
        boxes[g, bi] = table[bi]
    return boxes, scores, np.asarray(counts)


def _device_tables(eng, heads):
    """What the device's decode stage makes of `heads`: one group per image under the identity map (fmaf(x, 1, 0) is x)."""
    import torch
    n = eng.set_heads(heads)
    state = eng.gather_begin(n, 1, eng.num_boxes * eng.num_classes)
    dev = eng.device
    eng.decode_gather(state, n, torch.arange(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                      torch.tensor([IDENT] * n, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    return _tables(state, eng.num_boxes, eng.num_classes)[:2]


def _run(eng, n, merge, **kw):
    eng.set_nms_merge(merge)
    try:
        return [o.cpu().numpy() for o in eng.decode_nms_device(n, None, **kw)]
    finally:
        eng.set_nms_merge(False)


def _plain_entry(eng, n, box_map=None):
    """y4_decode_nms / y4_decode_nms_mapped called directly: today's entry points."""
    from yolo4hip import ext
    b, s, c, v, k = outs = eng.alloc_outputs(n)
    args = (ext.ptr(b), ext.ptr(s), ext.ptr(c), ext.ptr(v), ext.ptr(k), ext.stream_ptr())
    if box_map is None:
        ext.check(eng.lib.y4_decode_nms(eng.handle, n, -1.0, -1.0, *args))
    else:
        ext.check(eng.lib.y4_decode_nms_mapped(eng.handle, n, -1.0, -1.0, ext.ptr(box_map), *args))
    return [o.cpu().numpy() for o in outs]


def _check_against_oracle(eng, heads, rule="iou", per_class=100, total=100, maps=None):
    """Decode tables -> oracle; merge off and on on the same heads.  -> (merged outputs, plain outputs, oracle result)."""
    import torch
    kind, beta, agn = MC.RULES[rule]
    eng.set_nms_rule(kind, beta, agn)
    dev_b, dev_s = _device_tables(eng, heads)
    n = dev_b.shape[0]
    bm = None if maps is None else torch.from_numpy(np.ascontiguousarray(maps, np.float32)).to(eng.device)
    kw = {} if bm is None else {"box_map": bm}
    plain = _run(eng, n, False, **kw)
    merged = _run(eng, n, True, **kw)
    ref = MO.merged_nms(dev_b, dev_s, per_class, total, MC.IOU_THR, MC.SCORE_THR, kind, beta, agn, box_maps=maps)
    print(f"oracle on the device's tables: NMS margin {ref[5]:.3e}, membership margin {ref[6]:.3e}, valid {ref[3].tolist()}, "
          f"boxes moved {int((ref[0] != ref[7]).any(axis=2).sum())}")
    assert ref[6] >= 1e-5 and ref[5] >= 1e-6
    _same_bits(plain, (ref[7],) + tuple(ref[1:5]), "merge off")
    _same_bits(merged, ref[:5], "merge on")
    _same_bits(merged[1:], plain[1:], "merge on against merge off")             # (b): only the boxes change
    _same_bits(_plain_entry(eng, n, bm), plain, "merge off against the plain entry point")
    for i in range(n):
        assert not merged[0][i, int(merged[3][i]):].any()
    return merged, plain, ref


# ------------------------------------------------------------------------------------------------ (a), (b) random heads
@pytest.mark.parametrize("ncls,seed,rule,margin", MC.RANDOM_CASES)
def test_random_heads_equal_the_oracle_bit_for_bit(ncls, seed, rule, margin):
    heads, _, _ = RC.random_case(ncls, seed)
    _, eng = DC._engine(RC.RANDOM_SIZE, ncls, RC.RANDOM_N)
    merged, plain, ref = _check_against_oracle(eng, heads, rule)
    assert (merged[0] != plain[0]).any(axis=2).sum() >= 20
    eng.close()


def test_merge_is_engine_state_siblings_carry_it_and_bad_values_are_refused():
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    heads, _, _ = RC.random_case(3, 3)
    _, eng = DC._engine(RC.RANDOM_SIZE, 3, RC.RANDOM_N)
    assert eng.nms_merge is False
    n = eng.set_heads(heads)
    first = [o.cpu().numpy() for o in eng.decode_nms_device(n)]
    eng.set_nms_merge(True)
    assert eng.nms_merge is True
    sib = eng.sibling()
    assert sib.nms_merge is True
    middle = [o.cpu().numpy() for o in eng.decode_nms_device(n)]
    n = sib.set_heads(heads)
    _same_bits([o.cpu().numpy() for o in sib.decode_nms_device(n)], middle, "sibling")
    eng.set_nms_merge(False)
    _same_bits([o.cpu().numpy() for o in eng.decode_nms_device(n)], first, "off again")
    assert not np.array_equal(first[0], middle[0])
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError):
            eng.set_nms_merge(bad)
        with pytest.raises(ValueError):
            Engine(2, make_config(96), max_batch=1, dtype="bf16", nms_merge=bad)
    assert eng.nms_merge is False
    sib.close()
    eng.close()


def test_null_outputs_are_refused_before_any_launch():
    import torch
    from yolo4hip import ext
    heads, _, _ = RC.random_case(3, 3)
    _, eng = DC._engine(RC.RANDOM_SIZE, 3, RC.RANDOM_N)
    n = eng.set_heads(heads)
    b, s, c, v, k = (ext.ptr(o) for o in eng.alloc_outputs(n))
    cnt = torch.full((n,), -7, dtype=torch.int32, device=eng.device)
    lib, h = eng.lib, eng.handle
    assert lib.y4_decode_nms_merged(h, n, -1.0, -1.0, None, None, b, s, c, v, k, None) == -22
    assert lib.y4_decode_nms_merged(h, n, -1.0, -1.0, None, ext.ptr(cnt), b, s, c, v, None, None) == -22      # kept_idx is required
    assert lib.y4_decode_nms_merged(h, n, -1.0, -1.0, None, ext.ptr(cnt), None, s, c, v, k, None) == -22
    assert lib.y4_decode_nms_merged(h, n + 1, -1.0, -1.0, None, ext.ptr(cnt), b, s, c, v, k, None) == -22
    state = eng.gather_begin(1, 1, 64)
    sp = ext.ptr(state[1])
    assert lib.y4_nms_gathered_merged(h, 1, 1, 64, -1.0, sp, ext.ptr(cnt), b, s, c, v, None, None) == -22
    assert lib.y4_nms_gathered_merged(h, 1, 1, 64, -1.0, sp, None, b, s, c, v, k, None) == -22
    assert lib.y4_nms_gathered_merged(h, 1, 1, 1 << 25, -1.0, sp, ext.ptr(cnt), b, s, c, v, k, None) == -22   # capacity the sums do not cover
    assert b"2^25" in lib.y4_last_error()
    torch.cuda.synchronize()
    assert cnt.tolist() == [-7] * n
    # the cand_count output of the plain path: the images' raw candidate counts
    _, dev_s = _device_tables(eng, heads)
    o = eng.alloc_outputs(n)
    ext.check(lib.y4_decode_nms_merged(h, n, -1.0, -1.0, None, ext.ptr(cnt), *(ext.ptr(t) for t in o), ext.stream_ptr()))
    assert cnt.tolist() == [int((dev_s[i] > 0).sum()) for i in range(n)]
    eng.close()


# ------------------------------------------------------------------------------------------------ (c) later chunks
@pytest.mark.parametrize("name,total", MC.CHUNK_CASES)
def test_members_behind_the_first_chunk_move_their_kept_box(name, total):
    """The stack of a chunk case: its kept box absorbs a thousand candidates ranked behind the first 1024 keys -- with max_total =
    55 candidates NMS never visited, because it had its boxes (witness: tests/test_nms_merge_cpu.py, and again here on the
    device's tables)."""
    heads, _, _ = DC.chunk_case(name)
    _, eng = DC._engine(DC.SIZE_CHUNK, 2, 1, max_total=total)
    merged, plain, ref = _check_against_oracle(eng, heads, "iou", 100, total, MC.CHUNK_MAP)
    dev_b, dev_s = _device_tables(eng, heads)
    w = MC.chunk_witness(dev_b, dev_s, ref, total)
    k = w["slot"]
    assert (w["member_ranks"] >= DC.NMS_THREADS).sum() > 100
    if total == 55:
        assert w["last_kept"] < DC.NMS_THREADS and (w["member_ranks"] > w["last_kept"]).sum() > 1000
    assert np.abs(merged[0][0][k] - w["head_only"]).max() > 1e-4
    assert np.abs(merged[0][0][k] - plain[0][0][k]).max() > 1e-2
    assert merged[3][0] == total
    eng.close()


# ------------------------------------------------------------------------------------------------ (d) caps
@pytest.mark.parametrize("name,per_class,total", MC.CAP_CASES)
def test_caps_turn_candidates_away_and_the_merge_absorbs_them(name, per_class, total):
    size, ncls, heads, _, _ = DC.cap_input(name)
    _, eng = DC._engine(size, ncls, 1, max_per_class=per_class, max_total=total)
    merged, plain, ref = _check_against_oracle(eng, heads, "iou", per_class, total)
    assert merged[3][0] == total and (merged[0] != plain[0]).any()
    assert merged[0].shape == (1, total, 4)
    eng.close()


def test_a_candidate_its_class_cap_turned_away_is_absorbed_under_an_agnostic_rule():
    """nms_rule_cases.cap_case with max_per_class = 1 under an agnostic rule: class 0's second candidate (box 321) is turned
    away, the class-1 box beside it (324) is kept and absorbs it -- its x1 moves towards 321; slots >= valid are zero."""
    size, ncls, heads, _, _ = RC.cap_case()
    _, eng = DC._engine(size, ncls, 1, max_per_class=1)
    merged, plain, ref = _check_against_oracle(eng, heads, "agn_iou", 1, 100)
    assert merged[4][0][:2].tolist() == [906, 324] and merged[3][0] == 2
    assert merged[0][0][1][0] < plain[0][0][1][0] - 0.01 and np.array_equal(merged[0][0][0], plain[0][0][0])
    assert not merged[0][0][2:].any() and not merged[1][0][2:].any() and (merged[4][0][2:] == -1).all()
    eng.close()


# ------------------------------------------------------------------------------------------------ (e) box map
def test_with_a_box_map_the_order_is_mean_then_map_then_clip():
    heads, _, _ = RC.random_case(3, 3)
    _, eng = DC._engine(RC.RANDOM_SIZE, 3, RC.RANDOM_N)
    merged, plain, ref = _check_against_oracle(eng, heads, "iou", maps=MC.MAPS)
    unmapped = _run(eng, eng.set_heads(heads), True)
    _same_bits(merged[1:], unmapped[1:], "the map changes boxes only")
    for i in range(RC.RANDOM_N):
        v = int(merged[3][i])
        assert ((merged[0][i, :v] == 0) | (merged[0][i, :v] == 1)).any()
        assert (merged[0][i, :v] != unmapped[0][i, :v]).any(axis=1).sum() >= v // 2
    eng.close()


# ------------------------------------------------------------------------------------------------ (f) gathered
NBOX = 3 * sum((TC.SIZE // s) ** 2 for s in (8, 16, 32))


@functools.lru_cache(maxsize=None)
def _eng96(ncls):
    return DC._engine(TC.SIZE, ncls, TC.CHUNK)


def _gathered(eng, heads, group, slot, maps, n_groups, max_slots, group_cap, rule, merge):
    """set_heads per chunk -> decode_gather -> nms_gathered (merged when `merge`): -> (outputs, cand_count, the scratch's tables)."""
    import torch
    eng.set_nms_rule(*rule)
    eng.set_nms_merge(merge)
    try:
        state = eng.gather_begin(n_groups, max_slots, group_cap)
        g = torch.from_numpy(np.ascontiguousarray(group, np.int32)).to(eng.device)
        s = torch.from_numpy(np.ascontiguousarray(slot, np.int32)).to(eng.device)
        m = torch.from_numpy(np.ascontiguousarray(maps, np.float32).reshape(-1, 4)).to(eng.device)
        for r0 in range(0, len(group), TC.CHUNK):
            n = eng.set_heads([h[r0:r0 + TC.CHUNK] for h in heads])
            eng.decode_gather(state, n, g[r0:r0 + n], s[r0:r0 + n], m[r0:r0 + n])
        outs, cnt = eng.nms_gathered(state)
        torch.cuda.synchronize()
        cnt = cnt.cpu().numpy()
        tables = _tables(state, max_slots * NBOX, eng.num_classes, np.minimum(cnt, group_cap))
        return [o.cpu().numpy() for o in outs], cnt, tables
    finally:
        eng.set_nms_rule("iou")
        eng.set_nms_merge(False)


def test_one_object_seen_by_two_slots_comes_back_as_their_weighted_mean():
    """Row 0 carries the witness box of nms_rule_cases on stride-8 cell (5, 7), row 1 the same box on cell (5, 3) with a lower
    score; row 1's map shifts it by four cells and two pixels, so in the photo the two overlap with IoU 0.82: one is kept -- row
    0's -- and its merged box lies between the two rows' boxes, equal to neither."""
    _, eng = _eng96(3)
    heads = DC._heads_with(TC.SIZE, 3, 2, [(0, 0, 5, 7, 0, 1, 8.0, 2.0, RC.T_PAIR), (1, 0, 5, 3, 0, 1, 8.0, 1.0, RC.T_PAIR)])
    maps = np.array([IDENT, (1.0, (4 * 8 + 2) / TC.SIZE, 1.0, 0.0)], np.float32)
    rule = ("iou", 1.0, False)
    plain, cnt, (tb, ts, _) = _gathered(eng, heads, [0, 0], [0, 1], maps, 1, 2, 64, rule, False)
    merged, cnt2, _ = _gathered(eng, heads, [0, 0], [0, 1], maps, 1, 2, 64, rule, True)
    assert cnt.tolist() == cnt2.tolist() == [2] and plain[3].tolist() == [1]
    box_a, box_b = 3 * (5 * 12 + 7), NBOX + 3 * (5 * 12 + 3)
    assert plain[4][0][0] == box_a
    ref = MO.merged_nms(tb, ts, 100, 100, MC.IOU_THR, MC.SCORE_THR)
    assert ref[6] >= 1e-5
    _same_bits(plain, (ref[7],) + tuple(ref[1:5]), "merge off")
    _same_bits(merged, ref[:5], "merge on")
    a, b, m = tb[0, box_a], tb[0, box_b], merged[0][0][0]
    assert a[0] < m[0] < b[0] and a[2] < m[2] < b[2] and abs(b[0] - a[0] - 2 / TC.SIZE) < 1e-6
    assert not np.array_equal(m, np.clip(a, 0, 1)) and not np.array_equal(m, np.clip(b, 0, 1))
    # the weights are the scores: the mean lies nearer to row 0's box
    assert m[0] - a[0] < b[0] - m[0]


@pytest.mark.parametrize("ncls,seed,rule,margin", MC.TILED_CASES)
def test_gathered_merge_equals_the_oracle_over_the_group_list(ncls, seed, rule, margin):
    """The 16 rows of tiled_cases in two photos: the merged boxes equal the oracle over each photo's whole list, as the scratch
    holds it, bit for bit; three repeated calls -- the list's order varies from run to run -- give identical bits."""
    _, group, slot, maps, per_group = TC.geometry()
    _, eng = _eng96(ncls)
    r = TC.RULES[rule]
    args = (eng, TC.heads(ncls, seed), group, slot, maps, len(per_group), max(per_group), 1 << 15, r)
    plain, cnt, _ = _gathered(*args, False)
    merged, cnt2, (tb, ts, _) = _gathered(*args, True)
    assert cnt.tolist() == cnt2.tolist()
    _same_bits(merged[1:], plain[1:], "merge on against merge off")
    assert (merged[0] != plain[0]).any(axis=2).sum() >= 10
    for g in range(len(per_group)):
        ref = MO.merged_nms(tb[g:g + 1], ts[g:g + 1], 100, 100, TC.IOU_THR, TC.SCORE_THR, *r)
        print(f"photo {g}: {int(cnt[g])} candidates, NMS margin {ref[5]:.3e}, membership margin {ref[6]:.3e}")
        assert ref[6] >= 1e-5 and ref[5] >= 1e-6
        _same_bits([o[g:g + 1] for o in plain], (ref[7],) + tuple(ref[1:5]), f"merge off, photo {g}")
        _same_bits([o[g:g + 1] for o in merged], ref[:5], f"merge on, photo {g}")
    for _ in range(2):
        again, _, _ = _gathered(*args, True)
        _same_bits(again, merged, "repeated call")


def test_a_group_over_its_capacity_is_still_reported():
    _, group, slot, maps, per_group = TC.geometry()
    _, eng = _eng96(3)
    ref = TC.reference(3, 0, "iou")
    got, cnt, _ = _gathered(eng, TC.heads(3, 0), group, slot, maps, len(per_group), max(per_group), 64, TC.RULES["iou"], True)
    assert cnt.tolist() == ref[6].tolist() and (cnt > 64).all()
    b, s, c, v, k = got
    assert ((0 <= v) & (v <= 100)).all() and b.min() >= 0.0 and b.max() <= 1.0 and np.isfinite(b).all()


# ------------------------------------------------------------------------------------------------ (g) facade
FACADE_SIZE, FACADE_SCORE = 160, 0.05


@functools.lru_cache(maxsize=None)
def _models():
    """The tiny synthetic net of tests/test_gpu_tiled.py (bccd classes, 160^2, fp32, max_batch 4, score threshold lowered so that
    the untrained net keeps boxes), once without and once with nms_merge."""
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg = dict(make_config(FACADE_SIZE))
    cfg["score_threshold"] = FACADE_SCORE
    cls = os.path.join(CLASS_DIR, "bccd_classes.txt")
    off = Yolov4(None, cls, cfg, dtype="f32", max_batch=4)
    on = Yolov4(None, cls, cfg, dtype="f32", max_batch=4, nms_merge=True)
    return cfg, off, on


def _photo(h, w, seed):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _boxes_differ_only(on, off):
    assert int(off[3].sum()) > 0
    for k in (1, 2, 3):
        assert np.array_equal(_bits(on[k]), _bits(off[k]))
    assert not np.array_equal(on[0], off[0])


def test_facade_keyword_reaches_every_prediction_path(tmp_path):
    from yolo4hip import weights as W
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg, off, on = _models()
    assert (off.nms_merge, off.engine.nms_merge, on.nms_merge, on.engine.nms_merge) == (False, False, True, True)
    imgs = W.synth_images(3, FACADE_SIZE, 4)
    _boxes_differ_only(on.inference_model.predict(imgs), off.inference_model.predict(imgs))
    photo = _photo(200, 260, 2)
    _boxes_differ_only(on.predict_tiled(photo), off.predict_tiled(photo))
    d_on, d_off = on.predict_img(photo, plot_img=False), off.predict_img(photo, plot_img=False)
    assert len(d_on) == len(d_off) > 0
    assert list(d_on["class_name"]) == list(d_off["class_name"]) and np.array_equal(d_on["score"].values, d_off["score"].values)
    assert not np.array_equal(d_on[["x1", "y1", "x2", "y2"]].values, d_off[["x1", "y1", "x2", "y2"]].values)
    t_on, t_off = on.predict_img_tiled(photo, plot_img=False), off.predict_img_tiled(photo, plot_img=False)
    assert len(t_on) == len(t_off) > 0 and np.array_equal(t_on["score"].values, t_off["score"].values)
    # the engine-level call with the flag set by hand gives the facade's bits; after a checkpoint round trip too
    off.engine.set_nms_merge(True)
    try:
        want = off.engine.predict(imgs)
    finally:
        off.engine.set_nms_merge(False)
    for a, b in zip(on.inference_model.predict(imgs), want):
        assert np.array_equal(_bits(a), _bits(b))
    ckpt = str(tmp_path / "tiny.ckpt")
    on.save_model(ckpt)
    on.load_model(ckpt)
    assert on.engine.nms_merge is True
    for a, b in zip(on.engine.predict(imgs), want):
        assert np.array_equal(_bits(a), _bits(b))
    # the capacity contract of predict_tiled is unchanged
    with pytest.raises(RuntimeError, match="tile_candidates"):
        on.engine.predict_tiled([photo], tile_candidates=64, score_threshold=0.0)
    _boxes_differ_only(on.predict_tiled(photo), off.predict_tiled(photo))
    # the pipelined path takes the merged entry as well
    frames = (imgs * 255.0).round().astype(np.uint8)
    s_on, s_off = list(on.engine.predict_stream([frames], in_flight=2)), list(off.engine.predict_stream([frames], in_flight=2))
    _boxes_differ_only(s_on[0], s_off[0])
    for bad in (1, "on", None):
        with pytest.raises(ValueError):
            Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(96), max_batch=1, nms_merge=bad)


def test_facade_evaluate_map_runs_merged(tmp_path):
    """evaluate_map of a nms_merge=True model equals export_prediction + eval_map of the SAME model (the file pipeline of
    tests/test_gpu_evaluate_map.py), counts the detections the nms_merge=False model counts, and its boxes are the merged ones:
    the prediction files of the two models hold the same classes and scores and other coordinates."""
    from test_gpu_evaluate_map import THRESHOLDS, _file_pipeline, _ground_truth_from, _precondition
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    root = tmp_path
    imgdir, pred, gt, pred_off = (str(root / d) for d in ("img", "pred", "gt", "pred_off"))
    for d in (imgdir, pred, gt, pred_off):
        os.makedirs(d)
    names = [f"s{k}.jpeg" for k in range(3)]
    for name in names:
        shutil.copy(os.path.join(GOLDEN, "street.jpeg"), os.path.join(imgdir, name))
    ann0 = str(root / "ann0.txt")
    with open(ann0, "w") as fh:
        fh.write("".join(f"/data/{name}\n" for name in names))
    cfg = make_config(160)
    cfg["batch_size"] = 2
    cls_path = os.path.join(CLASS_DIR, "bccd_classes.txt")
    m = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2, tune=False, nms_merge=True)
    d = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2, tune=False)
    m.export_prediction(ann0, pred, imgdir, bs=2)
    d.export_prediction(ann0, pred_off, imgdir, bs=2)
    moved = 0
    for k in range(3):
        a = [line.split(" ") for line in open(os.path.join(pred, f"s{k}.txt")).read().splitlines()]
        b = [line.split(" ") for line in open(os.path.join(pred_off, f"s{k}.txt")).read().splitlines()]
        assert [r[:2] for r in a] == [r[:2] for r in b] and len(a) > 0
        moved += sum(1 for x, y in zip(a, b) if x[2:] != y[2:])
    assert moved > 0
    ann = str(root / "ann.txt")
    with open(ann, "w") as fh:
        for k, name in enumerate(names):
            dets = []
            for line in open(os.path.join(pred, f"s{k}.txt")).read().splitlines():
                cls, _conf, x1, y1, x2, y2 = line.split(" ")
                dets.append((m.class_names.index(cls), float(x1), float(y1), float(x2), float(y2)))
            fh.write(" ".join([f"/data/{name}"] + [",".join(str(v) for v in row) for row in _ground_truth_from(dets, k)]) + "\n")
    m.export_gt(ann, gt)
    p = {"model": m, "root": root, "imgdir": imgdir, "pred": pred, "gt": gt, "ann": ann}
    n, _ = _precondition(p)
    got = m.evaluate_map(ann, imgdir, bs=2, iou_thresholds=THRESHOLDS, channel_order="bgr")
    for t, thr in enumerate(THRESHOLDS):
        ref = _file_pipeline(p, thr, f"merge{t}")
        for key in ("mAP", "ap", "tp", "fp"):
            assert got["per_threshold"][thr][key] == ref[key], (thr, key, got["per_threshold"][thr][key], ref[key])
        for key in ("n_gt", "n_images", "n_det"):
            assert got[key] == ref[key], (key, got[key], ref[key])
    assert sum(got["n_det"].values()) == n
    plain = d.evaluate_map(ann, imgdir, bs=2, iou_thresholds=THRESHOLDS, channel_order="bgr")
    assert plain["n_det"] == got["n_det"]
    m.engine.close(), d.engine.close()
