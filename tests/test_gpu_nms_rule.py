"""The NMS pair rule on the device (y4_set_nms_rule: DIoU-NMS, class-agnostic suppression) against tests/nms_rule_oracle.py, at
every place nms_kernel evaluates it, with inputs whose witnesses (tests/nms_rule_cases.py, asserted without a GPU in
tests/test_nms_rule_cpu.py) say that the deciding pair is tested there.  Bars: tests/decode_nms_cases.assert_same_detections
(decisions identical, boxes within 1e-5, scores within 1e-6)."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import decode_nms_cases as DC
import nms_rule_cases as RC
import nms_rule_oracle as NR
from decode_nms_cases import _engine, assert_same_detections
from helpers import CLASS_DIR, GOLDEN

pytestmark = pytest.mark.gpu


def _run(eng, heads, **kw):
    n = eng.set_heads(heads)
    return [o.cpu().numpy() for o in eng.decode_nms_device(n, None, **kw)]


def _pair_kept(out, pairs):
    kept = RC.kept_boxes(out)
    return [(a in kept, b in kept) for a, b in pairs]


# ------------------------------------------------------------------------------------------------ 1. DIoU at every place
@pytest.mark.parametrize("beta", [1.0, 0.6])
@pytest.mark.parametrize("place", RC.PLACES)
def test_diou_witness_pair(place, beta):
    """'iou' keeps one box of the same-class witness pair and 'diou' both, wherever the kernel decides the pair; each result is
    the oracle's."""
    assert RC.place_holds(place)
    size, ncls, heads, _, _, pairs = RC.witness_case(place)
    _, eng = _engine(size, ncls, 1)
    got = _run(eng, heads)
    assert_same_detections(got, RC.witness_reference(place, False, "iou", 1.0, False)[:5])
    assert _pair_kept(got, pairs) == [(True, False)] * len(pairs)
    eng.set_nms_rule("diou", beta)
    got = _run(eng, heads)
    ref = RC.witness_reference(place, False, "diou", beta, False)
    assert ref[5] >= 1e-5
    assert_same_detections(got, ref[:5])
    assert _pair_kept(got, pairs) == [(True, True)] * len(pairs)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. random heads
@pytest.mark.parametrize("ncls,seed,rule,margin", RC.RANDOM_CASES)
def test_random_heads(ncls, seed, rule, margin):
    heads, _, _ = RC.random_case(ncls, seed)
    ref = RC.random_reference(ncls, seed, rule)
    print(f"min_margin {ref[5]:.3e}")
    assert ref[5] >= 1e-5 and abs(ref[5] - margin) <= 0.01 * margin      # (the recorded figure, to three digits)
    kind, beta, agn = RC.RULES[rule]
    _, eng = _engine(RC.RANDOM_SIZE, ncls, RC.RANDOM_N)
    eng.set_nms_rule(kind, beta, agn)
    assert_same_detections(_run(eng, heads), ref[:5])
    assert ref[3].sum() > 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. agnostic at every place
@pytest.mark.parametrize("place", RC.PLACES)
def test_agnostic_witness_pair(place):
    """The witness pair with its second box moved to another class: class-aware keeps both, agnostic keeps one."""
    assert RC.place_holds(place, True)
    size, ncls, heads, _, _, pairs = RC.witness_case(place, True)
    _, eng = _engine(size, ncls, 1)
    got = _run(eng, heads)
    assert_same_detections(got, RC.witness_reference(place, True, "iou", 1.0, False)[:5])
    assert _pair_kept(got, pairs) == [(True, True)] * len(pairs)
    eng.set_nms_rule("iou", agnostic=True)
    got = _run(eng, heads)
    assert_same_detections(got, RC.witness_reference(place, True, "iou", 1.0, True)[:5])
    assert _pair_kept(got, pairs) == [(True, False)] * len(pairs)
    eng.set_nms_rule("diou", 0.6, agnostic=True)          # both rules at once: the pair survives again
    got = _run(eng, heads)
    assert_same_detections(got, RC.witness_reference(place, True, "diou", 0.6, True)[:5])
    assert _pair_kept(got, pairs) == [(True, True)] * len(pairs)
    eng.close()


def test_agnostic_capped_candidate_suppresses_nothing():
    """max_per_class = 1 turns class 0's second candidate away; the class-1 box that overlaps it is kept.  Without the cap the
    second candidate is kept and suppresses it."""
    size, ncls, heads, b, s = RC.cap_case()
    for per_class, kept in ((1, [906, 324]), (100, [906, 321])):
        _, eng = _engine(size, ncls, 1, max_per_class=per_class)
        eng.set_nms_rule("iou", agnostic=True)
        ref = NR.combined_nms_rule(b, s, per_class, 100, RC.IOU_THR, RC.SCORE_THR, "iou", 1.0, True)
        got = _run(eng, heads)
        assert_same_detections(got, ref[:5])
        assert list(got[4][0][:2]) == kept and got[3][0] == 2
        eng.close()


# ------------------------------------------------------------------------------------------------ 3b. the rule in a later chunk
def _device_decode(eng, heads, boxes, scores):
    """What the DEVICE's decode stage makes of `heads` (one image): -> (boxes [1, nbox, 4], scores [1, nbox, C]) holding its
    float32 score of every candidate (0 elsewhere) and its unclipped box of every box that has one (the oracle's `boxes`
    elsewhere: NMS never reads those).  Read from the scratch of a gathered decode of one row into one group under the identity
    map (fmaf(x, 1, 0) is x): counters | keys | box table, each part on a 256-byte boundary (runtime.hip, GatherLayout)."""
    import torch
    _, nbox, ncls = scores.shape
    cap = nbox * ncls                                          # can never overflow
    assert eng.set_heads(heads) == 1
    state = eng.gather_begin(1, 1, cap)
    dev = eng.device
    eng.decode_gather(state, 1, torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                      torch.tensor([[1.0, 0.0, 1.0, 0.0]], dtype=torch.float32, device=dev))
    raw = state[1].cpu().numpy()
    up = lambda x: (x + 255) // 256 * 256                      # noqa: E731
    keys_off = up(64 * 4)
    boxes_off = keys_off + up(cap * 8)
    assert raw.size == boxes_off + up(nbox * 16)               # the layout assumed here is the library's
    count = int(raw[:4].view(np.uint32)[0])
    keys = raw[keys_off:keys_off + 8 * count].view(np.uint64)
    ids = ~(keys & np.uint64(0xffffffff)).astype(np.uint32)
    bi, ci = (ids // np.uint32(ncls)).astype(np.int64), (ids % np.uint32(ncls)).astype(np.int64)
    dev_scores = np.zeros_like(scores)
    dev_scores[0, bi, ci] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    dev_boxes = boxes.copy()
    dev_boxes[0, bi] = raw[boxes_off:boxes_off + nbox * 16].view(np.float32).reshape(nbox, 4)[bi]
    return dev_boxes, dev_scores


@functools.lru_cache(maxsize=None)
def _later_chunk_run(name, rule):
    """A LATER_CHUNK_CASES input under its rule on the device (shared by the two tests below): -> (the five outputs, the device's
    decoded boxes and scores)."""
    heads, b, s = DC.chunk_case(name)
    _, eng = _engine(DC.SIZE_CHUNK, 2, 1)
    eng.set_nms_rule(*RC.RULES[rule])
    decoded = _device_decode(eng, heads, b, s)
    got = _run(eng, heads)
    eng.close()
    return got, decoded


@pytest.mark.parametrize("name,rule", RC.LATER_CHUNK_CASES)
def test_rule_goes_on_in_a_later_chunk(name, rule):
    """The stack-and-disjoint images under a non-default rule: the later chunk's sort and wave-0 pass continue from the kept
    lists that the first chunk's pass of that rule left (witness: tests/test_decode_nms_cases_cpu.py).  Against the oracle from
    the raw heads on, decode included: decisions identical -- valid, kept indices and classes on int32 views -- and boxes and
    scores within the project's bars."""
    assert RC.later_chunk_witness(name, rule)["rank"] >= DC.NMS_THREADS
    got, ref = _later_chunk_run(name, rule)[0], RC.later_chunk_reference(name, rule)
    for k in (2, 3, 4):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k].view(np.int32), ref[k].view(np.int32))
    assert_same_detections(got, ref[:5])
    assert got[3][0] == 100


@pytest.mark.parametrize("name,rule", RC.LATER_CHUNK_CASES)
def test_rule_in_a_later_chunk_equals_the_oracle_bit_for_bit(name, rule):
    """The same runs, ALL five outputs equal to the oracle of the rule on int32 views.  The oracle's greedy pass runs on the boxes
    and scores the device's own decode stage computed from the heads (`_device_decode`): the same float32 values nms_kernel read,
    so every bit of the result is the NMS kernel's to get right.  (With the ORACLE's decode in front, 8 to 10 of the 400 box
    words and 10 or 11 of the 100 score words differ in their last bit or two -- the device's expf against NumPy's float32 exp,
    measured on an MI355X with this build and the one before it alike -- which is why that comparison, the test above, has bars.)
    The device's decode is itself held to the oracle's here: the same candidates, values within those bars."""
    _, b, s = DC.chunk_case(name)
    got, (dev_b, dev_s) = _later_chunk_run(name, rule)
    thr = np.float32(RC.SCORE_THR)
    assert np.array_equal(dev_s > thr, s > thr) and (s > thr).sum() > DC.NMS_THREADS
    cand = (s > thr).any(axis=2)
    print(f"device decode against the oracle's: scores {float(np.abs(dev_s - np.where(s > thr, s, 0)).max()):.3e}, "
          f"boxes relative {float((np.abs(dev_b[cand] - b[cand]) / np.abs(b[cand]).max()).max()):.3e}")
    assert np.abs(dev_s - np.where(s > thr, s, 0)).max() < 1e-6
    assert (np.abs(dev_b[cand] - b[cand]) <= 1e-5 * np.maximum(1.0, np.abs(b[cand]))).all()
    kind, beta, agn = RC.RULES[rule]
    ref = NR.combined_nms_rule(dev_b, dev_s, 100, 100, RC.IOU_THR, RC.SCORE_THR, kind, beta, agn)
    assert ref[5] >= 1e-6 and ref[3][0] == 100
    assert RC.rank_of_last_kept_under(dev_s[0], ref) >= DC.NMS_THREADS
    for what, g, r in zip(("boxes", "scores", "classes", "valid", "kept"), got, ref[:5]):
        print(f"{what}: {int((g.view(np.int32) != r.view(np.int32)).sum())} of {g.size} words differ")
    for k in (2, 3, 4, 0, 1):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), ("output", k)


# ------------------------------------------------------------------------------------------------ 4. state
def test_rule_is_handle_state_and_the_default_is_restored_bit_for_bit():
    heads, _, _ = RC.random_case(3, 3)
    _, eng = _engine(RC.RANDOM_SIZE, 3, RC.RANDOM_N)
    first = _run(eng, heads)
    eng.set_nms_rule("diou", 0.6)
    middle = _run(eng, heads)
    eng.set_nms_rule("iou")
    third = _run(eng, heads)
    for a, b in zip(first, third):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert not np.array_equal(first[4], middle[4])
    eng.close()


def test_get_nms_rule_round_trips_and_bad_values_are_refused():
    from yolo4hip import ext
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    _, eng = _engine(96, 2, 1)

    def get():
        k, b, a = C.c_int(-1), C.c_float(-1.0), C.c_int(-1)
        ext.check(eng.lib.y4_get_nms_rule(eng.handle, C.byref(k), C.byref(b), C.byref(a)))
        return k.value, b.value, a.value
    assert get() == (0, 1.0, 0)
    assert (eng.nms_kind, eng.nms_agnostic) == ("iou", False)
    ext.check(eng.lib.y4_set_nms_rule(eng.handle, 1, 0.6, 1))
    assert get() == (1, float(np.float32(0.6)), 1)
    eng.set_nms_rule("diou", 2.5)
    assert get() == (1, 2.5, 0) and (eng.nms_kind, eng.nms_beta, eng.nms_agnostic) == ("diou", 2.5, False)
    sib = eng.sibling()                                   # a sibling takes its parent's rule
    k, b, a = C.c_int(), C.c_float(), C.c_int()
    ext.check(sib.lib.y4_get_nms_rule(sib.handle, C.byref(k), C.byref(b), C.byref(a)))
    assert (k.value, b.value, a.value) == (1, 2.5, 0)
    sib.close()
    for bad in ((2, 1.0, 0), (-1, 1.0, 0), (1, 0.0, 0), (1, -0.6, 0), (1, float("nan"), 0), (1, float("inf"), 0), (0, -1.0, 0),
                (0, 1.0, 2), (1, 0.6, -1)):
        assert eng.lib.y4_set_nms_rule(eng.handle, *bad) == -22, bad        # Y4_EINVAL
        assert get() == (1, 2.5, 0)                        # ... and nothing changed
    assert eng.lib.y4_get_nms_rule(eng.handle, None, None, None) == -22
    for kw in ({"kind": "giou"}, {"kind": "diou", "beta": 0.0}, {"kind": "diou", "beta": float("nan")}, {"kind": "iou", "beta": -1.0},
               {"kind": "iou", "agnostic": 2}):
        with pytest.raises(ValueError):
            eng.set_nms_rule(**kw)
    eng.close()
    for kw in ({"nms_kind": "ciou"}, {"nms_beta": 0.0}, {"nms_kind": "diou", "nms_beta": float("inf")}):
        with pytest.raises(ValueError):
            Engine(2, make_config(96), max_batch=1, dtype="bf16", **kw)
        with pytest.raises(ValueError):
            Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(96), max_batch=1, **kw)


# ------------------------------------------------------------------------------------------------ 5. mapped
def test_mapped_output_keeps_the_decisions_of_the_rule():
    import torch
    heads, _, _ = RC.random_case(3, 6)
    ref = RC.random_reference(3, 6, "diou06")
    _, eng = _engine(RC.RANDOM_SIZE, 3, RC.RANDOM_N)
    eng.set_nms_rule("diou", 0.6)
    plain = _run(eng, heads)
    assert_same_detections(plain, ref[:5])
    maps = np.array([[1.25, -0.125, 1.0, 0.0], [1.0, 0.0, 1.6, -0.3]], np.float32)      # (ax, bx, ay, by) per image
    mapped = _run(eng, heads, box_map=torch.from_numpy(maps).to(eng.device))
    for k in (1, 2, 3, 4):
        assert np.array_equal(mapped[k].view(np.int32), plain[k].view(np.int32))
    # the boxes: the oracle's UNCLIPPED kept boxes through the map, then the clip
    _, b, _ = RC.random_case(3, 6)
    changed = 0
    for i in range(RC.RANDOM_N):
        v = int(plain[3][i])
        raw = b[i, plain[4][i, :v]].astype(np.float64)
        ax, bx, ay, by = (float(x) for x in maps[i])
        want = np.clip(np.stack([raw[:, 0] * ax + bx, raw[:, 1] * ay + by, raw[:, 2] * ax + bx, raw[:, 3] * ay + by], axis=1), 0.0, 1.0)
        assert np.abs(mapped[0][i, :v] - want).max() < 1e-5
        assert not mapped[0][i, v:].any()
        changed += int((np.abs(mapped[0][i, :v] - plain[0][i, :v]) > 1e-3).sum())
    assert changed > 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. facade
TINY = (160, 3, 1, 8)                                      # tests/golden/make_golden.py TINY[1]: size, classes, batch, seed


def _three_classes(tmp_path):
    path = str(tmp_path / "three_classes.txt")
    with open(path, "w") as fh:
        fh.write("a\nb\nc\n")
    return path


def test_facade_runs_the_rule_also_after_load_model(tmp_path):
    """Yolov4(nms_kind='diou', nms_agnostic=True) on the tiny net of tests/golden/tiny_net.npz (its seeded weights and image):
    inference_model.predict is the engine-level call with that rule, bit for bit, before and after load_model; and that is the
    oracle's result for the rule on the device's own heads, which differs from the default rule's."""
    from golden.make_golden import TINY as ALL
    from yolo4hip import weights as W
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    assert TINY in ALL
    size, ncls, n, seed = TINY
    cfg = make_config(size)
    imgs = W.synth_images(n, size, seed)
    # the engine-level call: the engine of a default-rule model (same weights, same schedule source), switched by hand
    d = Yolov4(None, _three_classes(tmp_path), cfg, dtype="f32", max_batch=n, synth_seed=seed, tune=False)
    eng = d.engine
    assert (eng.nms_kind, eng.nms_agnostic) == ("iou", False)
    eng.set_nms_rule("diou", 0.6, True)
    want = eng.predict(imgs)
    heads = eng.forward_heads(imgs)
    b, s = DC.boxes_and_scores(heads, ncls, cfg, size)
    ref = NR.combined_nms_rule(b, s, 100, 100, cfg["iou_threshold"], cfg["score_threshold"], "diou", 0.6, True)
    plain = NR.combined_nms_rule(b, s, 100, 100, cfg["iou_threshold"], cfg["score_threshold"], "iou", 1.0, False)
    assert ref[5] >= 1e-5 and ref[3][0] > 0 and not np.array_equal(ref[4], plain[4])
    assert_same_detections(eng.predict(imgs, with_indices=True), ref[:5])
    eng.close()
    m = Yolov4(None, _three_classes(tmp_path), cfg, dtype="f32", max_batch=n, synth_seed=seed, tune=False,
               nms_kind="diou", nms_agnostic=True)
    assert (m.nms_kind, m.nms_beta, m.nms_agnostic) == ("diou", 0.6, True)
    got = m.inference_model.predict(imgs)
    for a, w in zip(got, want):
        assert np.array_equal(a.view(np.int32), w.view(np.int32))
    ckpt = str(tmp_path / "tiny.ckpt")
    m.save_model(ckpt)
    m.load_model(ckpt)                                     # rebuilds inference_model with the default thresholds (the config's here)
    again = m.inference_model.predict(imgs)
    for a, w in zip(again, want):
        assert np.array_equal(a.view(np.int32), w.view(np.int32))
    m.engine.close()


def test_evaluate_map_with_the_rule_equals_the_file_pipeline(tmp_path):
    """evaluate_map of a model with a non-default rule against export_prediction + eval_map of the SAME model (the construction
    of tests/test_gpu_evaluate_map.py, reused)."""
    from test_gpu_evaluate_map import THRESHOLDS, _file_pipeline, _ground_truth_from, _precondition
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    root = tmp_path
    imgdir, pred, gt = (str(root / d) for d in ("img", "pred", "gt"))
    for d in (imgdir, pred, gt):
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
    m = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2, tune=False, nms_kind="diou", nms_agnostic=True)
    m.export_prediction(ann0, pred, imgdir, bs=2)
    ann = str(root / "ann.txt")
    counts = []
    with open(ann, "w") as fh:
        for k, name in enumerate(names):
            dets = []
            for line in open(os.path.join(pred, f"s{k}.txt")).read().splitlines():
                cls, _conf, x1, y1, x2, y2 = line.split(" ")
                dets.append((m.class_names.index(cls), float(x1), float(y1), float(x2), float(y2)))
            counts.append(len(dets))
            fh.write(" ".join([f"/data/{name}"] + [",".join(str(v) for v in row) for row in _ground_truth_from(dets, k)]) + "\n")
    assert sum(counts) >= 9
    m.export_gt(ann, gt)
    p = {"model": m, "root": root, "imgdir": imgdir, "pred": pred, "gt": gt, "ann": ann}
    n, _ = _precondition(p)
    got = m.evaluate_map(ann, imgdir, bs=2, iou_thresholds=THRESHOLDS, channel_order="bgr")
    for t, thr in enumerate(THRESHOLDS):
        ref = _file_pipeline(p, thr, f"rule{t}")
        for key in ("mAP", "ap", "tp", "fp"):
            assert got["per_threshold"][thr][key] == ref[key], (thr, key, got["per_threshold"][thr][key], ref[key])
        for key in ("n_gt", "n_images", "n_det"):
            assert got[key] == ref[key], (key, got[key], ref[key])
    assert sum(got["n_det"].values()) == n
    # the rule was in force: the default model detects another number of boxes on the same images
    d = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2, tune=False)
    pred_d = str(root / "pred_default")
    os.makedirs(pred_d)
    d.export_prediction(ann0, pred_d, imgdir, bs=2)
    counts_d = [len(open(os.path.join(pred_d, f"s{k}.txt")).read().splitlines()) for k in range(3)]
    print(f"detections per image: rule {counts}, default {counts_d}")
    assert counts != counts_d
    m.engine.close(), d.engine.close()
