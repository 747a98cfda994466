"""VOC mAP without a GPU: the per-image oracle (tests/map_oracle.py) plus `mapeval.MapAccumulator` over the crafted cases
(tests/map_cases.py) against `evalmap.eval_map` over the text files of the file pipeline, with `==`."""
import json
import os
import types

import numpy as np
import pytest

import map_cases
import map_oracle


def _fmt(v):
    return repr(float(v))


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """The cases as the file pipeline sees them: an annotation file, the ground-truth folder `Yolov4.export_gt` writes from it
    (the method itself, on a stand-in that only has class_names) and the prediction folder in `export_prediction`'s own
    formatting (float32 boxes after `*= w`, float32 scores, one f-string per line)."""
    from yolo4hip.api import Yolov4
    root = tmp_path_factory.mktemp("map")
    gt_dir, pred_dir = str(root / "gt"), str(root / "pred")
    os.makedirs(gt_dir), os.makedirs(pred_dir)
    cases = map_cases.cases()
    ann = str(root / "ann.txt")
    with open(ann, "w") as fh:
        for c in cases:
            objs = [",".join(_fmt(v) for v in row[:4]) + f",{int(row[4])}" for row in c["gt"][:c["gt_count"]]]
            fh.write(" ".join([f"/data/{c['stem']}.jpg"] + objs) + "\n")
    Yolov4.export_gt(types.SimpleNamespace(class_names=map_cases.CLASS_NAMES), ann, gt_dir)
    for c in cases:
        nb = c["valid"]
        boxes = c["boxes"][:nb].copy()
        boxes[:, [0, 2]] *= int(c["scale"][0])
        boxes[:, [1, 3]] *= int(c["scale"][1])
        names = [map_cases.CLASS_NAMES[int(v)] for v in c["classes"][:nb]]
        with open(os.path.join(pred_dir, c["stem"] + ".txt"), "w") as out:
            for j in range(nb):
                b = boxes[j]
                out.write(f'{names[j]} {c["scores"][j]} {b[0]} {b[1]} {b[2]} {b[3]}\n')
    return {"cases": cases, "ann": ann, "gt": gt_dir, "pred": pred_dir, "root": root}


def test_oracle_known_answers():
    """The restated rule on the cases whose answer is known by hand."""
    by = {c["stem"]: c for c in map_cases.cases()}
    thr = map_cases.THRESHOLD_SETS[10]
    tp, best, match, used = map_cases.oracle(by["exact_half"], thr)
    assert best[0] == 0.5 and match[0] == 0 and tp[0] == 1 and used[0] == 1           # TP at 0.5 only
    tp, best, match, used = map_cases.oracle(by["touching"], thr)
    assert best[0] == -1.0 and match[0] == -1 and best[1] == 10 / 190 and match[1] == 1 and not tp.any() and not used.any()
    tp, best, match, used = map_cases.oracle(by["used_best"], (0.5,))
    assert list(match[:2]) == [0, 0] and best[1] == 10000 / 10200 and list(tp[:2]) == [1, 0] and list(used[:2]) == [1, 0]
    tp, best, match, used = map_cases.oracle(by["twins"], (0.5,))
    assert list(match[:2]) == [0, 0] and list(best[:2]) == [1.0, 1.0] and list(tp[:2]) == [1, 0] and list(used[:2]) == [1, 0]
    tp, best, match, used = map_cases.oracle(by["a-b"], (0.5,))
    assert list(tp[:6]) == [1, 1, 1, 0, 0, 0] and list(match[:6]) == [1, 0, 2, 0, 1, 2]     # ties go to the lower slot
    tp, best, match, used = map_cases.oracle(by["a"], (0.5,))
    assert list(tp[:2]) == [1, 0]
    tp, best, match, used = map_cases.oracle(by["no_class_gt"], (0.5,))
    assert list(match[:2]) == [-1, 0] and list(tp[:2]) == [0, 1]
    tp, best, match, used = map_cases.oracle(by["scaled"], (0.5,))
    assert list(match[:3]) == [0, 2, 1] and best[0] == 1.0 and best[1] == 1.0 and best[2] < 1.0
    tp, best, match, used = map_cases.oracle(by["full"], map_cases.THRESHOLD_SETS[16])
    assert by["full"]["valid"] == 100 and by["full"]["gt_count"] == 256
    counts = [int(((tp >> t) & 1).sum()) for t in range(16)]
    assert counts == sorted(counts, reverse=True) and counts[0] > counts[-1] > 0        # the thresholds bite differently


@pytest.mark.parametrize("n_thr", [1, 10, 16])
def test_accumulator_equals_eval_map(dataset, n_thr):
    from yolo4hip import evalmap
    from yolo4hip.mapeval import MapAccumulator
    thresholds = map_cases.THRESHOLD_SETS[n_thr]
    cases = dataset["cases"]
    acc = MapAccumulator(map_cases.CLASS_NAMES, thresholds)
    used_by_stem = {}
    order = list(range(len(cases)))[::-1]                       # fed in another order than the files sort in, in three batches
    for part in (order[:5], order[5:6], order[6:]):
        sel = [cases[i] for i in part]
        boxes, scores, classes, valid, scale, gt, gt_count = map_cases.batch(sel)
        tp = np.stack([map_cases.oracle(c, thresholds)[0] for c in sel])
        for c in sel:
            used_by_stem[c["stem"]] = map_cases.oracle(c, thresholds)[3]
        acc.add([c["stem"] for c in sel], scores, classes, valid, tp, [c["gt"][:c["gt_count"], 4] for c in sel])
    got = acc.result()
    refs = []
    for t, thr in enumerate(thresholds):
        tmp, out = str(dataset["root"] / f"tmp_{n_thr}_{t}"), str(dataset["root"] / f"out_{n_thr}_{t}")
        os.makedirs(tmp), os.makedirs(out)
        ref = evalmap.eval_map(dataset["gt"], dataset["pred"], tmp, out, min_overlap=thr, verbose=False)
        refs.append(ref)
        mine = got["per_threshold"][thr]
        for key in ("mAP", "ap", "tp", "fp"):
            assert mine[key] == ref[key], (thr, key, mine[key], ref[key])
        for key in ("n_gt", "n_images", "n_det"):
            assert got[key] == ref[key], (key, got[key], ref[key])
        for c in cases:                                         # the final `used` flags eval_map leaves behind
            rows = json.load(open(os.path.join(tmp, c["stem"] + "_ground_truth.json")))
            assert len(rows) == c["gt_count"]
            assert [bool(r["used"]) for r in rows] == [bool((int(u) >> t) & 1) for u in used_by_stem[c["stem"]][:len(rows)]], \
                (thr, c["stem"])
    for key in ("mAP", "ap", "tp", "fp"):
        assert got[key] == refs[0][key]
    assert got["mAP_mean"] == sum(r["mAP"] for r in refs) / len(refs)
    assert sorted(got["ap"]) == ["apple", "fig", "kiwi", "pear"] and "date" in got["n_det"] and got["tp"]["date"] == 0
    assert 0.0 < got["mAP"] < 1.0


def test_image_order_is_the_file_order():
    """"a-b.txt" sorts before "a.txt": with equal confidences the stable sort keeps that order, and AP depends on it."""
    from yolo4hip.mapeval import MapAccumulator
    res = []
    for first, second in ((1, 0), (0, 1)):                      # tp flag of "a-b"'s detection, of "a"'s
        acc = MapAccumulator(["x"], (0.5,))
        acc.add(["a", "a-b"], np.array([[0.5], [0.5]], np.float32), np.zeros((2, 1), np.float32), np.array([1, 1], np.int32),
                np.array([[second], [first]], np.uint32), [[0], [0]])
        res.append(acc.result()["ap"]["x"])
    assert res == [0.5, 0.25]                                   # TP first: (1/2) * 1;  FP first: (1/2) * (1/2)


def test_accumulator_and_reader_refusals():
    from yolo4hip.data import read_map_annotations
    from yolo4hip.mapeval import MapAccumulator
    acc = MapAccumulator(["x"], (0.5,))
    one = (np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), np.array([0], np.int32), np.zeros((1, 1), np.uint32), [[0]])
    acc.add(["s"], *one)
    with pytest.raises(ValueError, match="stem"):
        acc.add(["s"], *one)
    with pytest.raises(ValueError):
        MapAccumulator(["x"], ())
    with pytest.raises(ValueError):
        MapAccumulator(["x"], [0.5] * 17)
    with pytest.raises(ValueError, match="no ground-truth"):
        MapAccumulator(["x"], (0.5,)).result()
    items = read_map_annotations(["/d/p.q.jpg 1,2,3.5,4,1 5,6,7,8,0\n", "r.png\n"], 2)
    assert [(name, stem) for name, stem, _ in items] == [("/d/p.q.jpg", "p"), ("r.png", "r")]
    assert items[0][2].dtype == np.float32 and items[0][2].tolist() == [[1, 2, 3.5, 4, 1], [5, 6, 7, 8, 0]]
    assert items[1][2].shape == (0, 5)
    with pytest.raises(ValueError, match="stem"):
        read_map_annotations(["a/x.jpg 1,2,3,4,0\n", "b/x.png\n"], 2)
    with pytest.raises(ValueError, match="class"):
        read_map_annotations(["x.jpg 1,2,3,4,2\n"], 2)
    with pytest.raises(ValueError, match="more than 256"):
        read_map_annotations(["x.jpg " + " ".join(["1,2,3,4,0"] * 257) + "\n"], 2)
    assert len(read_map_annotations(["x.jpg " + " ".join(["1,2,3,4,0"] * 256) + "\n"], 2)[0][2]) == 256


def test_reader_gives_the_cases_back(dataset):
    from yolo4hip.data import read_map_annotations
    items = read_map_annotations(open(dataset["ann"]).readlines(), len(map_cases.CLASS_NAMES))
    for (name, stem, boxes), c in zip(items, dataset["cases"]):
        assert stem == c["stem"] and np.array_equal(boxes, c["gt"][:c["gt_count"]])
