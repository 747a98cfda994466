"""y4_anchor_step / y4_anchor_fitness / y4_anchor_evolve and `fit_anchors` on the GPU against the NumPy oracle (tests/anchors_oracle.py)
with `==` everywhere: lane, wave, workgroup and grid-stride tails in n, k = 1 .. 16, P = 1 .. 65, G = 1 and 5; run-to-run identity;
the refused arguments; the cross-check that the anchor the search gives a box is the one `y4_loss_assign` gives it; and
`Yolov4.rebase_anchors` on the raw heads of two models."""
import os

import numpy as np
import pytest

import anchors_oracle as AO
from helpers import CLASS_DIR

pytestmark = pytest.mark.gpu

NS = [1, 63, 64, 65, 255, 256, 257, 1025, 4099]
KS = [1, 2, 9, 16]
F32 = np.float32


@pytest.fixture(scope="module")
def boxes():
    """n -> the seeded mixture of that size (computed once, never written to)."""
    out = {n: AO.mixture(n, 100 + n) for n in NS}
    for a in out.values():
        a.setflags(write=False)
    return out


def _device(wh):
    from yolo4hip.anchors import _Device
    return _Device(np.ascontiguousarray(wh))


def _sets(wh, k, P, seed):
    """P anchor sets around the start of these boxes, some sides clamped to one pixel."""
    from yolo4hip.anchors import draw_mult
    mult = draw_mult(seed, 1, P, k, sigma=0.4)[0]
    return np.maximum(AO.start(wh, k)[None] * mult, F32(1.0)).astype(F32)


@pytest.mark.parametrize("k", KS)
def test_step_equals_oracle(boxes, k):
    for n in NS:
        wh = boxes[n]
        dev = _device(wh)
        anchors = _sets(wh, k, 1, n + k)[0]
        nxt, stats, assign = dev.step(anchors, with_assign=True)
        rn, rs, ra = AO.step(wh, anchors)
        assert np.array_equal(stats, rs), (n, k, stats, rs)
        assert nxt.tobytes() == rn.tobytes(), (n, k, nxt, rn)
        assert np.array_equal(assign, ra), (n, k)
        nxt2, stats2, none = dev.step(anchors)                     # assign_dev == NULL
        assert none is None and nxt2.tobytes() == rn.tobytes() and np.array_equal(stats2, rs)


@pytest.mark.parametrize("P", [1, 3, 64, 65])
def test_fitness_equals_oracle(boxes, P):
    for n in NS:
        dev = _device(boxes[n])
        for k in KS:
            sets = _sets(boxes[n], k, P, 7 * n + k)
            f = dev.fitness(sets)
            ref = np.array([AO.fitness(boxes[n], s) for s in sets], dtype=np.int64)
            assert f.dtype == np.int64 and np.array_equal(f, ref), (n, k, P, np.nonzero(f != ref)[0][:4])


def test_more_boxes_than_one_pass_of_the_grid():
    """The launches cap the grid at 1024 workgroups: beyond 1024 * 256 boxes (step) and 1024 * 1024 boxes (fitness) a workgroup
    walks several tiles.  Two sizes just past those, with a ragged last tile."""
    wh = AO.mixture((1 << 20) + 1029, 9)
    dev = _device(wh[:(1 << 18) + 77])
    anchors = _sets(wh, 9, 1, 3)[0]
    nxt, stats, assign = dev.step(anchors, with_assign=True)
    rn, rs, ra = AO.step(wh[:(1 << 18) + 77], anchors)
    assert np.array_equal(stats, rs) and nxt.tobytes() == rn.tobytes() and np.array_equal(assign, ra)
    sets = _sets(wh, 2, 17, 4)                                     # two groups of sets: 16 and 1
    assert np.array_equal(_device(wh).fitness(sets), np.array([AO.fitness(wh, s) for s in sets], dtype=np.int64))


# (n, k, P, G, seed of the draw, Lloyd steps before the evolution); the two 20 x 16 cases start from the converged k-means
EVOLVE = [(1, 1, 1, 1, 0, 300), (63, 9, 1, 5, 0, 2), (64, 16, 3, 5, 2, 1), (65, 9, 16, 20, 17, 300), (255, 1, 64, 1, 0, 300),
          (256, 2, 65, 1, 3, 300), (257, 2, 3, 5, 0, 300), (1025, 16, 65, 5, 0, 1), (4099, 9, 16, 20, 0, 300), (4099, 9, 64, 5, 5, 3)]


@pytest.mark.parametrize("case", EVOLVE, ids=lambda c: "n%d-k%d-P%d-G%d" % c[:4])
def test_evolve_equals_oracle(boxes, case):
    from yolo4hip.anchors import draw_mult
    n, k, P, G, seed, steps = case
    wh = boxes[n]
    best, _steps, _conv = AO.lloyd(wh, AO.start(wh, k), steps)
    f0 = AO.fitness(wh, best)
    mult = draw_mult(seed, G, P, k)
    rb, rf, rh, ra = AO.evolve(wh, best, f0, mult)
    if G == 20:                                                    # the oracle alone shows both outcomes
        assert (ra >= 0).any() and (ra < 0).any(), ra
    b, f, hist, acc = _device(wh).evolve(best, f0, mult)
    assert np.array_equal(hist, rh), (case, np.argwhere(hist != rh)[:4])
    assert np.array_equal(acc, ra), (acc, ra)
    assert f == rf and b.tobytes() == rb.tobytes()


@pytest.mark.parametrize("n,seed", [(65, 17), (4099, 0)])
def test_fit_anchors_equals_oracle(boxes, n, seed):
    from yolo4hip.anchors import draw_mult, fit_anchors
    from yolo4hip.config import yolo_config
    wh = boxes[n]
    fit = fit_anchors(wh, generations=20, population=16, seed=seed)
    ref = AO.fit(wh, draw_mult(seed, 20, 16))
    assert (ref["accepted"] >= 0).any() and (ref["accepted"] < 0).any()
    for name in ("anchors", "anchors_kmeans"):
        assert getattr(fit, name).dtype == F32 and getattr(fit, name).tobytes() == ref[name].tobytes(), name
    for name in ("counts", "assign", "f_hist", "accepted"):
        assert np.array_equal(getattr(fit, name), ref[name]), name
    for name in ("fitness", "fitness_kmeans", "avg_iou", "avg_iou_kmeans", "iterations", "converged"):
        assert getattr(fit, name) == ref[name], (name, getattr(fit, name), ref[name])
    assert fit.converged and fit.avg_iou > fit.avg_iou_kmeans and fit.counts.sum() == n
    area = fit.anchors[:, 0] * fit.anchors[:, 1]
    assert np.all(area[1:] >= area[:-1])
    assert fit.avg_iou_of(fit.anchors) == fit.avg_iou
    coco = fit.avg_iou_of(yolo_config["anchors"])
    assert coco == AO.fitness(wh, np.array(yolo_config["anchors"], dtype=F32).reshape(9, 2)) / n / 2.0 ** 30 and coco < fit.avg_iou


def test_fit_anchors_init_iters_and_no_evolution(boxes):
    from yolo4hip.anchors import fit_anchors
    from yolo4hip.config import yolo_config
    wh = boxes[1025]
    init = np.array(yolo_config["anchors"], dtype=F32).reshape(9, 2)
    fit = fit_anchors(wh, iters=3, generations=0, init=init)
    ref = AO.fit(wh, None, iters=3, init=init)
    assert fit.iterations == 3 and not fit.converged and ref["iterations"] == 3 and not ref["converged"]
    assert fit.anchors.tobytes() == ref["anchors"].tobytes() and fit.fitness == ref["fitness"] == fit.fitness_kmeans
    assert np.array_equal(fit.assign, ref["assign"]) and len(fit.accepted) == 0
    for bad in (dict(population=0), dict(population=257), dict(generations=4097), dict(iters=-1), dict(init=init[:8])):
        with pytest.raises(ValueError):
            fit_anchors(wh, **bad)
    for bad in (np.zeros((0, 2), F32), np.array([[1, 0]], F32), np.array([[1, 16385]], F32), np.array([[np.nan, 2]], F32)):
        with pytest.raises(ValueError):
            fit_anchors(bad)


def test_two_runs_give_the_same_bytes(boxes):
    from yolo4hip.anchors import draw_mult
    wh = boxes[4099]
    dev = _device(wh)
    anchors = _sets(wh, 9, 1, 1)[0]
    sets = _sets(wh, 9, 65, 2)
    mult = draw_mult(4, 5, 64)
    f0 = AO.fitness(wh, anchors)
    runs = []
    for _ in range(2):
        nxt, stats, assign = dev.step(anchors, with_assign=True)
        b, f, hist, acc = dev.evolve(anchors, f0, mult)
        runs.append([nxt.tobytes(), stats.tobytes(), assign.tobytes(), dev.fitness(sets).tobytes(), b.tobytes(), f, hist.tobytes(),
                     acc.tobytes()])
    assert runs[0] == runs[1]


def test_every_limit_is_refused_before_a_launch():
    import torch
    from yolo4hip import ext
    lib = ext.load()
    dev = "cuda:0"
    wh = torch.ones((64, 2), dtype=torch.float32, device=dev)
    anc = torch.ones((16, 2), dtype=torch.float32, device=dev)
    nxt = torch.zeros((16, 2), dtype=torch.float32, device=dev)
    stats = torch.full((49,), -7, dtype=torch.int64, device=dev)
    f = torch.full((256,), -7, dtype=torch.int64, device=dev)
    mult = torch.ones((2, 4, 16, 2), dtype=torch.float32, device=dev)
    acc = torch.full((2,), -7, dtype=torch.int32, device=dev)
    p, s, null, EINVAL = ext.ptr, ext.stream_ptr(), None, -22
    off = lambda t, b: t.data_ptr() + b                             # noqa: E731  (a misaligned pointer)

    def step(wh_p=p(wh), n=64, a=p(anc), k=9, nx=p(nxt), st=p(stats)):
        return lib.y4_anchor_step(wh_p, n, a, k, nx, st, null, s)

    def fitness(wh_p=p(wh), n=64, sets=p(anc), P=1, k=9, out=p(f)):
        return lib.y4_anchor_fitness(wh_p, n, sets, P, k, out, s)

    def evolve(wh_p=p(wh), n=64, b=p(anc), fb=p(stats), m=p(mult), G=2, P=4, k=9, h=p(f), a=p(acc)):
        return lib.y4_anchor_evolve(wh_p, n, b, fb, m, G, P, k, h, a, s)

    assert step() == 0 and fitness() == 0
    torch.cuda.synchronize()
    stats.fill_(-7); f.fill_(-7)
    for call in (step, fitness, evolve):
        for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 22) + 1), dict(k=0), dict(k=17), dict(wh_p=null), dict(wh_p=off(wh, 4))):
            assert call(**kw) == EINVAL, (call.__name__, kw)
            assert b"anchor_" in lib.y4_last_error()
    for kw in (dict(a=null), dict(nx=null), dict(st=null), dict(st=off(stats, 4))):
        assert step(**kw) == EINVAL, kw
    for kw in (dict(P=0), dict(P=257), dict(sets=null), dict(out=null), dict(out=off(f, 4))):
        assert fitness(**kw) == EINVAL, kw
    for kw in (dict(P=0), dict(P=257), dict(G=0), dict(G=4097), dict(b=null), dict(fb=null), dict(fb=off(stats, 4)), dict(m=null),
               dict(h=null), dict(h=off(f, 4)), dict(a=null)):
        assert evolve(**kw) == EINVAL, kw
    torch.cuda.synchronize()
    assert int((stats != -7).sum()) == 0 and int((f != -7).sum()) == 0 and int((acc != -7).sum()) == 0      # nothing was launched
    # the limits themselves are accepted
    many = torch.ones((256, 9, 2), dtype=torch.float32, device=dev)
    assert step(k=16) == 0 and step(k=1) == 0 and fitness(P=256, sets=p(many)) == 0
    torch.cuda.synchronize()
    assert f.cpu().tolist() == [64 << 30] * 256                     # 64 unit boxes under a unit anchor: IoU 1 each


def test_search_index_is_the_label_assignment_on_the_device():
    """A 160 x 160, 3-class f32 engine built from fit.config(): 8 images of up to 25 boxes with centres on distinct stride-32 cells;
    every record y4_loss_assign writes carries scale * 3 + anchor == the search's `assign` for that box."""
    import torch
    from yolo4hip.anchors import fit_anchors
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    rng = np.random.default_rng(21)
    n_img, mb, side = 8, 25, 160
    sizes = AO.mixture(n_img * mb, 77, size=150.0).reshape(n_img, mb, 2)
    boxes = np.zeros((n_img, mb, 5), dtype=F32)
    used = []
    for i in range(n_img):
        m = mb if i else 7                                         # image 0 has fewer boxes than max_boxes
        cells = rng.permutation(25)[:m]
        cx, cy = (cells % 5 * 32 + 16).astype(F32), (cells // 5 * 32 + 16).astype(F32)
        x1, y1 = cx - sizes[i, :m, 0] / 2, cy - sizes[i, :m, 1] / 2
        boxes[i, :m] = np.stack([x1, y1, x1 + sizes[i, :m, 0], y1 + sizes[i, :m, 1], rng.integers(0, 3, m).astype(F32)], axis=1)
        used.append(m)
    valid = np.concatenate([np.arange(m) + i * mb for i, m in enumerate(used)])
    flat = boxes.reshape(-1, 5)[valid]
    wh = np.stack([flat[:, 2] - flat[:, 0], flat[:, 3] - flat[:, 1]], axis=1).astype(F32)      # what y4_loss_assign computes
    fit = fit_anchors(wh, generations=5, population=16, seed=1)
    assert len(set(fit.assign.tolist())) >= 6
    eng = Engine(3, fit.config(make_config(side, max_boxes=mb)), max_batch=n_img, dtype="f32")
    rec, cnt, xywh = (t.cpu().numpy() for t in eng.assign_device(torch.from_numpy(boxes).to(eng.device)))
    assert cnt.tolist() == used
    at = 0
    for i, m in enumerate(used):
        where = {(float(xywh[i, j, 0]), float(xywh[i, j, 1])): j for j in range(m)}
        assert len(where) == m
        seen = set()
        for r in rec[i, :m]:
            j = where[(float(r[4:5].view(F32)[0]), float(r[5:6].view(F32)[0]))]
            assert r[6:8].view(F32).tobytes() == wh[at + j].tobytes()
            assert int(r[0]) * 3 + int(r[3]) == int(fit.assign[at + j]), (i, j, r[:4], fit.assign[at + j])
            seen.add(j)
        assert len(seen) == m
        at += m
    eng.close()


def test_rebase_anchors_keeps_the_predicted_boxes():
    """Model A decodes with the old anchors, model B (same weights) with new ones and is rebased: the raw heads are bit-identical
    in every channel but tw / th, and there out_B - out_A is the shift within 2^-23 (|out_A| + |out_B| + |bias_B|) -- one rounding
    of the bias sum plus one of each epilogue add."""
    from yolo4hip import weights as W
    from yolo4hip.anchors import anchor_log_shift
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    names, ncls, side = os.path.join(CLASS_DIR, "bccd_classes.txt"), 3, 160
    old_cfg = make_config(side)
    new = AO.fit(AO.mixture(500, 31, size=150.0), None)["anchors"]
    new_cfg = dict(old_cfg, anchors=[float(v) for v in new.reshape(-1)])
    a = Yolov4(None, names, old_cfg, dtype="f32", max_batch=2, synth_seed=3, tune=False)
    b = Yolov4(None, names, new_cfg, dtype="f32", max_batch=2, synth_seed=3, tune=False)
    imgs = W.synth_images(2, side, seed=5)
    before = b.yolo_model.predict(imgs)
    b.rebase_anchors(old_cfg["anchors"])
    out_a, out_b = a.yolo_model.predict(imgs), b.yolo_model.predict(imgs)
    shift = anchor_log_shift(old_cfg["anchors"], new).astype(np.float64)
    ws_b = W.unflatten(b.plan, b._flat)
    nf = 5 + ncls
    moved = np.zeros(3 * nf, dtype=bool)
    moved[[an * nf + 2 + c for an in range(3) for c in (0, 1)]] = True
    for s, idx in enumerate((93, 101, 109)):
        assert before[s].tobytes() == out_a[s].tobytes()            # the same weights before the rebase
        ha, hb = out_a[s], out_b[s]
        assert ha.dtype == F32 and ha.shape == (2, side // (8 << s), side // (8 << s), 3 * nf)
        assert ha[..., ~moved].tobytes() == hb[..., ~moved].tobytes()
        for an in range(3):
            for c in (0, 1):
                ch = an * nf + 2 + c
                xa, xb = ha[..., ch].astype(np.float64), hb[..., ch].astype(np.float64)
                bound = 2.0 ** -23 * (np.abs(xa) + np.abs(xb) + abs(float(ws_b[idx].bias[ch])))
                err = np.abs((xb - xa) - shift[3 * s + an, c])
                assert np.all(err <= bound), (idx, ch, float(err.max()), float(bound.min()))
                assert np.any(xa != xb)
