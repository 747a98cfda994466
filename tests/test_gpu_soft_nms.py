"""Soft-NMS on the device (y4_set_nms_soft; soft_nms.hip) against tests/soft_nms_oracle.py on the inputs of tests/soft_nms_cases.py
(witnesses and margins asserted without a GPU in tests/test_soft_nms_cpu.py).

The oracle runs on the candidate list and the box table the device's own decode stage produced (read back from the scratch of a
gathered decode, as tests/test_gpu_nms_merge.py does), so every difference is the NMS kernel's.  Bars: kept ids, classes, valid and
order ==; boxes bit-equal to the decoded boxes clipped; scores within the per-score bound the float64 face derives (0 for a score
that was never decayed: bit-equal).  'hard' against the kernel that ships: all five outputs bit for bit."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import decode_nms_cases as DC
import merge_oracle as MO
import nms_rule_cases as RC
import soft_nms_cases as SC
import soft_nms_oracle as SO
import tiled_cases as TC
from helpers import CLASS_DIR, GOLDEN
from test_gpu_nms_merge import IDENT, _device_tables, _gathered, _same_bits

pytestmark = pytest.mark.gpu

HARD = ("hard", "iou", 1.0, False)


def _mode(mode):
    return SC.MODES[mode] if isinstance(mode, str) else mode


def _set(eng, mode, sigma=SC.SIGMA, min_score=None, top_k=SC.TOP_K_MAX):
    method, kind, beta, agn = _mode(mode)
    eng.set_nms_rule(kind, beta, agn)
    eng.set_nms_soft(method, sigma, min_score, top_k)


def _run(eng, heads, **kw):
    n = eng.set_heads(heads)
    return [o.cpu().numpy() for o in eng.decode_nms_device(n, None, **kw)]


def _oracle(dev_b, dev_s, mode, caps=None, iou_thr=SC.IOU_THR, sigma=SC.SIGMA, min_score=None, top_k=SC.TOP_K_MAX, face="f64"):
    caps = caps or {}
    method, kind, beta, agn = _mode(mode)
    return SO.soft_nms(dev_b, dev_s, caps.get("max_per_class", 100), caps.get("max_total", 100), iou_thr, SC.SCORE_THR, kind, beta,
                       agn, method, sigma, min_score, top_k, face)


def _assert_is_oracle(got, ref, what=""):
    """Decisions ==, boxes bit-equal, scores within the derived per-score bound (relative) of the float64 face."""
    for k in (3, 4, 2):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, "output", k, got[k], ref[k])
    assert np.array_equal(got[0].view(np.int32), ref[0].view(np.int32)), (what, "boxes")
    err = np.abs(got[1].astype(np.float64) - ref[1])
    tol = ref[6] * ref[1]
    print(f"{what}: valid {ref[3].tolist()}, margin {ref[5]:.3e}, decayed results {int((ref[6] > 0).sum())}, "
          f"largest score error {float((err / np.maximum(ref[1], 1e-30)).max()):.3e} (largest bound {float(ref[6].max()):.3e})")
    assert (err <= tol).all(), (what, "scores", float((err - tol).max()))
    for i in range(len(got[3])):                               # non-increasing, zero / -1 padded
        v = int(got[3][i])
        assert (np.diff(got[1][i, :v]) <= 0).all() and not got[1][i, v:].any() and (got[4][i, v:] == -1).all()


def _check(eng, heads, mode, caps=None, what="", **soft):
    """`heads` under `mode` on the device against the oracle on the device's decode tables -> (device outputs, oracle result)."""
    _set(eng, mode, **{k: v for k, v in soft.items() if k != "iou_thr"})
    dev_b, dev_s = _device_tables(eng, heads)
    kw = {"iou_threshold": soft["iou_thr"]} if "iou_thr" in soft else {}
    got = _run(eng, heads, **kw)
    ref = _oracle(dev_b, dev_s, mode, caps, **soft)
    assert ref[5] >= SC.MARGIN_BAR, (what, ref[5])
    _assert_is_oracle(got, ref, what)
    return got, ref


def _witness(name, mode="gauss_iou", **soft):
    size, ncls, heads, b, s, caps, wsoft = SC.witness(name)
    _, eng = DC._engine(size, ncls, 1, **caps)
    got, ref = _check(eng, heads, mode, caps, name, **dict(wsoft, **soft))
    eng.close()
    v = int(got[3][0])
    return [int(x) for x in got[4][0][:v]], [int(x) for x in got[2][0][:v]], got[1][0][:v], got


BI = lambda gy, gx: SC.box_index(SC.SIZE, gy, gx)      # noqa: E731


def _gauss(m):
    return float(np.exp(-m * m / SC.SIGMA))


# ------------------------------------------------------------------------------------------------ 1. witnesses
def test_witness_order_is_by_current_score():
    ids, _, sc, _ = _witness("order")
    assert ids == [BI(5, 4), BI(1, 9), BI(5, 5)] and abs(float(sc[2]) - 0.8 * _gauss(0.6)) < 2e-4


def test_witness_two_kept_boxes_decay_in_pick_order():
    ids, _, sc, _ = _witness("two_factors")
    f37, f19 = _gauss(3.0 / 7.0), _gauss(1.0 / 9.0)
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)]
    assert np.allclose(sc, [0.9, 0.85 * f19, 0.7 * f37 * f37], atol=2e-4)


def test_witness_classes_and_agnostic():
    ids, cls, sc, got = _witness("classes")
    assert ids == [BI(5, 4), BI(5, 5), BI(1, 9)] and cls == [1, 2, 1] and abs(float(sc[1]) - 0.8) < 2e-4
    ids, cls, sc, _ = _witness("classes", "gauss_iou_agn")
    assert ids == [BI(5, 4), BI(1, 9), BI(5, 5)] and cls == [1, 1, 2] and abs(float(sc[2]) - 0.8 * _gauss(0.6)) < 2e-4


def test_witness_floor_shrinks_valid():
    ids, _, _, got = _witness("floor")
    assert ids == [BI(5, 4), BI(1, 9)] and got[3][0] == 2


def test_witness_turned_away_decays_nothing():
    ids, cls, sc, _ = _witness("turned_away", "gauss_iou_agn")
    assert ids == [BI(1, 1), BI(8, 5)] and cls == [0, 1] and abs(float(sc[1]) - 0.7) < 2e-4


def test_witness_max_total_and_empty():
    ids, _, _, got = _witness("max_total")
    assert ids == [BI(1, 1), BI(5, 5)] and got[3][0] == 2 and got[4].shape == (1, 2)
    ids, _, _, got = _witness("empty")
    assert ids == [] and got[3][0] == 0 and not got[0].any() and not got[1].any() and not got[2].any() and (got[4] == -1).all()


def test_witness_ties_by_box_then_class():
    ids, cls, sc, _ = _witness("ties")
    boxes = sorted(BI(gy, gx) for gy, gx in ((7, 2), (1, 9), (4, 4), (1, 3)))
    assert ids == [b for b in boxes for _ in (0, 1)] and cls == [0, 2] * 4 and len(set(sc.tolist())) == 1


def test_witness_linear_at_exactly_the_threshold_does_not_decay():
    import nms_rule_oracle as NR
    size, ncls, heads, _, _, caps, _ = SC.witness("order")
    _, eng = DC._engine(size, ncls, 1)
    dev_b, dev_s = _device_tables(eng, heads)
    m = NR.measure(dev_b[0, BI(5, 5)], dev_b[0, [BI(5, 4)]], "iou", 1.0, np.float32)[0]      # the device's float32 IoU of the pair
    assert abs(float(m) - 0.6) < 1e-5
    lin = ("linear", "iou", 1.0, False)
    _set(eng, lin)
    at = _run(eng, heads, iou_threshold=float(m))
    assert at[4][0][:3].tolist() == [BI(5, 4), BI(5, 5), BI(1, 9)] and at[1][0][1] == dev_s[0, BI(5, 5), 1]
    _assert_is_oracle(at, _oracle(dev_b, dev_s, lin, iou_thr=float(m)), "at the threshold")
    below = _run(eng, heads, iou_threshold=float(np.nextafter(m, np.float32(0))))
    assert below[4][0][:3].tolist() == [BI(5, 4), BI(1, 9), BI(5, 5)] and abs(float(below[1][0][2]) - 0.8 * 0.4) < 2e-4
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. seeded random heads
@pytest.mark.parametrize("size,ncls,mode,seed", SC.RANDOM_CASES)
def test_random_heads(size, ncls, mode, seed):
    heads, _, _ = SC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    got, ref = _check(eng, heads, mode, what=f"{size} {ncls} {mode} {seed}")
    assert (ref[6] > 0).sum() >= 5 and got[3][0] >= 10
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. sizes
@functools.lru_cache(maxsize=None)
def _len_engine():
    return DC._engine(SC.SIZE_LEN, SC.NCLS_LEN, 1)[1]


@pytest.mark.parametrize("L", SC.LENGTHS)
def test_list_lengths(L):
    heads, _, _ = SC.length_case(L)
    eng = _len_engine()
    try:
        for mode in SC.LENGTH_MODES:
            got, ref = _check(eng, heads, mode, what=f"L {L} {mode}")
            assert min(L, 100) - 2 <= got[3][0] <= min(L, 100)
        if L <= SC.TOP_K_MAX:                                   # 'hard' is the kernel that ships
            eng.set_nms_soft(None)
            off = _run(eng, heads)
            _set(eng, HARD)
            _same_bits(_run(eng, heads), off, f"hard against off, L {L}")
    finally:
        eng.set_nms_soft(None)


@pytest.mark.parametrize("L", SC.EDGE_LENGTHS)
def test_exactly_top_k_participants(L):
    heads, _, _, loner = SC.edge_case(L)
    eng = _len_engine()
    try:
        got, ref = _check(eng, heads, ("hard", "iou", 1.0, True), what=f"edge {L}")
        if L <= SC.TOP_K_MAX:
            assert got[3][0] == 2 and got[4][0][1] == loner
        else:
            assert got[3][0] == 1 and got[4][0][0] != loner
    finally:
        eng.set_nms_soft(None)
        eng.set_nms_rule("iou")


def test_top_k_64_leaves_the_65th_key_out():
    heads, _, _, loner = SC.topk_case()
    _, eng = DC._engine(SC.SIZE_LEN, 3, 1)
    got, ref = _check(eng, heads, "gauss_iou", what="top_k 64", top_k=SC.TOPK_SMALL)
    v = int(got[3][0])
    assert loner not in got[4][0][:v] and got[1][0][:v].min() < 0.5
    _set(eng, "gauss_iou")                                     # every key takes part: the loner, alone in its class, is kept with its score
    full = _run(eng, heads)
    at = full[4][0].tolist().index(loner)
    assert full[2][0][at] == 1 and abs(float(full[1][0][at]) - 0.55) < 2e-4
    eng.close()


def test_more_classes_than_the_parallel_pass_has_words_for():
    size, ncls, heads, _, _, pairs = RC.witness_case("wave0_first")
    assert ncls > DC.PAR_MAX_C
    _, eng = DC._engine(size, ncls, 1)
    got, ref = _check(eng, heads, "gauss_iou", what="C 1025")
    a, b = pairs[0]
    assert got[3][0] == 2 and got[4][0][:2].tolist() == [a, b] and got[1][0][1] < 0.95 * ref[1][0][0]
    eng.set_nms_soft(None)
    off = _run(eng, heads)
    _set(eng, HARD)
    _same_bits(_run(eng, heads), off, "hard against off, C 1025")
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. 'hard' is the kernel that ships
def _hard_equals_off(eng, heads, rule=("iou", 1.0, False), what="", **kw):
    eng.set_nms_rule(*rule)
    eng.set_nms_soft(None)
    off = _run(eng, heads, **kw)
    eng.set_nms_soft("hard")
    hard = _run(eng, heads, **kw)
    eng.set_nms_soft(None)
    _same_bits(hard, off, what)
    return off


def _rule_heads(ncls, seed):
    """Two images at 160^2: C = 3 the random heads of nms_rule_cases; C = 80 sparser ones (those have 11 k candidates per image) with
    some 2.5 k candidates per image -- more than the hard kernel's first chunk, fewer than top_k."""
    if ncls == 3:
        heads, _, s = RC.random_case(ncls, seed)
        return heads, s
    from yolo4hip.config import make_config
    heads = DC._random_heads(np.random.default_rng([seed, ncls]), RC.RANDOM_N, RC.RANDOM_SIZE, ncls, -1.0, -2.5)
    return heads, DC.boxes_and_scores(heads, ncls, make_config(RC.RANDOM_SIZE), RC.RANDOM_SIZE)[1]


@pytest.mark.parametrize("ncls,seed", [(3, 3), (3, 6), (80, 3), (80, 4)])
def test_hard_equals_off_on_random_heads_under_every_rule(ncls, seed):
    import torch
    heads, s = _rule_heads(ncls, seed)
    counts = (s > np.float32(RC.SCORE_THR)).sum(axis=(1, 2))
    assert counts.max() <= SC.TOP_K_MAX and (ncls == 3 or counts.min() > DC.NMS_THREADS)
    _, eng = DC._engine(RC.RANDOM_SIZE, ncls, RC.RANDOM_N)
    maps = torch.tensor([[1.25, -0.125, 1.0, 0.0], [1.0, 0.0, 1.6, -0.3]], dtype=torch.float32, device=eng.device)
    for rule in [("iou", 1.0, False)] + [RC.RULES[r] for r in sorted(RC.RULES)]:
        off = _hard_equals_off(eng, heads, rule, f"{rule}")
        assert off[3].sum() > 0
        _hard_equals_off(eng, heads, rule, f"{rule} mapped", box_map=maps)
    eng.close()


@pytest.mark.parametrize("name", ["s1300", "s2500"])
def test_hard_equals_off_on_the_later_chunk_stacks(name):
    heads, _, s = DC.chunk_case(name)
    assert DC.NMS_THREADS < (s > np.float32(SC.SCORE_THR)).sum() <= SC.TOP_K_MAX
    _, eng = DC._engine(DC.SIZE_CHUNK, 2, 1)
    for rule in (("iou", 1.0, False), ("diou", 0.6, False), ("iou", 1.0, True)):
        off = _hard_equals_off(eng, heads, rule, f"{name} {rule}")
        assert off[3][0] == 100
    eng.close()


@pytest.mark.parametrize("per_class,total,inp", [c for c in DC.CAP_CASES if c[2] != "dense6"])
def test_hard_equals_off_under_the_caps(per_class, total, inp):
    size, ncls, heads, _, s = DC.cap_input(inp)
    assert (s > np.float32(SC.SCORE_THR)).sum() <= SC.TOP_K_MAX
    _, eng = DC._engine(size, ncls, 1, max_per_class=per_class, max_total=total)
    _hard_equals_off(eng, heads, what=f"caps {per_class} {total} {inp}")
    _hard_equals_off(eng, heads, ("iou", 1.0, True), what=f"caps {per_class} {total} {inp} agnostic")
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. paths
def test_mapped_output_moves_only_the_boxes():
    import torch
    size, ncls, mode, seed = SC.RANDOM_CASES[0]
    heads, _, _ = SC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    plain, ref = _check(eng, heads, mode, what="plain")
    bm = np.array([[1.25, -0.125, 1.6, -0.3]], np.float32)
    mapped = _run(eng, heads, box_map=torch.from_numpy(bm).to(eng.device))
    _same_bits(mapped[1:], plain[1:], "mapped against plain")
    dev_b, _ = _device_tables(eng, heads)
    v = int(plain[3][0])
    want = MO.map_and_clip(dev_b[0, plain[4][0, :v]], bm[0])
    assert np.abs(mapped[0][0, :v] - want).max() < 1e-6 and not mapped[0][0, v:].any()
    assert (np.abs(mapped[0][0, :v] - plain[0][0, :v]) > 1e-3).any()
    eng.close()


NBOX96 = 3 * sum((TC.SIZE // s) ** 2 for s in (8, 16, 32))


def test_gathered_two_rows_that_see_the_same_box():
    """Row 0 carries the witness box of nms_rule_cases on cell (5, 7), row 1 the same box four cells to the left with a lower score
    and a map that shifts it by four cells and two pixels: IoU 0.82 in the photo.  Hard NMS keeps one; gaussian (sigma 2) keeps
    both, row 1's with its score times exp(-0.82^2 / 2).  Twice: the group's list order varies from run to run."""
    _, eng = DC._engine(TC.SIZE, 3, TC.CHUNK)
    heads = DC._heads_with(TC.SIZE, 3, 2, [(0, 0, 5, 7, 0, 1, 8.0, 2.0, RC.T_PAIR), (1, 0, 5, 3, 0, 1, 8.0, 1.0, RC.T_PAIR)])
    maps = np.array([IDENT, (1.0, (4 * 8 + 2) / TC.SIZE, 1.0, 0.0)], np.float32)
    rule = ("iou", 1.0, False)
    args = (eng, heads, [0, 0], [0, 1], maps, 1, 2, 64, rule, False)
    off, cnt, (tb, ts, _) = _gathered(*args)
    assert cnt.tolist() == [2] and off[3].tolist() == [1]
    eng.set_nms_soft("hard")
    _same_bits(_gathered(*args)[0], off, "gathered, hard against off")
    eng.set_nms_soft("gaussian", 2.0)
    got, cnt, _ = _gathered(*args)
    ref = _oracle(tb, ts, "gauss_iou", sigma=2.0)
    assert ref[5] >= SC.MARGIN_BAR and got[3].tolist() == [2]
    _assert_is_oracle(got, ref, "gathered")
    box_a, box_b = 3 * (5 * 12 + 7), NBOX96 + 3 * (5 * 12 + 3)
    assert got[4][0][:2].tolist() == [box_a, box_b] and abs(got[1][0][1] / ts[0, box_b, 1] - np.exp(-0.82 ** 2 / 2.0)) < 0.02
    _same_bits(_gathered(*args)[0], got, "gathered, repeated call")
    eng.close()


@pytest.mark.parametrize("ncls", [3, 80])
def test_gathered_photo_hard_equals_off_and_repeats_bit_for_bit(ncls):
    """The second photo of tiled_cases (three rows, one group): 'hard' through y4_nms_gathered equals soft-off, and a gaussian
    call repeated gives the same bits although the group's list is written in another order every time."""
    _, group, slot, maps, per_group = TC.geometry()
    sel = np.nonzero(group == 1)[0]
    heads = [h[sel] for h in TC.heads(ncls, 0)]
    _, eng = DC._engine(TC.SIZE, ncls, TC.CHUNK)
    for rule in (("iou", 1.0, False), ("diou", 0.6, False), ("iou", 1.0, True)):
        args = (eng, heads, [0] * len(sel), list(range(len(sel))), maps[sel], 1, len(sel), 1 << 15, rule, False)
        eng.set_nms_soft(None)
        off, cnt, _ = _gathered(*args)
        assert 100 < cnt[0] <= SC.TOP_K_MAX and off[3][0] > 10
        eng.set_nms_soft("hard")
        _same_bits(_gathered(*args)[0], off, f"gathered {rule}, hard against off")
        eng.set_nms_soft("gaussian")
        first = _gathered(*args)[0]
        assert not np.array_equal(first[1], off[1])
        for _ in range(2):
            _same_bits(_gathered(*args)[0], first, f"gathered {rule}, repeated call")
    eng.close()


def test_plain_path_repeats_bit_for_bit():
    size, ncls, mode, seed = SC.RANDOM_CASES[-1]
    heads, _, _ = SC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    _set(eng, mode)
    first = _run(eng, heads)
    for _ in range(3):
        _same_bits(_run(eng, heads), first, "repeated call")
    eng.close()


@pytest.mark.parametrize("mode", ["gauss_iou", "lin_diou_agn"])
def test_merged_forms_keep_the_soft_results_and_move_only_the_boxes(mode):
    """nms_merge with soft mode on: kept set, scores, classes and valid are the unmerged soft call's; the boxes are the merge
    oracle's for that kept set -- members decided on the original boxes, weighted with the original scores."""
    size, ncls, seed = 96, 3, SC.RANDOM_SEEDS[(96, 3, mode)]
    heads, _, _ = SC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    plain, ref = _check(eng, heads, mode, what="unmerged")
    dev_b, dev_s = _device_tables(eng, heads)
    eng.set_nms_merge(True)
    merged = _run(eng, heads)
    eng.set_nms_merge(False)
    _same_bits(merged[1:], plain[1:], "merged against unmerged")
    _, kind, beta, agn = _mode(mode)
    want, masks, margin = MO.merge_image(dev_b[0], dev_s[0], plain[4][0], plain[2][0], plain[3][0], SC.IOU_THR, SC.SCORE_THR, kind, beta,
                                         agn, None, 100)
    print(f"membership margin {margin:.3e}, boxes moved {int((want != plain[0][0]).any(axis=1).sum())}")
    assert margin >= 1e-5 and (want != plain[0][0]).any(axis=1).sum() >= 3
    assert np.array_equal(merged[0][0].view(np.int32), want.view(np.int32))
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. contract
def _get(eng):
    from yolo4hip import ext
    m, sg, ms, k = C.c_int(-9), C.c_float(-9.0), C.c_float(-9.0), C.c_int(-9)
    ext.check(eng.lib.y4_get_nms_soft(eng.handle, C.byref(m), C.byref(sg), C.byref(ms), C.byref(k)))
    return m.value, sg.value, ms.value, k.value


def test_contract_round_trip_refusals_and_siblings():
    from yolo4hip import ext
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    _, eng = DC._engine(96, 2, 1)
    assert _get(eng) == (0, 0.5, -1.0, 4096)
    assert (eng.nms_soft, eng.nms_sigma, eng.nms_soft_min_score, eng.nms_top_k) == (None, 0.5, None, 4096)
    ext.check(eng.lib.y4_set_nms_soft(eng.handle, 2, 0.25, 0.125, 77))
    assert _get(eng) == (2, 0.25, 0.125, 77)
    eng.set_nms_soft("gaussian", 0.75, 0.375, 512)
    assert _get(eng) == (1, 0.75, 0.375, 512)
    assert (eng.nms_soft, eng.nms_sigma, eng.nms_soft_min_score, eng.nms_top_k) == ("gaussian", 0.75, 0.375, 512)
    sib = eng.sibling()                                    # a sibling takes its parent's mode
    assert _get(sib) == (1, 0.75, 0.375, 512) and sib.nms_soft == "gaussian"
    sib.close()
    nan, inf = float("nan"), float("inf")
    for bad in ((4, 0.5, -1.0, 4096), (-1, 0.5, -1.0, 4096), (1, 0.0, -1.0, 4096), (1, -0.5, -1.0, 4096), (1, nan, -1.0, 4096),
                (1, inf, -1.0, 4096), (0, 0.0, -1.0, 4096), (3, nan, -1.0, 4096), (1, 0.5, nan, 4096), (1, 0.5, inf, 4096),
                (1, 0.5, -inf, 4096), (1, 0.5, 1.0, 4096), (1, 0.5, 1.5, 4096), (1, 0.5, -1.0, 0), (1, 0.5, -1.0, 4097),
                (1, 0.5, -1.0, -3)):
        assert eng.lib.y4_set_nms_soft(eng.handle, *bad) == -22, bad          # Y4_EINVAL
        assert _get(eng) == (1, 0.75, 0.375, 512)             # ... and nothing changed
    for null in range(4):
        args = [C.byref(C.c_int()), C.byref(C.c_float()), C.byref(C.c_float()), C.byref(C.c_int())]
        args[null] = None
        assert eng.lib.y4_get_nms_soft(eng.handle, *args) == -22
    assert eng.lib.y4_set_nms_rule(eng.handle, 2, 1.0, 0) == -22            # soft mode is no third kind
    for kw in ({"method": "exp"}, {"method": 1}, {"method": "gaussian", "sigma": 0.0}, {"method": None, "sigma": nan},
               {"method": "linear", "sigma": "x"}, {"method": "gaussian", "min_score": 1.0}, {"method": "gaussian", "min_score": -0.1},
               {"method": "gaussian", "min_score": nan}, {"method": "hard", "top_k": 0}, {"method": "hard", "top_k": 4097},
               {"method": "hard", "top_k": 64.0}, {"method": "hard", "top_k": True}):
        with pytest.raises(ValueError):
            eng.set_nms_soft(**kw)
        assert _get(eng) == (1, 0.75, 0.375, 512)
    eng.close()
    for kw in ({"nms_soft": "soft"}, {"nms_sigma": 0.0}, {"nms_soft": "gaussian", "nms_sigma": inf}, {"nms_soft_min_score": 1.0},
               {"nms_top_k": 5000}):
        with pytest.raises(ValueError):
            Engine(2, make_config(96), max_batch=1, dtype="bf16", **kw)
        with pytest.raises(ValueError):
            Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(96), max_batch=1, **kw)


def test_off_restores_the_bits_and_stream_siblings_follow():
    size, ncls, mode, seed = SC.RANDOM_CASES[0]
    heads, _, _ = SC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    first = _run(eng, heads)
    eng.set_nms_soft("gaussian")
    middle = _run(eng, heads)
    eng.set_nms_soft(None)
    assert _get(eng) == (0, 0.5, -1.0, 4096)
    _same_bits(_run(eng, heads), first, "off again")
    assert not np.array_equal(first[1], middle[1])
    eng._stream_siblings = [eng.sibling()]                 # what predict_stream keeps; set_nms_soft reaches them
    eng.set_nms_soft("linear", 0.5, 0.4, 100)
    assert _get(eng._stream_siblings[0]) == (2, 0.5, float(np.float32(0.4)), 100) and eng._stream_siblings[0].nms_soft == "linear"
    eng._stream_siblings[0].close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. facade
def test_facade_runs_soft_nms_on_every_path(tmp_path):
    """Yolov4(nms_soft='gaussian') on the tiny test set: predict, predict_tiled, predict_tta, evaluate_map and evaluate_coco run
    under it; evaluate_coco equals the oracle fed the same model's detections (the pattern of test_gpu_evaluate_coco.py); scores
    come out non-increasing; the keyword survives load_model."""
    import coco_oracle
    from test_gpu_evaluate_coco import PATHS, _assert_equals_oracle, _ground_truth_from, _images, _predict, _write_annotation
    from yolo4hip import prepost
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    imgdir = str(tmp_path / "img")
    os.makedirs(imgdir)
    names = [f"s{k}.jpeg" for k in range(3)]
    for name in names:
        shutil.copy(os.path.join(GOLDEN, "street.jpeg"), os.path.join(imgdir, name))
    cfg = make_config(160)
    cfg["batch_size"] = 2
    cls_path = os.path.join(CLASS_DIR, "bccd_classes.txt")
    m = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2, nms_soft="gaussian")
    d = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2)
    assert (m.nms_soft, m.nms_sigma, m.nms_soft_min_score, m.nms_top_k) == ("gaussian", 0.5, None, 4096)
    assert m.engine.nms_soft == "gaussian" and d.engine.nms_soft is None
    raws = [prepost.imread_rgb(os.path.join(imgdir, name)) for name in names]
    for path in PATHS:
        pred = _predict(m, path, raws)
        base = _predict(d, path, raws)
        for k in range(3):
            v = int(pred[3][k])
            assert v >= 3 and (np.diff(pred[1][k, :v]) <= 0).all()
        assert not np.array_equal(pred[1], base[1]), path          # the mode was in force
        gts = []
        for k, raw in enumerate(raws):
            nb = int(pred[3][k])
            px = coco_oracle.pixel_boxes(pred[0][k, :nb], (raw.shape[1], raw.shape[0]))
            gts.append(_ground_truth_from([tuple(px[j]) + (pred[2][k, j],) for j in range(nb)], k))
        ann = str(tmp_path / f"ann_{path}.txt")
        _write_annotation(ann, names, gts)
        res = m.evaluate_coco(ann, imgdir, bs=2, **PATHS[path])
        _assert_equals_oracle(res, _images(pred, raws, gts), path)
        if path == "plain":
            vm = m.evaluate_map(ann, imgdir, bs=2, iou_thresholds=(0.5,))
            assert sum(vm["n_det"].values()) == int(pred[3].sum()) and 0.0 < vm["per_threshold"][0.5]["mAP"] <= 1.0
            imgs = m.engine.preprocess_u8_batch(raws[:2])[0]
            before = m.inference_model.predict(imgs)
            ckpt = str(tmp_path / "tiny.ckpt")
            m.save_model(ckpt)
            m.load_model(ckpt)
            assert m.engine.nms_soft == "gaussian"
            for a, b in zip(m.inference_model.predict(imgs), before):
                assert np.array_equal(a.view(np.int32), b.view(np.int32))
    m.engine.close(), d.engine.close()
