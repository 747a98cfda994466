"""Matrix-NMS on the device (y4_set_nms_matrix; matrix_nms.hip) against tests/matrix_nms_oracle.py on the inputs of
tests/matrix_nms_cases.py (witnesses and margins asserted without a GPU in tests/test_matrix_nms_cpu.py).

The oracle runs on the candidate list and the box table the device's own decode stage produced (read back from the scratch of a
gathered decode, as tests/test_gpu_soft_nms.py does), so every difference is the NMS kernel's.  Bars: kept ids, classes, valid and
order ==; boxes bit-equal to the decoded boxes clipped; scores: linear under 'iou' and under 'diou' at beta = 1 the bits of the
float32 face (every operation is correctly rounded on both sides), otherwise within the per-score bound the float64 face derives (0
for a score that was not decayed: bit-equal).  The largest measured distance goes to profiles/matrix_nms/parity_measured.json."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import decode_nms_cases as DC
import matrix_nms_cases as MC
import matrix_nms_oracle as MX
import merge_oracle as MO
import nms_rule_cases as RC
import soft_nms_cases as SC
import tiled_cases as TC
from helpers import CLASS_DIR, GOLDEN
from test_gpu_nms_merge import IDENT, _device_tables, _gathered, _same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(name, err, bound):
    """Keep the largest (relative score error, its bound) seen under `name` in profiles/matrix_nms/parity_measured.json."""
    path = os.path.join(ROOT, "profiles", "matrix_nms", "parity_measured.json")
    try:
        with open(path) as f:
            data = json.load(f)
    except (OSError, ValueError):
        data = {}
    if name not in data or err >= data[name]["largest_relative_score_error"]:
        data[name] = {"largest_relative_score_error": err, "largest_bound": bound}
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:
        pass                                                   # (a read-only checkout: the assertion does not depend on the file)


def _mode(mode):
    return MC.MODES[mode] if isinstance(mode, str) else mode


def _set(eng, mode, sigma=SC.SIGMA, min_score=None, top_k=SC.TOP_K_MAX):
    method, kind, beta, agn = _mode(mode)
    eng.set_nms_rule(kind, beta, agn)
    eng.set_nms_matrix(method, sigma, min_score, top_k)


def _run(eng, heads, **kw):
    n = eng.set_heads(heads)
    return [o.cpu().numpy() for o in eng.decode_nms_device(n, None, **kw)]


def _oracle(dev_b, dev_s, mode, caps=None, sigma=SC.SIGMA, min_score=None, top_k=SC.TOP_K_MAX, face="f64"):
    caps = caps or {}
    method, kind, beta, agn = _mode(mode)
    return MX.matrix_nms(dev_b, dev_s, caps.get("max_per_class", 100), caps.get("max_total", 100), SC.SCORE_THR, kind, beta, agn, method,
                         sigma, min_score, top_k, face)


def _exact(mode):
    """Is every operation of the mode correctly rounded on both sides?  (no expf, no powf)"""
    method, kind, beta, _ = _mode(mode)
    return method == "linear" and (kind == "iou" or float(beta) == 1.0)


def _assert_is_oracle(got, ref, what="", ref32=None):
    """Decisions ==, boxes bit-equal, scores within the derived per-score bound (relative) of the float64 face -- and the bits of
    the float32 face `ref32` where one is given."""
    for k in (3, 4, 2):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, "output", k, got[k], ref[k])
    assert np.array_equal(got[0].view(np.int32), ref[0].view(np.int32)), (what, "boxes")
    err = np.abs(got[1].astype(np.float64) - ref[1])
    tol = ref[6] * ref[1]
    rel = float((err / np.maximum(ref[1], 1e-30)).max())
    print(f"{what}: valid {ref[3].tolist()}, margin {ref[5]:.3e}, decayed results {int((ref[6] > 0).sum())}, "
          f"largest score error {rel:.3e} (largest bound {float(ref[6].max()):.3e})")
    _record(what.split(":")[0], rel, float(ref[6].max()))
    assert (err <= tol).all(), (what, "scores", float((err - tol).max()))
    if ref32 is not None:
        assert np.array_equal(got[1].view(np.int32), ref32[1].view(np.int32)), (what, "scores against the float32 face")
    for i in range(len(got[3])):                               # non-increasing, zero / -1 padded
        v = int(got[3][i])
        assert (np.diff(got[1][i, :v]) <= 0).all() and not got[1][i, v:].any() and (got[4][i, v:] == -1).all()


def _check(eng, heads, mode, caps=None, what="", **kw):
    """`heads` under `mode` on the device against the oracle on the device's decode tables -> (device outputs, oracle result)."""
    _set(eng, mode, **kw)
    dev_b, dev_s = _device_tables(eng, heads)
    got = _run(eng, heads)
    ref = _oracle(dev_b, dev_s, mode, caps, **kw)
    assert ref[5] >= MC.MARGIN_BAR, (what, ref[5])
    _assert_is_oracle(got, ref, what, _oracle(dev_b, dev_s, mode, caps, face="f32", **kw) if _exact(mode) else None)
    return got, ref


def _witness(name, mode="gauss_iou", **over):
    size, ncls, heads, b, s, caps, kw = MC.witness(name)
    _, eng = DC._engine(size, ncls, 1, **caps)
    try:
        got, ref = _check(eng, heads, mode, caps, f"witness: {name} {mode}", **dict(kw, **over))
    finally:
        eng.close()
    v = int(got[3][0])
    return [int(x) for x in got[4][0][:v]], [int(x) for x in got[2][0][:v]], got[1][0][:v], got


BI = lambda gy, gx: SC.box_index(SC.SIZE, gy, gx)      # noqa: E731


# ------------------------------------------------------------------------------------------------ 1. witnesses
def test_witness_decay_is_the_minimum_not_the_product():
    ids, _, sc, _ = _witness("two_factors")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)] and np.allclose(sc, [0.9, 0.82927, 0.48480], atol=2e-4)
    ids, _, sc, _ = _witness("two_factors", "lin_iou")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)] and np.allclose(sc, [0.9, 0.75556, 0.4], atol=2e-4)


def test_witness_chain_is_compensated():
    ids, _, sc, got = _witness("chain")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)] and got[3][0] == 3 and np.allclose(sc, [0.9, 0.66595, 0.38940], atol=2e-4)
    ids, _, sc, _ = _witness("chain", "lin_iou")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)]


def test_witness_classes_and_agnostic():
    ids, cls, sc, _ = _witness("classes")
    assert ids == [BI(5, 4), BI(5, 5), BI(1, 9)] and cls == [1, 2, 1] and abs(float(sc[1]) - 0.8) < 2e-4
    ids, cls, sc, _ = _witness("classes", "gauss_iou_agn")
    assert ids == [BI(5, 4), BI(1, 9), BI(5, 5)] and cls == [1, 1, 2] and abs(float(sc[2]) - 0.38940) < 2e-4


def test_witness_floor_is_strict():
    ids, _, _, got = _witness("floor")
    assert ids == [BI(5, 4), BI(1, 9)] and got[3][0] == 2
    size, ncls, heads, _, _, _, _ = MC.witness("order")
    _, eng = DC._engine(size, ncls, 1)
    _set(eng, "gauss_iou")
    bp = _run(eng, heads)[1][0][2]                              # B' on the device
    _set(eng, "gauss_iou", min_score=float(bp))
    assert _run(eng, heads)[3][0] == 2
    _set(eng, "gauss_iou", min_score=float(np.nextafter(bp, np.float32(0))))
    at = _run(eng, heads)
    assert at[3][0] == 3 and at[1][0][2] == bp
    eng.close()


def test_witness_a_skipped_candidate_still_decays():
    ids, cls, sc, _ = _witness("skipped_still_decays", "gauss_iou_agn")
    assert ids == [BI(1, 1), BI(8, 5)] and cls == [0, 1] and abs(float(sc[1]) - 0.7 * np.exp(-0.72)) < 2e-4
    ids, cls, sc, _ = _witness("skipped_still_decays", "lin_iou_agn")
    assert ids == [BI(1, 1), BI(8, 5)] and abs(float(sc[1]) - 0.28) < 2e-4


def test_witness_max_total_ties_and_empty():
    ids, _, _, got = _witness("max_total")
    assert ids == [BI(1, 1), BI(5, 5)] and got[3][0] == 2 and got[4].shape == (1, 2)
    for mode in ("gauss_iou", "lin_iou"):
        ids, cls, sc, _ = _witness("ties", mode)
        boxes = sorted(BI(gy, gx) for gy, gx in ((7, 2), (1, 9), (4, 4), (1, 3)))
        assert ids == [b for b in boxes for _ in (0, 1)] and cls == [0, 2] * 4 and len(set(sc.tolist())) == 1
    ids, _, _, got = _witness("empty")
    assert ids == [] and got[3][0] == 0 and not got[0].any() and not got[1].any() and not got[2].any() and (got[4] == -1).all()


def test_witness_identical_boxes_under_linear():
    ids, cls, _, got = _witness("identical", "lin_iou_agn")
    assert ids == [BI(5, 5)] and cls == [0] and np.isfinite(got[1]).all()
    ids, _, sc, _ = _witness("identical", "gauss_iou_agn")
    assert len(ids) == 3 and sc[2] < sc[1] < 0.2
    assert len(_witness("identical", "lin_iou")[0]) == 3


def test_witness_order_and_pairs_are_soft_nms_bit_for_bit():
    """c = 0 for both candidates of a class: gaussian Matrix-NMS is gaussian Soft-NMS, all five outputs."""
    size, ncls, heads, _, _, _, _ = MC.witness("order")
    for sz, nc, hd in ((size, ncls, heads), (SC.SIZE_LEN, SC.NCLS_LEN, MC.pairs_case()[0])):
        _, eng = DC._engine(sz, nc, 1)
        got, ref = _check(eng, hd, "gauss_iou", what=f"pairs: {sz}")
        eng.set_nms_matrix(None)
        eng.set_nms_soft("gaussian")
        _same_bits(got, _run(eng, hd), f"matrix against soft, {sz}")
        assert (ref[6] > 0).sum() >= 1
        eng.close()


def test_disjoint_lists_are_the_hard_kernel_bit_for_bit():
    heads, _, _ = MC.disjoint_case()
    _, eng = DC._engine(SC.SIZE_LEN, SC.NCLS_LEN, 1)
    off = _run(eng, heads)
    assert off[3][0] == 100
    for mode in ("gauss_iou", "lin_iou", "gauss_diou", "lin_diou"):
        got, ref = _check(eng, heads, mode, what=f"disjoint: {mode}")
        _same_bits(got, off, f"disjoint {mode} against off")
        eng.set_nms_matrix(None)
    for name in ("max_total", "ties"):                          # (and two witnesses: a cap, exact ties)
        size, ncls, hd, _, _, caps, _ = MC.witness(name)
        _, e2 = DC._engine(size, ncls, 1, **caps)
        off = _run(e2, hd)
        _set(e2, "gauss_iou")
        _same_bits(_run(e2, hd), off, f"{name} against off")
        e2.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. seeded random heads
@pytest.mark.parametrize("size,ncls,mode,seed", MC.RANDOM_CASES)
def test_random_heads(size, ncls, mode, seed):
    heads, _, _ = MC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    got, ref = _check(eng, heads, mode, what=f"random: {size} {ncls} {mode} {seed}")
    assert (ref[6] > 0).sum() >= 5 and got[3][0] >= 10
    eng.close()


def test_diou_at_beta_1_linear_is_the_float32_face():
    size, ncls, seed = 96, 3, MC.RANDOM_SEEDS[(96, 3, "lin_diou")]
    heads, _, _ = MC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    mode = ("linear", "diou", 1.0, False)
    _set(eng, mode)
    dev_b, dev_s = _device_tables(eng, heads)
    got = _run(eng, heads)
    f32 = _oracle(dev_b, dev_s, mode, face="f32")
    _same_bits(got, f32[:5], "linear diou beta 1")
    assert (got[1][0] != np.sort(dev_s[dev_s > np.float32(SC.SCORE_THR)])[::-1][:100]).sum() >= 5
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. sizes
@functools.lru_cache(maxsize=None)
def _len_engine():
    return DC._engine(SC.SIZE_LEN, SC.NCLS_LEN, 1)[1]


@pytest.mark.parametrize("L", SC.LENGTHS)
def test_list_lengths(L):
    heads, _, _ = SC.length_case(L, MC.LENGTH_SEEDS[L])
    eng = _len_engine()
    try:
        for mode in MC.LENGTH_MODES:
            got, ref = _check(eng, heads, mode, what=f"lengths: L {L} {mode}")
            assert got[3][0] == min(L, 100)
    finally:
        eng.set_nms_matrix(None)


@pytest.mark.parametrize("L", SC.EDGE_LENGTHS)
def test_exactly_top_k_participants(L):
    """4095 keys of one agnostic segment, every pair interacting, and the loner: kept iff it is one of the top_k."""
    heads, _, _, loner = SC.edge_case(L)
    eng = _len_engine()
    try:
        for mode in ("gauss_iou_agn", "lin_iou_agn"):
            got, ref = _check(eng, heads, mode, what=f"edge: {L} {mode}")
            if L <= SC.TOP_K_MAX:
                assert got[3][0] == 2 and got[4][0][1] == loner
            else:
                assert got[3][0] == 1 and got[4][0][0] != loner
    finally:
        eng.set_nms_matrix(None)
        eng.set_nms_rule("iou")


def test_top_k_64_leaves_the_65th_key_out():
    heads, _, _, loner = SC.topk_case()
    _, eng = DC._engine(SC.SIZE_LEN, 3, 1)
    got, ref = _check(eng, heads, "gauss_iou", what="top_k: 64", top_k=SC.TOPK_SMALL)
    v = int(got[3][0])
    assert loner not in got[4][0][:v] and got[1][0][:v].min() < 0.5
    got, ref = _check(eng, heads, "gauss_iou", what="top_k: all")       # every key takes part: the loner, alone in its class, keeps its score
    at = got[4][0].tolist().index(loner)
    assert got[2][0][at] == 1 and abs(float(got[1][0][at]) - 0.55) < 2e-4
    eng.close()


def test_more_classes_than_the_parallel_pass_has_words_for():
    size, ncls, heads, _, _, pairs = RC.witness_case("wave0_first")
    assert ncls > DC.PAR_MAX_C
    _, eng = DC._engine(size, ncls, 1)
    got, ref = _check(eng, heads, "gauss_iou", what="classes: 1025")
    a, b = pairs[0]
    assert got[3][0] == 2 and got[4][0][:2].tolist() == [a, b] and got[1][0][1] < 0.95 * ref[1][0][0]
    eng.close()


@pytest.mark.parametrize("per_class,total,mode,seed", MC.CAP_RANDOM)
def test_caps_on_random_heads(per_class, total, mode, seed):
    """max_per_class below max_total takes the cap pass: class-aware (the class's segment) and agnostic (the whole list)."""
    heads, _, _ = MC.random_case(96, 3, seed)
    caps = {"max_per_class": per_class, "max_total": total}
    _, eng = DC._engine(96, 3, 1, **caps)
    got, ref = _check(eng, heads, mode, caps, f"caps: {per_class} {total} {mode} {seed}")
    v = int(got[3][0])
    assert np.bincount(got[2][0][:v].astype(np.int64)).max() == min(per_class, v)
    eng.close()


@pytest.mark.parametrize("per_class,total,inp", [c for c in DC.CAP_CASES if c[2] in MC.CAP_INPUTS])
def test_caps_on_the_later_chunk_stack_and_the_grid(per_class, total, inp):
    """2660 and 2704 candidates in two classes: segments longer than a thread's first register, max_total up to 1024."""
    size, ncls, heads, _, s = DC.cap_input(inp)
    assert DC.NMS_THREADS < (s > np.float32(SC.SCORE_THR)).sum() <= SC.TOP_K_MAX
    caps = {"max_per_class": per_class, "max_total": total}
    _, eng = DC._engine(size, ncls, 1, **caps)
    for mode in MC.CAP_MODES:
        _check(eng, heads, mode, caps, f"caps: {per_class} {total} {inp} {mode}")
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. paths
def test_mapped_output_moves_only_the_boxes():
    import torch
    size, ncls, mode, seed = MC.RANDOM_CASES[0]
    heads, _, _ = MC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    plain, ref = _check(eng, heads, mode, what="mapped: plain")
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
    args = (eng, heads, [0, 0], [0, 1], maps, 1, 2, 64, ("iou", 1.0, False), False)
    off, cnt, (tb, ts, _) = _gathered(*args)
    assert cnt.tolist() == [2] and off[3].tolist() == [1]
    eng.set_nms_matrix("gaussian", 2.0)
    got, cnt, _ = _gathered(*args)
    ref = _oracle(tb, ts, "gauss_iou", sigma=2.0)
    assert ref[5] >= MC.MARGIN_BAR and got[3].tolist() == [2]
    _assert_is_oracle(got, ref, "gathered: two rows")
    box_a, box_b = 3 * (5 * 12 + 7), NBOX96 + 3 * (5 * 12 + 3)
    assert got[4][0][:2].tolist() == [box_a, box_b] and abs(got[1][0][1] / ts[0, box_b, 1] - np.exp(-0.82 ** 2 / 2.0)) < 0.02
    _same_bits(_gathered(*args)[0], got, "gathered, repeated call")
    eng.close()


@pytest.mark.parametrize("ncls", [3, 80])
def test_gathered_photo_repeats_bit_for_bit(ncls):
    """The second photo of tiled_cases (three rows, one group) through y4_nms_gathered: a call repeated gives the same bits although
    the group's list is written in another order every time."""
    _, group, slot, maps, per_group = TC.geometry()
    sel = np.nonzero(group == 1)[0]
    heads = [h[sel] for h in TC.heads(ncls, 0)]
    _, eng = DC._engine(TC.SIZE, ncls, TC.CHUNK)
    for rule, method in ((("iou", 1.0, False), "gaussian"), (("diou", 0.6, False), "linear"), (("iou", 1.0, True), "gaussian")):
        args = (eng, heads, [0] * len(sel), list(range(len(sel))), maps[sel], 1, len(sel), 1 << 15, rule, False)
        eng.set_nms_matrix(None)
        off, cnt, _ = _gathered(*args)
        assert 100 < cnt[0] <= SC.TOP_K_MAX and off[3][0] > 10
        eng.set_nms_matrix(method)
        first = _gathered(*args)[0]
        assert not np.array_equal(first[1], off[1])
        for _ in range(2):
            _same_bits(_gathered(*args)[0], first, f"gathered {rule} {method}, repeated call")
    eng.close()


def test_plain_path_repeats_bit_for_bit():
    size, ncls, mode, seed = MC.RANDOM_CASES[-1]
    heads, _, _ = MC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    _set(eng, mode)
    first = _run(eng, heads)
    for _ in range(3):
        _same_bits(_run(eng, heads), first, "repeated call")
    eng.close()


@pytest.mark.parametrize("mode", ["gauss_iou", "lin_diou_agn"])
def test_merged_forms_keep_the_matrix_results_and_move_only_the_boxes(mode):
    """nms_merge with the matrix mode on: kept set, scores, classes and valid are the unmerged matrix call's; the boxes are the merge
    oracle's for that kept set -- members decided on the original boxes with iou_threshold, weighted with the original scores."""
    size, ncls, seed = 96, 3, MC.RANDOM_SEEDS[(96, 3, mode)]
    heads, _, _ = MC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    plain, ref = _check(eng, heads, mode, what=f"merged: unmerged {mode}")
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


# ------------------------------------------------------------------------------------------------ 5. contract
def _get(eng, which="matrix"):
    from yolo4hip import ext
    m, sg, ms, k = C.c_int(-9), C.c_float(-9.0), C.c_float(-9.0), C.c_int(-9)
    ext.check(getattr(eng.lib, f"y4_get_nms_{which}")(eng.handle, C.byref(m), C.byref(sg), C.byref(ms), C.byref(k)))
    return m.value, sg.value, ms.value, k.value


def test_contract_round_trip_refusals_and_siblings():
    from yolo4hip import ext
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    _, eng = DC._engine(96, 2, 1)
    assert _get(eng) == (0, 0.5, -1.0, 4096)
    assert (eng.nms_matrix, eng.nms_matrix_sigma, eng.nms_matrix_min_score, eng.nms_matrix_top_k) == (None, 0.5, None, 4096)
    ext.check(eng.lib.y4_set_nms_matrix(eng.handle, 2, 0.25, 0.125, 77))
    assert _get(eng) == (2, 0.25, 0.125, 77)
    eng.set_nms_matrix("gaussian", 0.75, 0.375, 512)
    assert _get(eng) == (1, 0.75, 0.375, 512)
    assert (eng.nms_matrix, eng.nms_matrix_sigma, eng.nms_matrix_min_score, eng.nms_matrix_top_k) == ("gaussian", 0.75, 0.375, 512)
    sib = eng.sibling()                                    # a sibling takes its parent's mode
    assert _get(sib) == (1, 0.75, 0.375, 512) and sib.nms_matrix == "gaussian" and sib.nms_soft is None
    sib.close()
    nan, inf = float("nan"), float("inf")
    for bad in ((3, 0.5, -1.0, 4096), (-1, 0.5, -1.0, 4096), (1, 0.0, -1.0, 4096), (1, -0.5, -1.0, 4096), (1, nan, -1.0, 4096),
                (1, inf, -1.0, 4096), (0, 0.0, -1.0, 4096), (2, nan, -1.0, 4096), (1, 0.5, nan, 4096), (1, 0.5, inf, 4096),
                (1, 0.5, -inf, 4096), (1, 0.5, 1.0, 4096), (1, 0.5, 1.5, 4096), (1, 0.5, -1.0, 0), (1, 0.5, -1.0, 4097),
                (1, 0.5, -1.0, -3)):
        assert eng.lib.y4_set_nms_matrix(eng.handle, *bad) == -22, bad        # Y4_EINVAL
        assert _get(eng) == (1, 0.75, 0.375, 512)             # ... and nothing changed
    for null in range(4):
        args = [C.byref(C.c_int()), C.byref(C.c_float()), C.byref(C.c_float()), C.byref(C.c_int())]
        args[null] = None
        assert eng.lib.y4_get_nms_matrix(eng.handle, *args) == -22
    # the two decay modes exclude each other, in both directions, with both states unchanged
    for m in (1, 2, 3):
        assert eng.lib.y4_set_nms_soft(eng.handle, m, 0.5, -1.0, 4096) == -22
    assert _get(eng, "soft") == (0, 0.5, -1.0, 4096) and _get(eng) == (1, 0.75, 0.375, 512)
    ext.check(eng.lib.y4_set_nms_soft(eng.handle, 0, 0.25, -1.0, 100))          # (off is no conflict)
    with pytest.raises(ValueError):
        eng.set_nms_soft("gaussian")
    assert eng.nms_soft is None and _get(eng, "soft") == (0, 0.25, -1.0, 100)
    eng.set_nms_matrix(None)
    assert _get(eng) == (0, 0.5, -1.0, 4096)
    assert eng.lib.y4_set_nms_soft(eng.handle, 4, 0.5, -1.0, 4096) == -22       # as before: no method 4
    eng.set_nms_soft("linear", 0.5, 0.4, 100)
    for m in (1, 2):
        assert eng.lib.y4_set_nms_matrix(eng.handle, m, 0.5, -1.0, 4096) == -22
    with pytest.raises(ValueError):
        eng.set_nms_matrix("gaussian")
    assert _get(eng) == (0, 0.5, -1.0, 4096) and eng.nms_matrix is None and _get(eng, "soft") == (2, 0.5, float(np.float32(0.4)), 100)
    ext.check(eng.lib.y4_set_nms_matrix(eng.handle, 0, 0.5, -1.0, 4096))        # (off is no conflict)
    eng.set_nms_soft(None)
    eng.set_nms_matrix("linear", 0.75, 0.375, 512)
    for kw in ({"method": "exp"}, {"method": "hard"}, {"method": 1}, {"method": "gaussian", "sigma": 0.0}, {"method": None, "sigma": nan},
               {"method": "linear", "sigma": "x"}, {"method": "gaussian", "min_score": 1.0}, {"method": "gaussian", "min_score": -0.1},
               {"method": "gaussian", "min_score": nan}, {"method": "linear", "top_k": 0}, {"method": "linear", "top_k": 4097},
               {"method": "linear", "top_k": 64.0}, {"method": "linear", "top_k": True}):
        with pytest.raises(ValueError):
            eng.set_nms_matrix(**kw)
        assert _get(eng) == (2, 0.75, 0.375, 512)
    eng.close()
    for kw in ({"nms_matrix": "hard"}, {"nms_matrix": "gaussian", "nms_soft": "gaussian"}, {"nms_matrix": "linear", "nms_soft": "hard"},
               {"nms_matrix": "gaussian", "nms_sigma": inf}, {"nms_matrix": "gaussian", "nms_soft_min_score": 1.0},
               {"nms_matrix": "linear", "nms_top_k": 5000}, {"nms_matrix": 1}):
        with pytest.raises(ValueError):
            Engine(2, make_config(96), max_batch=1, dtype="bf16", **kw)
        with pytest.raises(ValueError):
            Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(96), max_batch=1, **kw)
    e = Engine(2, make_config(96), max_batch=1, dtype="bf16", nms_matrix="linear", nms_sigma=0.25, nms_soft_min_score=0.125, nms_top_k=300)
    assert _get(e) == (2, 0.25, 0.125, 300) and _get(e, "soft")[0] == 0 and e.nms_matrix == "linear" and e.nms_soft is None
    e.close()


def test_sibling_takes_both_decay_modes_also_one_that_is_off_with_parameters():
    from yolo4hip import ext
    _, eng = DC._engine(96, 2, 1)
    ext.check(eng.lib.y4_set_nms_matrix(eng.handle, 0, 0.25, 0.125, 77))
    eng.set_nms_matrix(None, 0.25, 0.125, 77)
    eng.set_nms_soft("linear", 0.75, 0.375, 512)
    sib = eng.sibling()
    assert _get(sib, "soft") == (2, 0.75, 0.375, 512) and _get(sib) == (0, 0.25, 0.125, 77)
    for name, value in (("nms_soft", "linear"), ("nms_sigma", 0.75), ("nms_soft_min_score", 0.375), ("nms_top_k", 512), ("nms_matrix", None),
                        ("nms_matrix_sigma", 0.25), ("nms_matrix_min_score", 0.125), ("nms_matrix_top_k", 77)):
        assert getattr(eng, name) == value and getattr(sib, name) == value, name
    sib.close()
    eng.close()


def test_off_restores_the_bits_and_stream_siblings_follow():
    size, ncls, mode, seed = MC.RANDOM_CASES[0]
    heads, _, _ = MC.random_case(size, ncls, seed)
    _, eng = DC._engine(size, ncls, 1)
    first = _run(eng, heads)
    eng.set_nms_matrix("gaussian")
    middle = _run(eng, heads)
    eng.set_nms_matrix(None)
    assert _get(eng) == (0, 0.5, -1.0, 4096)
    _same_bits(_run(eng, heads), first, "off again")
    assert not np.array_equal(first[1], middle[1])
    eng._stream_siblings = [eng.sibling()]                 # what predict_stream keeps; set_nms_matrix reaches them
    eng.set_nms_matrix("linear", 0.5, 0.4, 100)
    assert _get(eng._stream_siblings[0]) == (2, 0.5, float(np.float32(0.4)), 100) and eng._stream_siblings[0].nms_matrix == "linear"
    eng._stream_siblings[0].close()
    eng.close()


# ------------------------------------------------------------------------------------------------ 6. facade
def test_facade_runs_matrix_nms_on_predict_tiled_and_tta():
    """Yolov4(nms_matrix='gaussian') on three copies of the street photo: predict, predict_tiled and predict_tta run under it --
    scores differ from the default model's, come out non-increasing, and the engine carries the mode."""
    from test_gpu_evaluate_coco import _predict
    from yolo4hip import prepost
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg = make_config(160)
    cfg["batch_size"] = 2
    cls_path = os.path.join(CLASS_DIR, "bccd_classes.txt")
    m = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2, nms_matrix="gaussian")
    d = Yolov4(None, cls_path, cfg, dtype="f32", max_batch=2)
    assert m.nms_matrix == "gaussian" and m.nms_soft is None and m.engine.nms_matrix == "gaussian" and d.engine.nms_matrix is None
    raws = [prepost.imread_rgb(os.path.join(GOLDEN, "street.jpeg"))] * 3
    for path in ("plain", "tiled", "views"):
        pred = _predict(m, path, raws)
        base = _predict(d, path, raws)
        for k in range(3):
            v = int(pred[3][k])
            assert v >= 3 and (np.diff(pred[1][k, :v]) <= 0).all()
        assert not np.array_equal(pred[1], base[1]), path          # the mode was in force
    m.engine.close(), d.engine.close()
