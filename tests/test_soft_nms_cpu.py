"""The Soft-NMS oracle (tests/soft_nms_oracle.py) and the inputs of tests/soft_nms_cases.py, without a GPU: the oracle on
hand-computed witnesses, its 'hard' method against oracle/decode_nms.py, and the margin of every seeded case.

The margin bar.  The device works in float32, the float64 face of the oracle behind the (float32) measure in float64.  A working
score is decayed at most once per kept box, max_total times, and one float32 decay adds at most soft_nms_oracle.decay_ulps(...)
units of 2^-24 of relative error (derived there): 2 u + 2 * EXPF_ULPS + 1 for the gaussian factor exp(-u), u = m^2 / sigma <= 2 at
sigma = 0.5 -- 7 units at the very most, 3 to 4 for the overlaps that occur (u <= 1/2) -- and 2 for the linear one.  At
max_total = 100 that is 100 * 7 * 2^-24 = 4.2e-5 in the worst case and about 2e-5 typically: a decision whose two sides are at least
1e-4 apart (relative) in the float64 face is the same decision in float32.  Every seeded case must show that margin; a seed that
does not is replaced in soft_nms_cases.py."""
import numpy as np
import pytest

import decode_nms_cases as DC
import nms_rule_cases as RC
import soft_nms_cases as SC
import soft_nms_oracle as SO


def _oracle(b, s, caps=None, soft=None, mode="gauss_iou", face="f32", iou_thr=SC.IOU_THR, top_k=SC.TOP_K_MAX):
    caps, soft = caps or {}, soft or {}
    method, kind, beta, agn = SC.MODES[mode] if isinstance(mode, str) else mode
    return SO.soft_nms(b, s, caps.get("max_per_class", 100), caps.get("max_total", 100), iou_thr, SC.SCORE_THR, kind, beta, agn,
                       method, SC.SIGMA, soft.get("min_score"), top_k, face)


def _wit(name, mode="gauss_iou", face="f64", **kw):
    size, ncls, heads, b, s, caps, soft = SC.witness(name)
    r = _oracle(b, s, caps, soft, mode, face, **kw)
    v = int(r[3][0])
    return [int(x) for x in r[4][0][:v]], [int(x) for x in r[2][0][:v]], r[1][0][:v].astype(np.float64), r


def _gauss(m):
    return float(np.exp(-m * m / SC.SIGMA))


BI = lambda gy, gx: SC.box_index(SC.SIZE, gy, gx)      # noqa: E731


# ------------------------------------------------------------------------------------------------ 1. witnesses, by hand
def test_the_bound_stays_under_the_margin_bar():
    assert SO.global_bound(100, SC.SIGMA, "gaussian") < 0.5 * SC.MARGIN_BAR
    assert SO.global_bound(100, SC.SIGMA, "linear") < 0.5 * SC.MARGIN_BAR
    assert abs(SO.global_bound(100, SC.SIGMA, "gaussian") - 100 * 7 * 2.0 ** -24) < 1e-12


def test_witness_order_is_by_current_score():
    ids, cls, sc, _ = _wit("order")
    assert ids == [BI(5, 4), BI(1, 9), BI(5, 5)]                     # A, C, B'
    assert np.allclose(sc, [0.9, 0.5, 0.8 * _gauss(0.6)], atol=2e-4) and sc[2] < sc[1]
    # the hard kernel's walk (and 'hard' here) visits B before C
    assert _wit("order", ("hard", "iou", 1.0, False))[0] == [BI(5, 4), BI(1, 9)]
    assert _wit("order", ("hard", "iou", 1.0, False), iou_thr=0.7)[0] == [BI(5, 4), BI(5, 5), BI(1, 9)]


def test_witness_two_kept_boxes_decay_in_pick_order():
    ids, _, sc, _ = _wit("two_factors")
    f37, f19 = _gauss(3.0 / 7.0), _gauss(1.0 / 9.0)
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)]                     # A, E, D
    assert np.allclose(sc, [0.9, 0.85 * f19, 0.7 * f37 * f37], atol=2e-4)
    assert abs(sc[2] - 0.7 * f37) > 0.1                              # one factor alone is far away


def test_witness_classes_and_agnostic():
    ids, cls, sc, _ = _wit("classes")
    assert ids == [BI(5, 4), BI(5, 5), BI(1, 9)] and cls == [1, 2, 1]
    assert sc[1] == float(SC.witness("classes")[4][0, BI(5, 5), 2])   # not decayed: its float32 score, exactly
    ids, cls, sc, _ = _wit("classes", "gauss_iou_agn")
    assert ids == [BI(5, 4), BI(1, 9), BI(5, 5)] and cls == [1, 1, 2]
    assert abs(sc[2] - 0.8 * _gauss(0.6)) < 2e-4


def test_witness_floor():
    ids, _, _, r = _wit("floor")
    assert ids == [BI(5, 4), BI(1, 9)] and r[3][0] == 2               # B' = 0.389 <= 0.45 is gone
    assert len(_wit("order")[0]) == 3


def test_witness_turned_away_decays_nothing():
    ids, cls, sc, _ = _wit("turned_away", "gauss_iou_agn")
    assert ids == [BI(1, 1), BI(8, 5)] and cls == [0, 1]
    assert sc[1] == float(SC.witness("turned_away")[4][0, BI(8, 5), 1])
    # without the cap A2 is kept and X decayed
    size, ncls, heads, b, s, caps, soft = SC.witness("turned_away")
    r = _oracle(b, s, {}, soft, "gauss_iou_agn", "f64")
    assert [int(x) for x in r[4][0][:3]] == [BI(1, 1), BI(8, 4), BI(8, 5)] and abs(r[1][0][2] - 0.7 * _gauss(0.6)) < 2e-4


def test_witness_max_total_and_empty():
    ids, _, _, r = _wit("max_total")
    assert ids == [BI(1, 1), BI(5, 5)] and r[3][0] == 2 and r[4][0].shape == (2,)
    ids, _, _, r = _wit("empty")
    assert ids == [] and r[3][0] == 0 and not r[0].any() and not r[1].any() and (r[4] == -1).all()


def test_witness_ties_by_box_then_class():
    ids, cls, sc, _ = _wit("ties")
    boxes = sorted(BI(gy, gx) for gy, gx in ((7, 2), (1, 9), (4, 4), (1, 3)))
    assert ids == [b for b in boxes for _ in (0, 1)] and cls == [0, 2] * 4
    assert len(set(sc.tolist())) == 1                                # exact ties


def test_witness_linear_at_exactly_the_threshold():
    """The float32 IoU of the pair of `order` as the threshold: m > thr fails, B keeps its score; one float32 step below, it decays."""
    import nms_rule_oracle as NR
    size, ncls, heads, b, s, caps, soft = SC.witness("order")
    m = NR.measure(b[0, BI(5, 5)], b[0, [BI(5, 4)]], "iou", 1.0, np.float32)[0]
    assert abs(float(m) - 0.6) < 1e-5
    lin = ("linear", "iou", 1.0, False)
    r = _oracle(b, s, caps, soft, lin, "f32", iou_thr=float(m))
    assert [int(x) for x in r[4][0][:3]] == [BI(5, 4), BI(5, 5), BI(1, 9)] and r[1][0][1] == s[0, BI(5, 5), 1]
    r = _oracle(b, s, caps, soft, lin, "f32", iou_thr=float(np.nextafter(m, np.float32(0))))
    assert [int(x) for x in r[4][0][:3]] == [BI(5, 4), BI(1, 9), BI(5, 5)]
    assert abs(float(r[1][0][2]) - 0.8 * (1.0 - 0.6)) < 2e-4


def test_topk_case_leaves_the_65th_key_out():
    heads, b, s, loner = SC.topk_case()
    order = DC.candidate_order(s[0], SC.SCORE_THR)
    assert len(order) == 200 and int(order[SC.TOPK_SMALL][0]) == loner      # the 65th key
    r = _oracle(b, s, face="f64", top_k=SC.TOPK_SMALL)
    v = int(r[3][0])
    assert loner not in r[4][0][:v] and r[1][0][:v].min() < s[0, loner, 1]
    assert r[5] >= SC.MARGIN_BAR
    assert loner in _oracle(b, s, face="f64")[4][0]


@pytest.mark.parametrize("L", SC.EDGE_LENGTHS)
def test_edge_case_loner_is_kept_iff_it_is_a_participant(L):
    heads, b, s, loner = SC.edge_case(L)
    r = _oracle(b, s, mode=("hard", "iou", 1.0, True), face="f64")
    assert r[5] >= SC.MARGIN_BAR
    if L <= SC.TOP_K_MAX:
        assert r[3][0] == 2 and r[4][0][1] == loner
    else:
        assert r[3][0] == 1 and r[4][0][0] != loner


# ------------------------------------------------------------------------------------------------ 2. 'hard' is the rule that ships
def _same_bits(got, ref):
    for k in range(5):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, k
        assert np.array_equal(got[k].view(np.int32), ref[k].view(np.int32)), k


@pytest.mark.parametrize("name", ["s1300", "s2500"])
def test_hard_equals_combined_nms_on_the_chunk_cases(name):
    _, b, s = DC.chunk_case(name)
    assert int((s > np.float32(SC.SCORE_THR)).sum()) <= SC.TOP_K_MAX
    _same_bits(_oracle(b, s, mode=("hard", "iou", 1.0, False)), DC.chunk_reference(name))


@pytest.mark.parametrize("per_class,total", DC.CAP_PAIRS)
def test_hard_equals_combined_nms_under_the_caps(per_class, total):
    _, _, _, b, s = DC.cap_input("small6")
    got = _oracle(b, s, {"max_per_class": per_class, "max_total": total}, mode=("hard", "iou", 1.0, False))
    _same_bits(got, DC.cap_reference("small6", per_class, total))


@pytest.mark.parametrize("ncls,seed", [(3, 3), (80, 4)])
@pytest.mark.parametrize("rule", sorted(RC.RULES))
def test_hard_equals_the_rule_oracle_on_random_heads(ncls, seed, rule):
    _, b, s = RC.random_case(ncls, seed)
    kind, beta, agn = RC.RULES[rule]
    _same_bits(_oracle(b, s, mode=("hard", kind, beta, agn)), RC.random_reference(ncls, seed, rule)[:5])


# ------------------------------------------------------------------------------------------------ 3. margins of the seeded cases
def test_every_input_and_mode_has_a_seed():
    assert set(SC.RANDOM_SEEDS) == {(size, ncls, mode) for (size, ncls) in SC.RANDOM_BIAS for mode in SC.MODES}
    assert set(SC.LENGTH_SEEDS) == set(SC.LENGTHS)


@pytest.mark.parametrize("size,ncls,mode,seed", SC.RANDOM_CASES)
def test_random_case_margin(size, ncls, mode, seed):
    _, b, s = SC.random_case(size, ncls, seed)
    r = _oracle(b, s, mode=mode, face="f64")
    print(f"candidates {int((s > np.float32(SC.SCORE_THR)).sum())}, valid {int(r[3][0])}, margin {r[5]:.3e}, largest score bound {r[6].max():.3e}")
    assert r[5] >= SC.MARGIN_BAR and r[3][0] >= 10
    assert r[6].max() <= SO.global_bound(100, SC.SIGMA, SC.MODES[mode][0])
    # something was decayed, and the two faces agree on every decision
    f32 = _oracle(b, s, mode=mode, face="f32")
    for k in (2, 3, 4):
        assert np.array_equal(f32[k], r[k])
    v = int(r[3][0])
    assert (r[6][0, :v] > 0).sum() >= 5
    assert (np.abs(f32[1].astype(np.float64) - r[1]) <= r[6] * r[1]).all()


@pytest.mark.parametrize("L", SC.LENGTHS)
def test_length_case_margin(L):
    _, b, s = SC.length_case(L)
    for mode in SC.LENGTH_MODES:
        r = _oracle(b, s, mode=mode, face="f64")
        print(f"{mode}: valid {int(r[3][0])}, margin {r[5]:.3e}")
        assert r[5] >= SC.MARGIN_BAR
        assert min(L, 100) - 2 <= r[3][0] <= min(L, 100)               # (two crowd boxes fall under the floor)
        if L >= 6:
            assert (r[6][0] > 0).sum() >= (2 if mode.startswith("gauss") else 1)     # decayed crowd boxes are among the results
