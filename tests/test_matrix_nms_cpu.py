"""The Matrix-NMS oracle (tests/matrix_nms_oracle.py) and the inputs of tests/matrix_nms_cases.py, without a GPU: the oracle on
hand-computed witnesses, against the Soft-NMS oracle where the two rules coincide, and the margin of every seeded case.

The margin bar.  The device works in float32, the float64 face of the oracle behind the (float32) measure in float64.  A score is
decayed ONCE, by one term and one product: matrix_nms_oracle.term_ulps derives (a + b) / sigma + 2 |a - b| / sigma + 2 EXPF_ULPS units
of 2^-24 for the gaussian term (a = c^2, b = m^2 in [0, 1]: at most 10 at sigma = 0.5) and 3 for the linear one, plus 1 for the
product -- 6.6e-7 at the very most, where Soft-NMS accumulates up to max_total decays.  A decision whose two sides are at least 1e-4
apart (relative) in the float64 face is the same decision in float32 with two orders of magnitude to spare; the bar is the
project's (soft_nms_cases.MARGIN_BAR).  Every seeded case must show that margin; a seed that does not is replaced in
matrix_nms_cases.py."""
import time

import numpy as np
import pytest

import decode_nms_cases as DC
import matrix_nms_cases as MC
import matrix_nms_oracle as MX
import soft_nms_cases as SC
import soft_nms_oracle as SO


def _oracle(b, s, caps=None, kw=None, mode="gauss_iou", face="f64", top_k=SC.TOP_K_MAX):
    caps, kw = caps or {}, kw or {}
    method, kind, beta, agn = MC.MODES[mode] if isinstance(mode, str) else mode
    return MX.matrix_nms(b, s, caps.get("max_per_class", 100), caps.get("max_total", 100), SC.SCORE_THR, kind, beta, agn, method,
                         SC.SIGMA, kw.get("min_score"), top_k, face)


def _soft(b, s, mode="gauss_iou", face="f32"):
    method, kind, beta, agn = MC.MODES[mode]
    return SO.soft_nms(b, s, 100, 100, SC.IOU_THR, SC.SCORE_THR, kind, beta, agn, method, SC.SIGMA, None, SC.TOP_K_MAX, face)


def _wit(name, mode="gauss_iou", face="f64", **over):
    size, ncls, heads, b, s, caps, kw = MC.witness(name)
    r = _oracle(b, s, caps, dict(kw, **over), mode, face)
    v = int(r[3][0])
    return [int(x) for x in r[4][0][:v]], [int(x) for x in r[2][0][:v]], r[1][0][:v].astype(np.float64), r


def _gauss(x):
    return float(np.exp(x / SC.SIGMA))


BI = lambda gy, gx: SC.box_index(SC.SIZE, gy, gx)      # noqa: E731


# ------------------------------------------------------------------------------------------------ 1. the issue's four witnesses
def test_the_bound_stays_under_the_margin_bar():
    assert MX.global_bound(SC.SIGMA, "gaussian") < 0.01 * MC.MARGIN_BAR
    assert MX.global_bound(SC.SIGMA, "linear") < 0.01 * MC.MARGIN_BAR


def test_witness_decay_is_the_minimum_not_the_product():
    ids, _, sc, _ = _wit("two_factors")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)]                     # A, E, D
    # E: exp(-(1/9)^2 / sigma).  D: A's term exp(-(3/7)^2 / sigma), E's term exp(((1/9)^2 - (3/7)^2) / sigma) is the larger one
    assert np.allclose(sc, [0.9, 0.82927, 0.48480], atol=1e-5)
    assert abs(sc[2] - 0.7 * _gauss(-(3.0 / 7.0) ** 2)) < 2e-4
    soft = _soft(*MC.witness("two_factors")[3:5], face="f64")
    assert abs(soft[1][0][2] - 0.33576) < 1e-5 and sc[2] - soft[1][0][2] > 0.1      # Soft-NMS multiplies both factors
    ids, _, sc, _ = _wit("two_factors", "lin_iou")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)] and np.allclose(sc, [0.9, 0.75556, 0.4], atol=1e-5)


def test_witness_chain_is_compensated():
    ids, _, sc, r = _wit("chain")
    assert ids == [BI(5, 4), BI(5, 6), BI(5, 5)] and r[3][0] == 3     # A, C, B'
    assert np.allclose(sc, [0.9, 0.66595, 0.38940], atol=1e-5)
    # C: A's term exp(-0.158^2 / sigma) = 0.951 against B's compensated term exp((0.6^2 - 0.375^2) / sigma) > 1: the minimum is A's.
    # Without the compensation B's term would be exp(-0.375^2 / sigma) and C 0.52839
    m_ac, m_bc = 6.0 * 20 / (32 * 20 + 12 * 20 - 6.0 * 20), 12.0 * 20 / (32 * 20)       # A [20, 52], B [28, 60], C [46, 58]
    assert abs(m_ac - 0.158) < 1e-3 and abs(sc[1] - 0.7 * _gauss(-m_ac ** 2)) < 2e-4
    assert abs(0.7 * _gauss(-m_bc ** 2) - 0.52839) < 1e-5 and sc[1] - 0.52839 > 0.1
    soft = _soft(*MC.witness("chain")[3:5], face="f64")
    assert soft[3][0] == 2                                            # Soft-NMS: A's and B''s factors push C under the floor


def test_witness_two_candidates_of_a_class_are_soft_nms_bit_for_bit():
    _, _, _, b, s, _, _ = MC.witness("order")
    mx, so = _oracle(b, s, face="f32"), _soft(b, s)
    for k in range(5):
        assert mx[k].dtype == so[k].dtype and np.array_equal(mx[k].view(np.int32), so[k].view(np.int32)), k
    assert mx[4][0][:3].tolist() == [BI(5, 4), BI(1, 9), BI(5, 5)] and float(mx[1][0][2]) == 0.3894016444683075
    _, b, s = MC.pairs_case()
    mx, so = _oracle(b, s, face="f32"), _soft(b, s)
    for k in range(5):
        assert np.array_equal(mx[k].view(np.int32), so[k].view(np.int32)), k
    assert (mx[1][0] < 0.5).sum() >= 10                               # decayed scores are among the results


def test_witness_classes_and_agnostic():
    ids, cls, sc, _ = _wit("classes")
    assert ids == [BI(5, 4), BI(5, 5), BI(1, 9)] and cls == [1, 2, 1]
    assert sc[1] == float(MC.witness("classes")[4][0, BI(5, 5), 2])   # not decayed: its float32 score, exactly
    ids, cls, sc, _ = _wit("classes", "gauss_iou_agn")
    assert ids == [BI(5, 4), BI(1, 9), BI(5, 5)] and cls == [1, 1, 2] and abs(sc[2] - 0.38940) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. further witnesses
def test_witness_floor_is_strict():
    ids, _, _, r = _wit("floor")
    assert ids == [BI(5, 4), BI(1, 9)] and r[3][0] == 2               # B' = 0.389 <= 0.45 is gone
    bp = _wit("order", face="f32")[2][2]                              # B' in float32
    assert _wit("order", face="f32", min_score=float(bp))[0] == [BI(5, 4), BI(1, 9)]
    assert _wit("order", face="f32", min_score=float(np.nextafter(np.float32(bp), np.float32(0))))[0] == [BI(5, 4), BI(1, 9), BI(5, 5)]


def test_witness_a_skipped_candidate_still_decays():
    ids, cls, sc, _ = _wit("skipped_still_decays", "gauss_iou_agn")
    assert ids == [BI(1, 1), BI(8, 5)] and cls == [0, 1]              # A; A2 skipped (its class is full); X
    assert abs(sc[1] - 0.7 * _gauss(-0.36)) < 2e-4                    # ... decayed by A2 all the same
    size, ncls, heads, b, s, caps, kw = MC.witness("skipped_still_decays")
    r = _oracle(b, s, {}, kw, "gauss_iou_agn")
    assert [int(x) for x in r[4][0][:3]] == [BI(1, 1), BI(8, 4), BI(8, 5)] and abs(r[1][0][2] - sc[1]) == 0.0


def test_witness_max_total_ties_and_empty():
    ids, _, _, r = _wit("max_total")
    assert ids == [BI(1, 1), BI(5, 5)] and r[3][0] == 2 and r[4][0].shape == (2,)
    ids, cls, sc, _ = _wit("ties")
    boxes = sorted(BI(gy, gx) for gy, gx in ((7, 2), (1, 9), (4, 4), (1, 3)))
    assert ids == [b for b in boxes for _ in (0, 1)] and cls == [0, 2] * 4 and len(set(sc.tolist())) == 1
    ids, _, _, r = _wit("empty")
    assert ids == [] and r[3][0] == 0 and not r[0].any() and not r[1].any() and (r[4] == -1).all()


def test_witness_identical_boxes_under_linear():
    for face in ("f32", "f64"):
        ids, cls, sc, r = _wit("identical", "lin_iou_agn", face)
        assert ids == [BI(5, 5)] and cls == [0] and np.isfinite(r[1]).all()      # c = 1: the second's term is left out; both others 0
    assert len(_wit("identical", "lin_iou")[0]) == 3                  # class-aware: three classes, nothing interacts


def test_topk_case_leaves_the_65th_key_out():
    heads, b, s, loner = SC.topk_case()
    r = _oracle(b, s, top_k=SC.TOPK_SMALL)
    v = int(r[3][0])
    assert loner not in r[4][0][:v] and r[1][0][:v].min() < s[0, loner, 1] and r[5] >= MC.MARGIN_BAR
    assert loner in _oracle(b, s)[4][0]


@pytest.mark.parametrize("L", SC.EDGE_LENGTHS)
def test_edge_case_loner_is_kept_iff_it_is_a_participant(L):
    """4095 keys that all interact with each other under an agnostic rule: the whole stack behind its best key falls under the floor."""
    heads, b, s, loner = SC.edge_case(L)
    t0 = time.time()
    for mode in ("gauss_iou_agn", "lin_iou_agn"):
        r = _oracle(b, s, mode=mode)
        assert r[5] >= MC.MARGIN_BAR
        if L <= SC.TOP_K_MAX:
            assert r[3][0] == 2 and r[4][0][1] == loner
        else:
            assert r[3][0] == 1 and r[4][0][0] != loner
    assert time.time() - t0 < 30.0                                    # seconds, not minutes


def test_disjoint_case_decays_nothing():
    _, b, s = MC.disjoint_case()
    order = np.sort(s[s > np.float32(SC.SCORE_THR)])[::-1][:100]
    for mode in ("gauss_iou", "lin_iou"):
        r = _oracle(b, s, mode=mode, face="f32")
        assert r[3][0] == 100 and np.array_equal(r[1][0], order) and not r[6].any()


# ------------------------------------------------------------------------------------------------ 3. margins of the seeded cases
def test_every_input_and_mode_has_a_seed():
    assert set(MC.RANDOM_SEEDS) == {(size, ncls, mode) for (size, ncls) in MC.SHAPES for mode in MC.MODES}
    assert set(MC.LENGTH_SEEDS) == set(SC.LENGTHS)
    assert {m[:2] for m in MC.MODES.values()} == {(a, k) for a in MX.METHODS for k in ("iou", "diou")}


@pytest.mark.parametrize("size,ncls,mode,seed", MC.RANDOM_CASES)
def test_random_case_margin(size, ncls, mode, seed):
    _, b, s = MC.random_case(size, ncls, seed)
    r = _oracle(b, s, mode=mode)
    print(f"candidates {int((s > np.float32(SC.SCORE_THR)).sum())}, valid {int(r[3][0])}, margin {r[5]:.3e}, largest score bound {r[6].max():.3e}")
    assert r[5] >= MC.MARGIN_BAR and r[3][0] >= 10
    method, kind, beta, _ = MC.MODES[mode]
    if kind == "iou":
        assert r[6].max() <= MX.global_bound(SC.SIGMA, method)
    # something was decayed, and the two faces agree on every decision
    f32 = _oracle(b, s, mode=mode, face="f32")
    for k in (2, 3, 4):
        assert np.array_equal(f32[k], r[k])
    v = int(r[3][0])
    assert (r[6][0, :v] > 0).sum() >= 5
    assert (np.abs(f32[1].astype(np.float64) - r[1]) <= r[6] * r[1]).all()


@pytest.mark.parametrize("L", SC.LENGTHS)
def test_length_case_margin(L):
    _, b, s = SC.length_case(L, MC.LENGTH_SEEDS[L])
    for mode in MC.LENGTH_MODES:
        r = _oracle(b, s, mode=mode)
        print(f"{mode}: valid {int(r[3][0])}, margin {r[5]:.3e}")
        assert r[5] >= MC.MARGIN_BAR and r[3][0] == min(L, 100)
        if L >= 6:
            assert (r[6][0] > 0).sum() >= 2                            # decayed crowd boxes are among the results


@pytest.mark.parametrize("per_class,total,mode,seed", MC.CAP_RANDOM)
def test_capped_random_case_margin(per_class, total, mode, seed):
    _, b, s = MC.random_case(96, 3, seed)
    caps = {"max_per_class": per_class, "max_total": total}
    r = _oracle(b, s, caps, mode=mode)
    v = int(r[3][0])
    assert r[5] >= MC.MARGIN_BAR and (r[6][0, :v] > 0).sum() >= 2
    assert v <= total and np.bincount(r[2][0][:v].astype(np.int64)).max() == min(per_class, v)      # the cap binds
    assert not np.array_equal(r[4], _oracle(b, s, {"max_total": total}, mode=mode)[4])


@pytest.mark.parametrize("per_class,total,inp", [c for c in DC.CAP_CASES if c[2] in MC.CAP_INPUTS])
def test_cap_input_margin(per_class, total, inp):
    _, _, _, b, s = DC.cap_input(inp)
    for mode in MC.CAP_MODES:
        r = _oracle(b, s, {"max_per_class": per_class, "max_total": total}, mode=mode)
        v = int(r[3][0])
        assert r[5] >= MC.MARGIN_BAR and 1 <= v <= total and np.bincount(r[2][0][:v].astype(np.int64)).max() <= per_class
