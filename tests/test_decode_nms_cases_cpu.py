"""The conditions on the inputs of tests/test_gpu_decode_nms_paths.py, checked with the oracle alone (no GPU): every case
carries a witness (tests/decode_nms_cases.py) that it reaches the path of decode_nms.hip it is meant for.  A witness that stops
holding -- a generator changed, a kernel constant changed and was restated in decode_nms_cases.py -- fails HERE, instead of the
GPU test silently going back to the common path."""
import numpy as np
import pytest

import decode_nms_cases as DC
import nms_rule_cases as RC
from decode_nms_cases import NMS_THREADS, SORT_CAP


def _cfg(size):
    from yolo4hip.config import make_config
    return make_config(size)


def _witness(name):
    _, _, s = DC.chunk_case(name)
    ref = DC.chunk_reference(name)
    return DC.chunk_witness(s[0], _cfg(DC.SIZE_CHUNK)["score_threshold"], (ref[4][0], ref[2][0], ref[3][0]))


# ------------------------------------------------------------------------------------------------ the witnesses themselves
def test_candidate_order_and_rank_on_a_hand_made_image():
    scores = np.array([[0.5, 0.9], [0.9, 0.3], [0.9, 0.9], [0.31, 0.0]], np.float32)
    order = DC.candidate_order(scores, 0.3)
    # 0.9s first: box asc, then class asc; 0.3 itself is no candidate (strict)
    assert order.tolist() == [[0, 1], [1, 0], [2, 0], [2, 1], [0, 0], [3, 0]]
    kept_idx = np.array([0, 2, 3, -1]); classes = np.array([1.0, 0.0, 0.0, 0.0])
    assert DC.ranks_of_kept(order, kept_idx, classes, 3) == [0, 2, 5]
    assert DC.rank_of_last_kept(order, kept_idx, classes, 3) == 5
    assert DC.rank_of_last_kept(order, kept_idx, classes, 0) == -1


def test_chunk_bounds():
    assert DC.first_chunk_bounds(1000) == (1000, 1000) and DC.second_chunk_bounds(1024) == (0, 0)
    assert DC.first_chunk_bounds(1025) == (512, 1024) and DC.second_chunk_bounds(1460) == (436, 948)


def test_wave_flushes_replay():
    # C = 80: a cell adds up to 240 keys, the slice takes 512: the third full cell of a wave flushes ("full"); an image boundary
    # inside a wave flushes what is staged ("change"); cells without candidates are never visited
    counts = np.zeros(32, int)
    counts[[0, 1, 2]] = 240
    assert DC.wave_flushes(counts, 1000, 80) == [(1, 0), (0, 0)]
    counts[:] = 0
    counts[[17, 22]] = 5
    assert DC.wave_flushes(counts, 20, 80) == [(0, 0), (0, 1)]
    assert DC.wave_flushes(counts, 16, 80) == [(0, 0), (0, 0)]        # the boundary is the wave's own: nothing staged before it
    assert DC.n16(189) == 694 and 693 * 189 < 16 * 8192 <= 694 * 189


# ------------------------------------------------------------------------------------------------ later chunks
@pytest.mark.parametrize("name,T,rank", [("s1300", 1460, 1398), ("s2500", 2660, 2598), ("s4500", 4660, 4598), ("s5400", 5560, 5498)])
def test_stack_cases_have_the_measured_figures(name, T, rank):
    w = _witness(name)
    assert (w["T"], w["rank"], w["valid"]) == (T, rank, 100), w
    ref = DC.chunk_reference(name)
    assert np.bincount(ref[2][0].astype(int)).tolist() == [1, 99]


def test_s1300_second_chunk_is_rank_sorted():
    w = _witness("s1300")
    assert w["T"] > NMS_THREADS and w["rank"] >= NMS_THREADS          # the first chunk cannot hold the last kept box
    assert 0 < w["rem_lo"] and w["rem_hi"] <= NMS_THREADS                # what remains pads to at most 1024: the rank sort


@pytest.mark.parametrize("name", ["s2500", "s2500d200"])
def test_s2500_second_chunk_takes_the_register_bitonic_sort(name):
    w = _witness(name)
    assert w["rank"] >= NMS_THREADS
    assert w["rem_lo"] > NMS_THREADS and w["rem_hi"] <= SORT_CAP         # pads to 2048 or 4096, no select
    if name == "s2500d200":
        assert w["kept_before_last_batch"] > 64, w                       # the wave-0 pass reads a kept list longer than one wave


@pytest.mark.parametrize("name", ["s4500", "s4400"])
def test_s4500_second_chunk_is_4096_keys(name):
    w = _witness(name)
    assert w["rank"] >= NMS_THREADS
    assert w["rem_lo"] > SORT_CAP // 2                                    # pads to 4096: both in-thread exchange distances
    if name == "s4400":
        assert w["rem_hi"] <= SORT_CAP                                    # ... and whatever the first chunk took, no select
    else:
        assert w["rem_hi"] <= SORT_CAP + NMS_THREADS // 2                 # (a first chunk under 564 keys leaves a 4096-key select)
    assert w["rank"] >= w["T"] - 64 - 64                                  # the last kept box is in the chunk's last batches


def test_s5400_needs_a_select_with_a_finite_cutoff_and_a_third_chunk():
    w = _witness("s5400")
    assert w["rem_lo"] > SORT_CAP                                         # more than a chunk remains: exact select below the cutoff
    assert w["rank"] >= NMS_THREADS + SORT_CAP                           # the first two chunks cannot hold the last kept box
    assert w["rem_hi"] - SORT_CAP <= NMS_THREADS                          # the third chunk is rank sorted


@pytest.mark.parametrize("name,rule", RC.LATER_CHUNK_CASES)
def test_rule_cases_are_decided_in_a_later_chunk(name, rule):
    """The inputs of test_gpu_nms_rule.test_rule_goes_on_in_a_later_chunk: under the rule, the oracle's last kept box still ranks
    behind everything a first chunk can hold, and the first chunk has kept boxes for the later pass to continue from."""
    w = RC.later_chunk_witness(name, rule)
    ref = RC.later_chunk_reference(name, rule)
    assert w["T"] > NMS_THREADS and w["rank"] >= NMS_THREADS, w
    assert any(r < NMS_THREADS // 2 for r in w["ranks"])                  # kept by the first chunk's pass, whatever its pivot
    assert sum(1 for r in w["ranks"] if r >= NMS_THREADS) > 1             # more than one box is kept by the later chunk's pass
    if name == "s1300":
        assert 0 < w["rem_lo"] and w["rem_hi"] <= NMS_THREADS             # the later chunk is rank sorted
    else:
        assert w["rem_lo"] > NMS_THREADS and w["rem_hi"] <= SORT_CAP      # ... goes through nms_sort_regs, no select
    # no tested pair hangs on the last bits of the measure: it is some ten float32 operations on values <= 1 (half an ulp, 6e-8,
    # each) and one powf (a few ulp of a penalty < 0.1), so two correct float32 evaluations differ by well under 1e-6
    assert ref[5] >= 1e-6, ref[5]
    assert ref[3][0] == 100


def test_iou_zero_dense_case_visits_more_than_two_chunks():
    heads, ref, w = DC.iou_zero_case()
    assert w["rank"] > NMS_THREADS + SORT_CAP, w
    assert w["valid"] < 100                                               # never full: every candidate is visited


# ------------------------------------------------------------------------------------------------ caps
@pytest.mark.parametrize("per_class,total,inp", DC.CAP_CASES)
def test_cap_cases_bind(per_class, total, inp):
    size, ncls, _, _, s = DC.cap_input(inp)
    thr = _cfg(size)["score_threshold"]
    T = int((s > np.float32(thr)).sum())
    if inp == "small6":
        assert T <= NMS_THREADS, T                 # one chunk: the round-parallel pass
    else:
        assert T > NMS_THREADS + 512, T            # the greedy pass goes on in a later chunk
    unc = DC.cap_reference(inp, None, None)
    capped = DC.cap_reference(inp, per_class, total)
    survivors = np.bincount(unc[2][0, :unc[3][0]].astype(int), minlength=ncls)
    if (per_class, total, inp) in DC.CAP_CANNOT_BIND:
        assert survivors.sum() < total and capped[3][0] == unc[3][0] == survivors.sum()
        assert inp != "s2500" or capped[3][0] > 100
        return
    capped_sum = int(np.minimum(survivors, per_class).sum())
    if per_class < total:                          # the kernel's cap_binds: a class is turned away ...
        assert survivors.max() > per_class, survivors
        k = capped[3][0]                           # ... and it shows: the result is not the uncapped one cut to its length
        assert not (np.array_equal(capped[4][0, :k], unc[4][0, :k]) and np.array_equal(capped[2][0, :k], unc[2][0, :k]))
    else:                                          # max_total binds
        assert survivors.sum() > total
    assert capped[3][0] == min(total, capped_sum) < unc[3][0]
    if inp == "s2500" and per_class < total:
        # the cap decides in a LATER chunk: the capped run never fills max_total, so it visits every candidate, and behind the
        # first chunk lie boxes that nothing suppresses (the uncapped run keeps them) -- only the full class turns them away
        order = DC.candidate_order(s[0], thr)
        late = [(int(unc[4][0, k]), int(unc[2][0, k])) for k, r in
                enumerate(DC.ranks_of_kept(order, unc[4][0], unc[2][0], unc[3][0])) if r >= NMS_THREADS]
        mine = {(int(capped[4][0, k]), int(capped[2][0, k])) for k in range(capped[3][0])}
        assert capped[3][0] < total and len(late) > 64 and not mine & set(late)


def test_grid_case_ties_and_fills_1024():
    size, ncls, _, _, s = DC.cap_input("grid2704")
    thr = _cfg(size)["score_threshold"]
    vals = s[s > np.float32(thr)]
    assert vals.size == 2704 and np.all(vals == vals[0])       # one score: one histogram bin holds everything -> exact select of 1024
    ref = DC.cap_reference("grid2704", 1024, 1024)
    assert ref[3][0] == 1024 and np.array_equal(ref[4][0], np.arange(1024) * 3)     # anchor 0 of the first 1024 cells, in index order


# ------------------------------------------------------------------------------------------------ 16-cell decode variant
@pytest.mark.parametrize("ncls", sorted(DC.DENSE_CASES))
def test_dense_cases_flush_inside_a_wave(ncls):
    heads, ref, counts = DC.dense_case(ncls)
    n = heads[0].shape[0]
    assert n == DC.n16(DC.CELLS_DENSE) and n * DC.CELLS_DENSE >= DC.DC_SCREEN * DC.DC_SCREEN_MIN_WAVES > (n - 1) * DC.CELLS_DENSE
    assert DC.CELLS_DENSE % DC.DC_SCREEN != 0
    fl = DC.wave_flushes(counts, DC.CELLS_DENSE, ncls)
    spans = [g for g in range(len(fl)) if (g * 16) // DC.CELLS_DENSE != min(g * 16 + 15, len(counts) - 1) // DC.CELLS_DENSE]
    assert any(fl[g][1] > 0 for g in spans)                     # staged keys of one image written out because the next begins
    assert ref[3].min() == 0 or ref[3].min() < 100              # sparse images are sparse ...
    assert all(ref[3][i] == 100 for i in DC.dense_positions(n))  # ... and the dense ones full
    if 16 * 3 * ncls > DC.DC_STAGE:                            # (C = 3: sixteen cells hold 144 keys at most, the slice never fills)
        group_max = max(int(counts[g:g + 16].sum()) for g in range(0, len(counts), 16))
        assert group_max > DC.DC_STAGE - 3 * ncls
        assert any(f > 0 for f, _ in fl)                        # the slice-full flush
        assert any(f > 0 and c > 0 for (f, c), g in zip(fl, range(len(fl))) if g in spans)      # both kinds inside ONE wave


# ------------------------------------------------------------------------------------------------ generic kernel, many classes, edges
@pytest.mark.parametrize("size,ncls,n", [(96, 81, 3), (96, 200, 2), ((160, 96), 81, 2)])
def test_generic_decode_cases_leave_the_cell_kernel(size, ncls, n):
    assert 3 * (5 + ncls) > DC.CELL_KERNEL_MAX_VALUES
    heads = DC.generic_heads(size, ncls, n)
    H, W = (size, size) if isinstance(size, int) else size
    nbox = 3 * sum((H // s) * (W // s) for s in (8, 16, 32))
    assert heads[0].shape == (n, H // 8, W // 8, 3 * (5 + ncls))
    assert (n * nbox) % 256 != 0 and nbox % 256 != 0            # blocks straddle images; the last block has lanes out of range


def test_many_class_case():
    ncls = DC.PAR_MAX_C + 1
    heads = DC.many_class_heads()
    cfg = _cfg(96)
    b, s = DC.boxes_and_scores(heads, ncls, cfg, 96)
    ref = DC.reference(heads, ncls, cfg, 96)
    assert ref[3].tolist() == [100, 100]
    T = int((s[1] > np.float32(cfg["score_threshold"])).sum())
    assert T <= NMS_THREADS                                     # one chunk: the wave-0 pass takes it because C > PAR_MAX_C
    order = DC.candidate_order(s[1], cfg["score_threshold"])
    assert DC.rank_of_last_kept(order, ref[4][1], ref[2][1], ref[3][1]) > 288      # behind the whole stack
    cls = ref[2][1].astype(int)
    assert (cls == ncls - 1).sum() == 1 and (cls == 0).sum() == 99


def test_overflow_case_under_the_oracle():
    heads = DC.overflow_heads()
    cfg = _cfg(96)
    with np.errstate(over="ignore"):
        b, s = DC.boxes_and_scores(heads, 3, cfg, 96)
    assert np.isinf(b).any() and not np.isnan(b).any()
    ref = DC.reference(heads, 3, cfg, 96)
    assert ref[3][0] == 100 and not any(np.isnan(r).any() for r in ref)
    kb = ref[0][0]
    assert (np.all(kb == np.array([0, 0, 1, 1], np.float32), axis=1)).any()            # an inf box, clipped
    assert ((kb[:, 2] == kb[:, 0]) & (kb[:, 3] == kb[:, 1])).any()                      # a zero-area box is kept
