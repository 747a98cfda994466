"""Decode + NMS against the oracle on EVERY path of csrc/decode_nms.hip: the generic decode kernel (C >= 81), the 16-cell decode
variant, more classes than the round-parallel pass takes, second and third NMS chunks through both sorts and the exact select,
both caps away from 100 / 100, the edges of the arithmetic, and the per-image counters across batches of changing size.

Which path a launch takes cannot be seen from outside; each input therefore carries a witness computed from the oracle alone
(tests/decode_nms_cases.py), asserted without a GPU in tests/test_decode_nms_cases_cpu.py.  Here the kernels are only fed legal
inputs and compared: valid counts, kept indices and classes identical, boxes within 1e-5, scores within 1e-6 (`_compare`, the
rule of tests/test_gpu_decode_nms.py)."""
import time

import numpy as np
import pytest

import decode_nms_cases as DC
from decode_nms_cases import _compare, _engine, _heads_with, _random_heads

pytestmark = pytest.mark.gpu


def _timed_compare(eng, cfg, heads, size, ncls, **kw):
    """`_compare` with the reference computed first, so that the printed time is the device side alone (upload, decode, NMS,
    download)."""
    ref = kw.pop("ref", None)
    if ref is None:
        ref = DC.reference(heads, ncls, cfg, size, kw.get("iou", -1.0), kw.get("score", -1.0), kw.get("per_class", 100),
                           kw.get("total", 100))
    t0 = time.perf_counter()
    out = _compare(eng, cfg, heads, size, ncls, ref=ref, **kw)
    print(f"device side: {1e3 * (time.perf_counter() - t0):.1f} ms")
    return out


# ------------------------------------------------------------------------------------------------ generic decode kernel
@pytest.mark.parametrize("size,ncls,n", [
    (96, 81, 3),           # the smallest C that leaves the cell kernel: two class sweeps, the second with 17 lanes; nbox = 567
    (96, 200, 2),          # four sweeps, the last with 8 lanes
    ((160, 96), 81, 2),    # rectangular: row / column from a cell index with gw != gh
])
def test_generic_decode_kernel(size, ncls, n):
    """decode_kernel (3 * (5 + C) > 256): one image dense, the others sparse; nbox is no multiple of the 256-lane block, so blocks
    straddle images and the last one has lanes out of range."""
    cfg, eng = _engine(size, ncls, n)
    heads = DC.generic_heads(size, ncls, n)
    if isinstance(size, int):
        got, ref = _timed_compare(eng, cfg, heads, size, ncls)
    else:
        from test_gpu_rect import rect_inference_from_heads
        H, W = size
        ref = rect_inference_from_heads(heads, ncls, cfg["anchors"], cfg["xyscale"], H, W,
                                        iou_threshold=cfg["iou_threshold"], score_threshold=cfg["score_threshold"])
        got, ref = _timed_compare(eng, cfg, heads, size, ncls, ref=ref)
    assert got[3].sum() > 0 and got[3][1] == 100
    assert (got[2][got[4] >= 0] >= 64).any()            # a class of the second sweep is among the kept ones
    eng.close()


# ------------------------------------------------------------------------------------------------ C > PAR_MAX_C
def test_more_classes_than_the_round_parallel_pass_takes():
    """C = 1025: the FIRST chunk goes through the wave-0 pass.  Image 0 random, image 1 a stack on class 1024 between disjoint
    boxes of class 0: suppression and order decide which 100 come out."""
    ncls = DC.PAR_MAX_C + 1
    cfg, eng = _engine(96, ncls, 2)
    got, ref = _timed_compare(eng, cfg, DC.many_class_heads(), 96, ncls)
    assert got[3].tolist() == [100, 100]
    assert (got[2][1] == ncls - 1).sum() == 1 and (got[2][1] == 0).sum() == 99
    eng.close()


# ------------------------------------------------------------------------------------------------ 16-cell decode variant
@pytest.mark.parametrize("ncls", sorted(DC.DENSE_CASES))
def test_sixteen_cell_decode_variant(ncls):
    """decode_launch takes decode_cell_kernel<16> once N * cells_per_img >= 16 * 8192.  At 96^2 an image has 189 cells -- no
    multiple of 16, so waves straddle images -- and N16 = ceil(16 * 8192 / 189) = 694 is the smallest such batch.  All N16
    images against the oracle; then the first N16 - 1 images on the same engine, which the 4-cell variant decodes: the candidate
    lists come in another order, NMS sorts them, every row must be the same bit for bit.
    This is the suite's one larger decode test (C = 80: 127 MB of heads)."""
    n = DC.n16(DC.CELLS_DENSE)
    assert n * DC.CELLS_DENSE >= DC.DC_SCREEN * DC.DC_SCREEN_MIN_WAVES > (n - 1) * DC.CELLS_DENSE
    heads, ref, _ = DC.dense_case(ncls)
    cfg, eng = _engine(DC.SIZE_DENSE, ncls, n)
    got, _ = _timed_compare(eng, cfg, heads, DC.SIZE_DENSE, ncls, ref=ref)
    assert all(got[3][i] == 100 for i in DC.dense_positions(n))
    t0 = time.perf_counter()
    m = eng.set_heads([h[:n - 1] for h in heads])
    small = [o.cpu().numpy() for o in eng.decode_nms_device(m)]
    print(f"device side, N16 - 1: {1e3 * (time.perf_counter() - t0):.1f} ms")
    for a, b in zip(small, got):
        assert np.array_equal(a.view(np.int32), b[:n - 1].view(np.int32))
    eng.close()


# ------------------------------------------------------------------------------------------------ later chunks
@pytest.mark.parametrize("name", sorted(DC.CHUNK_CASES))
def test_later_chunks(name):
    """The stack-and-disjoint images: the oracle's last kept box lies behind the whole stack, in a second chunk that is rank
    sorted (s1300), goes through the register bitonic network at 2048 / 4096 keys (s2500, s4400, s4500), or in a third chunk
    behind an exact select with a finite cutoff (s5400)."""
    heads, _, _ = DC.chunk_case(name)
    cfg, eng = _engine(DC.SIZE_CHUNK, 2, 1)
    got, _ = _timed_compare(eng, cfg, heads, DC.SIZE_CHUNK, 2, ref=DC.chunk_reference(name))
    assert got[3][0] == 100 and (got[2][0] == 0).sum() == 1
    eng.close()


def test_later_chunks_differ_within_one_launch():
    """Three of them in one batch: one workgroup per image, each on its own path."""
    names = ("s5400", "s1300", "s2500")
    heads = [np.concatenate([DC.chunk_case(nm)[0][s] for nm in names], axis=0) for s in range(3)]
    ref = [np.concatenate([DC.chunk_reference(nm)[k] for nm in names], axis=0) for k in range(5)]
    cfg, eng = _engine(DC.SIZE_CHUNK, 2, 3)
    _timed_compare(eng, cfg, heads, DC.SIZE_CHUNK, 2, ref=ref)
    eng.close()


def test_iou_zero_visits_every_chunk():
    """iou_threshold = 0.0 on dense heads (9 255 candidates): the kept list never fills, and the last kept boxes -- zero-area,
    so nothing suppresses them -- are the very last candidates."""
    heads, ref, w = DC.iou_zero_case()
    assert w["rank"] > DC.NMS_THREADS + DC.SORT_CAP
    cfg, eng = _engine(DC.SIZE_IOU0, 3, 1)
    got, _ = _timed_compare(eng, cfg, heads, DC.SIZE_IOU0, 3, iou=0.0, ref=ref)
    assert got[3][0] == w["valid"]
    eng.close()


# ------------------------------------------------------------------------------------------------ caps
@pytest.mark.parametrize("per_class,total,inp", DC.CAP_CASES)
def test_caps(per_class, total, inp):
    """max_per_class and max_total away from 100 / 100, on an input of one chunk (round-parallel pass: pcount / pflag) and on
    inputs whose decision falls in a later chunk (wave-0 pass: the same-class count)."""
    size, ncls, heads, _, _ = DC.cap_input(inp)
    cfg, eng = _engine(size, ncls, 1, max_per_class=per_class, max_total=total)
    got, ref = _timed_compare(eng, cfg, heads, size, ncls, per_class=per_class, total=total,
                              ref=DC.cap_reference(inp, per_class, total))
    v = int(got[3][0])
    assert [g.shape[1] for g in (got[0], got[1], got[2], got[4])] == [total] * 4           # max_total rows ...
    assert not got[0][0, v:].any() and not got[1][0, v:].any() and not got[2][0, v:].any()  # ... zero padded
    assert np.all(got[4][0, v:] == -1) and np.all(got[4][0, :v] >= 0)
    cls = got[2][0, :v].astype(int)
    assert np.bincount(cls, minlength=ncls).max() <= per_class
    if inp == "grid2704":
        assert v == 1024
    if (per_class, total, inp) == (2, 1024, "dense6"):
        assert v == 12
    eng.close()


def test_caps_out_of_range_are_refused():
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    for caps in ({"max_total": 1025}, {"max_per_class": 0}, {"max_total": 0}):
        with pytest.raises(ext.Y4Error) as e:
            Engine(2, make_config(96), max_batch=1, dtype="bf16", **caps)
        assert e.value.code == -22                      # Y4_EINVAL


def test_sibling_carries_the_caps():
    cfg, eng = _engine(96, 3, 1, max_per_class=2, max_total=5)
    sib = eng.sibling()
    assert (sib.cfg.max_per_class, sib.cfg.max_total, sib.T) == (2, 5, 5)
    heads = _random_heads(np.random.default_rng(4), 1, 96, 3, 1.0, 0.0)
    _compare(sib, cfg, heads, 96, 3, per_class=2, total=5)
    sib.close()
    eng.close()


# ------------------------------------------------------------------------------------------------ arithmetic edges
def test_wh_overflow_and_underflow():
    """expf of a wh logit of 95 is inf: inf corners, NaN IoU between two such boxes (never > threshold: both stay), clipped to
    (0, 0, 1, 1); of -110 it is 0: a zero-area box, IoU 0 with everything."""
    cfg, eng = _engine(96, 3, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        got, ref = _timed_compare(eng, cfg, DC.overflow_heads(), 96, 3)
    assert got[3][0] == 100 and not any(np.isnan(g).any() for g in got)
    kb = got[0][0]
    assert np.all(kb == np.array([0, 0, 1, 1], np.float32), axis=1).any()
    assert ((kb[:, 2] == kb[:, 0]) & (kb[:, 3] == kb[:, 1])).any()
    eng.close()


def test_score_equal_to_the_threshold_is_no_candidate():
    """All-zero logits: every score is exactly 0.25.  At score_threshold = 0.25 nothing passes (strict >); just below it, all do."""
    size, ncls = 96, 3
    cfg, eng = _engine(size, ncls, 1)
    heads = [np.zeros((1, size // s, size // s, 3 * (5 + ncls)), np.float32) for s in (8, 16, 32)]
    got, _ = _timed_compare(eng, cfg, heads, size, ncls, score=0.25)
    assert got[3][0] == 0 and np.all(got[4] == -1)
    got, _ = _timed_compare(eng, cfg, heads, size, ncls, score=0.24999999)
    assert got[3][0] == 100 and np.all(got[1][0] == 0.25)
    eng.close()


# ------------------------------------------------------------------------------------------------ counters across batches
def test_counters_when_the_batch_shrinks_and_grows():
    """One engine, max_batch 3: dense n = 3, sparse n = 1, dense n = 3 again.  NMS leaves its images' candidate counters at zero
    and the handle remembers whether all of them are; every run equals its oracle and the third the first, bit for bit."""
    size, ncls = 160, 5
    cfg, eng = _engine(size, ncls, 3)
    dense = _random_heads(np.random.default_rng(21), 3, size, ncls, 1.0, 0.0)
    sparse = _random_heads(np.random.default_rng(22), 1, size, ncls, -6.0, -2.0)
    first, ref = _timed_compare(eng, cfg, dense, size, ncls)
    assert first[3].min() > 1
    _timed_compare(eng, cfg, sparse, size, ncls)
    third, _ = _timed_compare(eng, cfg, dense, size, ncls, ref=ref)
    for a, b in zip(first, third):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    eng.close()
