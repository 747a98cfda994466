"""Cached frozen features: y4_feature_store / y4_feature_load / y4_forward_tail through the Engine, and
`Yolov4.fit(cache_features=True)` against the uncached call.  Everything is compared with ==: a cache row holds the bits the
forward wrote, and by the canonical K order a conv gives the same bits in whatever launch it runs.

3 classes, synthetic weights, no tuning; 160 x 160 and 96 x 160 -- the smallest inputs with three grids (20 / 10 / 5 cells and
12x20 / 6x10 / 3x5), a retained tensor of every channel count, and, at max_batch 4 with 3 images (the Engine tests) or batches of
3 through max_batch 2 (fit), a partial chunk."""
import functools
import os

import numpy as np
import pytest

import loss_cases as LC
from helpers import CLASS_DIR
from test_loss_cpu import _write_dataset

pytestmark = pytest.mark.gpu

NCLS = 3
SHAPES = [(160, 160), (96, 160)]
CACHED = {1: (92, 100, 108), 2: (91, 99, 107)}           # the convs whose outputs a row holds, per retention level
TAIL = {1: (93, 101, 109), 2: (92, 100, 108, 93, 101, 109)}
ES = {"f32": 4, "bf16": 2, "f16": 2}
Y4_ESTATE, Y4_EINVAL = -1, -22
PATTERN = 0xA5
# (dtype, chain fusion): the runs exist for the 16-bit dtypes only
KERNELS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]


@functools.lru_cache(maxsize=None)
def _flat(hw):
    from yolo4hip import weights as W
    from yolo4hip.plan import build_plan
    return W.flatten(W.synth_weights(build_plan(hw, NCLS), seed=2))


def _engine(hw, dtype, level, chain=False, alias=False, max_batch=4):
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    eng = Engine(NCLS, make_config(hw if hw[0] != hw[1] else hw[0]), max_batch=max_batch, dtype=dtype, device="cuda:0",
                 alias_workspace=alias, retain_head_inputs=level)
    eng.load_weight_blob(_flat(hw))
    if chain:
        assert eng.set_chain_fusion(True) > 0
    return eng


def _images(eng, n, seed):
    import torch
    x = np.random.default_rng(seed).uniform(0, 1, size=(n,) + tuple(eng.img_hw) + (3,)).astype(np.float32)
    return torch.from_numpy(x).to(eng.device)


def _boxes(eng, hw):
    import torch
    return torch.from_numpy(np.ascontiguousarray(LC.make_boxes(hw, NCLS, 4, 9)[[1, 2, 3]])).to(eng.device)


def _row_layout(hw, dtype, level):
    """(row bytes, offsets) from the plan: the three grids times 256 / 512 / 1024 channels at level 1, half that at level 2"""
    sizes = [(hw[0] // s) * (hw[1] // s) * c // level * ES[dtype] for s, c in zip((8, 16, 32), (256, 512, 1024))]
    offs = [0, sizes[0], sizes[0] + sizes[1]]
    assert all(o % 256 == 0 for o in offs) and sum(sizes) % 256 == 0
    return sum(sizes), tuple(offs), sizes


def _taps(eng, n, convs, with_taps):
    """bits of the heads and, on an engine that keeps them, of the named convs' outputs"""
    out = {"heads": [h.cpu().numpy().view(np.int32) for h in eng.heads_device(n)]}
    if with_taps:
        for c in convs:
            out[c] = eng.conv_output(c, n).view(np.int32)
    return out


def _grads(eng, n, boxes, level, dtype):
    import torch
    got = {"loss": eng.loss_device(n, boxes_dev=boxes), "dw": eng.head_grad_device(n, boxes_dev=boxes)}
    if level == 2 and dtype == "f16":
        got["dk"], got["overflow"] = eng.block_grad_device(n, boxes_dev=boxes, loss_scale=1024.0)
    elif level == 2:
        got["dk"] = eng.block_grad_device(n, boxes_dev=boxes)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.int32) for k, v in got.items()}


def _row_as_f32(cache, slot, off, count, dtype):
    import torch
    t = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    return cache[slot, off:off + count * ES[dtype]].view(t).to(torch.float32).cpu().numpy().view(np.int32)


ROUND_TRIP = [(hw, d, ch, lv, False) for hw in SHAPES for d, ch in KERNELS for lv in (1, 2)] + \
             [(hw, "bf16", True, lv, True) for hw in SHAPES for lv in (1, 2)]


# ---- 1. the round trip through the C ABI
@pytest.mark.parametrize("hw,dtype,chain,level,alias", ROUND_TRIP)
def test_store_clobber_load_tail_gives_the_forward_bits(hw, dtype, chain, level, alias):
    """Forward A, store A at permuted slots, forward B over it, load A's rows into OTHER batch positions, run the tail: heads and
    conv outputs are A's, row by row.  Loaded into their own positions: y4_loss, y4_head_grad and, at level 2, y4_block_grad too.
    alias: the aliased workspace `fit` trains on (no conv taps there, the heads and gradients say it all)."""
    import torch
    n = 3
    eng = _engine(hw, dtype, level, chain, alias)
    row, offs, sizes = _row_layout(hw, dtype, level)
    assert eng.feature_row_bytes() == (row, offs)
    convs = CACHED[level] + TAIL[level]
    A, B, boxes = _images(eng, n, 1), _images(eng, n, 2), _boxes(eng, hw)
    eng.forward_device(A)
    want = _taps(eng, n, convs, not alias)
    want_g = _grads(eng, n, boxes, level, dtype)
    cache = eng.alloc_feature_cache(5)
    assert cache.dtype == torch.uint8 and tuple(cache.shape) == (5, row) and cache.device == eng.device
    cache.fill_(PATTERN)
    stored = [4, 0, 2]
    eng.store_features(cache, stored)
    if not alias:                    # a row IS the dense tensors, in the engine's dtype
        for i, slot in enumerate(stored):
            for k, c in enumerate(CACHED[level]):
                got = _row_as_f32(cache, slot, offs[k], sizes[k] // ES[dtype], dtype)
                assert np.array_equal(got, want[c][i].reshape(-1)), (c, i)
    assert bool((cache[[1, 3]] == PATTERN).all())
    eng.forward_device(B)
    other = _taps(eng, n, convs, not alias)
    assert all(not np.array_equal(a, b) for a, b in zip(other["heads"], want["heads"]))
    # image perm[p] goes to batch position p
    perm = [1, 2, 0]
    eng.load_features(cache, [stored[i] for i in perm])
    eng.forward_tail_device(n)
    got = _taps(eng, n, convs, not alias)
    for key in want:
        for a, b in (zip(got[key], want[key]) if key == "heads" else [(got[key], want[key])]):
            for p in range(n):
                assert np.array_equal(a[p], b[perm[p]]), (key, p)
    want_loss = want_g["loss"][perm]
    assert np.array_equal(eng.loss_device(n, boxes_dev=boxes[perm].contiguous()).cpu().numpy().view(np.int32), want_loss)
    # back where they came from: the sums of the gradients run in the forward's order
    eng.forward_device(B)
    eng.load_features(cache, stored)
    eng.forward_tail_device(n)
    got_g = _grads(eng, n, boxes, level, dtype)
    assert set(got_g) == set(want_g) and ("dk" in got_g) == (level == 2)
    for key in want_g:
        assert np.array_equal(got_g[key], want_g[key]), key
    assert np.any(want_g["dw"] != 0) and (level == 1 or np.any(want_g["dk"] != 0))
    if "overflow" in want_g:
        assert not want_g["overflow"].any()
    # decode + NMS run on the tail's heads (and its objectness side array) as on the forward's
    dets = [o.cpu().numpy() for o in eng.decode_nms_device(n)]
    eng.forward_device(A)
    for a, b in zip(dets, [o.cpu().numpy() for o in eng.decode_nms_device(n)]):
        assert np.array_equal(a, b)
    eng.close()


# ---- 2. a copy touches what it names and nothing else
@pytest.mark.parametrize("hw,dtype,level", [((160, 160), "bf16", 1), ((96, 160), "f32", 2), ((96, 160), "f16", 1)])
def test_copies_do_not_leak(hw, dtype, level):
    import torch
    eng = _engine(hw, dtype, level)
    row = eng.feature_row_bytes()[0]
    convs = CACHED[level]
    eng.forward_device(_images(eng, 4, 3))
    # the cache is the middle of a larger allocation: a guard row on either side
    big = torch.full((7, row), PATTERN, dtype=torch.uint8, device=eng.device)
    cache = big[1:6]
    eng.store_features(cache, [3, 1])
    host = big.cpu().numpy()
    for r in (0, 1, 3, 5, 6):                                # guards and the rows not named (cache rows 0, 2, 4)
        assert (host[r] == PATTERN).all(), r
    for r in (2, 4):                                         # the named rows (cache rows 1, 3) are written over their whole length:
        assert (host[r] != PATTERN).any()                    # compared with the tensors below
    before = _taps(eng, 4, convs, True)
    for i, slot in enumerate([3, 1]):
        got = np.concatenate([_row_as_f32(cache, slot, o, s // ES[dtype], dtype) for o, s in zip(*_row_layout(hw, dtype, level)[1:])])
        assert np.array_equal(got, np.concatenate([before[c][i].reshape(-1) for c in convs]))
    # a load of one row writes batch position 0 and leaves positions 1..3 alone
    eng.load_features(cache, [3])
    after = _taps(eng, 4, convs, True)
    for c in convs:
        assert np.array_equal(after[c][0], before[c][0]) and np.array_equal(after[c][1:], before[c][1:])
    eng.load_features(cache, [1])
    after = _taps(eng, 4, convs, True)
    for c in convs:
        assert np.array_equal(after[c][0], before[c][1]) and np.array_equal(after[c][1:], before[c][1:])
    assert np.array_equal(big.cpu().numpy(), host)
    eng.close()


# ---- 3. refusals
def test_refusals_leave_cache_and_workspace_alone():
    import torch
    from yolo4hip import ext
    hw, level = (96, 160), 2
    eng = _engine(hw, "bf16", level)
    eng.forward_device(_images(eng, 4, 5))
    cache = eng.alloc_feature_cache(4)
    cache.fill_(PATTERN)
    before = _taps(eng, 4, CACHED[level], True)
    for fn in (eng.store_features, eng.load_features):
        for slots in ([0, -1], [4, 1], [0, 1, 2, 3, 0]):      # below, at cache_rows, more images than max_batch
            with pytest.raises(ext.Y4Error) as e:
                fn(cache, slots)
            assert e.value.code == Y4_EINVAL, (fn.__name__, slots)
    with pytest.raises(ext.Y4Error) as e:
        eng.store_features(cache, [2, 1, 2])
    assert e.value.code == Y4_EINVAL and "twice" in str(e.value)
    with pytest.raises(ext.Y4Error) as e:
        eng.forward_tail_device(5)
    assert e.value.code == Y4_EINVAL
    with pytest.raises(ValueError):
        eng.store_features(cache[:, :-256], [0])
    torch.cuda.synchronize()
    assert bool((cache == PATTERN).all())
    after = _taps(eng, 4, CACHED[level], True)
    for key in before:
        for a, b in zip(before[key], after[key]):
            assert np.array_equal(a, b)
    eng.load_features(cache, [2, 2])                          # a load may name a row twice
    eng.close()
    plain = _engine(hw, "bf16", 0)
    plain.forward_device(_images(plain, 2, 5))
    for call in (plain.feature_row_bytes, lambda: plain.forward_tail_device(2), lambda: plain.alloc_feature_cache(2)):
        with pytest.raises(ext.Y4Error) as e:
            call()
        assert e.value.code == Y4_ESTATE
    plain.close()


# ---- 4. fit(cache_features=True) is fit()
SIZES = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64), (128, 96), (160, 120)]
FIT_CASES = [("heads", "f32", None), ("heads", "bf16", None), ("head_blocks", "f32", None), ("head_blocks", "bf16", None),
             ("head_blocks", "f16", 1024.0)]


def _facade(hw, dtype):
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    cfg = make_config(hw if hw[0] != hw[1] else hw[0], batch_size=3)
    return Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), cfg, dtype=dtype, max_batch=2, synth_seed=3, tune=False)


def _fit(tmp_path, monkeypatch, hw, dtype, trainable, loss_scale, **kw):
    """One fit of 3 epochs over 7 images in shuffled batches of 3 through max_batch 2 -> (model, history, per epoch the calls of
    Engine.forward_device and prepost.imread_rgb)."""
    from yolo4hip import prepost
    from yolo4hip.data import DataGenerator
    from yolo4hip.engine import Engine
    calls = [{"forward": 0, "imread": 0}]
    real_forward, real_imread = Engine.forward_device, prepost.imread_rgb

    def forward(self, imgs):
        calls[-1]["forward"] += 1
        return real_forward(self, imgs)

    def imread(path):
        calls[-1]["imread"] += 1
        return real_imread(path)

    class NextEpoch:
        def on_epoch_end(self, epoch, logs):
            calls.append({"forward": 0, "imread": 0})
    m = _facade(hw, dtype)
    before = m._flat.copy()
    lines = _write_dataset(tmp_path, SIZES, [3, 0, 5, 8, 1, 4, 2])
    with monkeypatch.context() as mp:
        mp.setattr(Engine, "forward_device", forward)
        mp.setattr(prepost, "imread_rgb", imread)
        np.random.seed(11)
        gen = DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=True, config=m.config)
        extra = {} if loss_scale is None else {"loss_scale": loss_scale}
        hist = m.fit(gen, 3, callbacks=[NextEpoch()], trainable=trainable, learning_rate=1e-3, **extra, **kw)
    return m, before, hist, calls[:3]


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("trainable,dtype,loss_scale", FIT_CASES)
def test_fit_with_cached_features_is_fit(tmp_path, monkeypatch, hw, trainable, dtype, loss_scale):
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    m, before, hist, calls = _fit(tmp_path / "a", monkeypatch, hw, dtype, trainable, loss_scale)
    m2, before2, hist2, calls2 = _fit(tmp_path / "b", monkeypatch, hw, dtype, trainable, loss_scale, cache_features=True)
    print(hw, trainable, dtype, "history", hist.history, "cached", hist2.history, "calls", calls, calls2)
    assert set(hist.history) == set(hist2.history) and len(hist.history["loss"]) == 3
    for key in hist.history:
        assert hist.history[key] == hist2.history[key], key
    assert np.isfinite(hist.history["loss"]).all() and len(set(hist.history["loss"])) == 3
    assert np.array_equal(m._flat.view(np.int32), m2._flat.view(np.int32))
    assert np.any(m._flat != before) and np.array_equal(before, before2)
    # 3 batches of 3, 3, 1 images through max_batch 2: 5 forwards and 7 photos per uncached epoch
    assert calls == [{"forward": 5, "imread": 7}] * 3
    assert calls2 == [{"forward": 5, "imread": 7}, {"forward": 0, "imread": 0}, {"forward": 0, "imread": 0}]


# ---- 5. what the facade refuses
def test_facade_refusals_change_nothing(tmp_path):
    from yolo4hip.augment import AugmentConfig
    from yolo4hip.data import DataGenerator
    hw = (160, 160)
    m = _facade(hw, "bf16")
    before = m._flat.copy()
    lines = _write_dataset(tmp_path, SIZES, [3, 0, 5, 8, 1, 4, 2])
    names = os.path.join(CLASS_DIR, "bccd_classes.txt")
    gen = DataGenerator(lines, names, str(tmp_path), shuffle=False, config=m.config)
    with pytest.raises(ValueError, match="augment"):
        m.fit(DataGenerator(lines, names, str(tmp_path), config=m.config, augment=AugmentConfig(), seed=1), 2, trainable="heads",
              cache_features=True)

    class Bare:
        """a generator of the reference's kind: batches and boxes, nothing else"""
        max_boxes = gen.max_boxes

        def __len__(self):
            return len(gen)

        def boxes(self, i):
            return gen.boxes(i)
    with pytest.raises(ValueError, match="labels"):
        m.fit(Bare(), 2, trainable="heads", cache_features=True)
    for trainable, level in (("heads", 1), ("head_blocks", 2)):
        row = _row_layout(hw, "bf16", level)[0]
        with pytest.raises(MemoryError) as e:
            m.fit(gen, 2, trainable=trainable, cache_features=1)
        assert str(row) in str(e.value) and str(7 * row) in str(e.value)
        with pytest.raises(MemoryError):
            m.fit(gen, 2, trainable=trainable, cache_features=7 * row - 1)
    with pytest.raises(ValueError):
        m.fit(gen, 2, trainable="heads", cache_features="yes")
    assert np.array_equal(m._flat.view(np.int32), before.view(np.int32))
    # and the budget that holds the cache exactly is taken
    hist = m.fit(gen, 2, trainable="heads", cache_features=7 * _row_layout(hw, "bf16", 1)[0])
    assert len(hist.history["loss"]) == 2 and np.any(m._flat != before)
