"""DataGenerator.labels(i): the boxes of `boxes(i)` without its photos, and with its draws from the global np.random --
what keeps `Yolov4.fit(cache_features=True)` aligned with the uncached call (tests/test_gpu_feature_cache.py)."""
import os

import numpy as np
import pytest

from helpers import CLASS_DIR
from test_loss_cpu import _write_dataset

SIZES = [(120, 200), (160, 160), (90, 64), (200, 150), (64, 64), (128, 96), (160, 120)]
BOXES = [3, 0, 5, 8, 1, 4, 2]


def _generator(tmp_path, lines, **kw):
    from yolo4hip.config import make_config
    from yolo4hip.data import DataGenerator
    return DataGenerator(lines, os.path.join(CLASS_DIR, "bccd_classes.txt"), str(tmp_path), shuffle=True,
                         config=make_config((96, 160), batch_size=3), **kw)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture
def imread_count(monkeypatch):
    from yolo4hip import prepost
    calls, real = [], prepost.imread_rgb

    def counting(path):
        calls.append(path)
        return real(path)
    monkeypatch.setattr(prepost, "imread_rgb", counting)
    return calls


def test_labels_are_the_boxes_of_boxes_with_the_same_draws(tmp_path, imread_count):
    """Two generators seeded alike, 7 images in shuffled batches of 3, three epochs: A reads every batch through `boxes`, B reads
    the first epoch through `boxes` and every later one through `labels`.  Every batch's boxes are equal with ==, the state of
    np.random is equal after every call, and `labels` reads no photo."""
    lines = _write_dataset(tmp_path, SIZES, BOXES)
    np.random.seed(7)
    a = _generator(tmp_path, lines)
    state_a = np.random.get_state()
    np.random.seed(7)
    b = _generator(tmp_path, lines)
    state_b = np.random.get_state()
    assert len(a) == 3 and np.array_equal(a.indexes, b.indexes) and _same_state(state_a, state_b)
    for epoch in range(3):
        for i in range(len(a)):
            np.random.set_state(state_a)
            want = a.boxes(i)[1]
            state_a = np.random.get_state()
            np.random.set_state(state_b)
            reads = len(imread_count)
            got = b.boxes(i)[1] if epoch == 0 else b.labels(i)
            state_b = np.random.get_state()
            assert epoch == 0 or len(imread_count) == reads, "labels decoded a photo"
            assert got.dtype == np.float32 and got.shape == want.shape == (len(a.indexes[3 * i:3 * i + 3]), 100, 5)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (epoch, i)
            assert _same_state(state_a, state_b), (epoch, i)
        np.random.set_state(state_a)
        a.on_epoch_end()
        state_a = np.random.get_state()
        np.random.set_state(state_b)
        b.on_epoch_end()
        state_b = np.random.get_state()
        assert np.array_equal(a.indexes, b.indexes) and _same_state(state_a, state_b)
    assert sorted(a.indexes.tolist()) == list(range(7)) and not np.array_equal(a.indexes, np.arange(7))


def test_labels_before_any_read_take_the_size_from_the_header(tmp_path, imread_count):
    """A generator that never read a line asks the image header: the same boxes, the same draws, no photo decoded."""
    lines = _write_dataset(tmp_path, SIZES, BOXES)
    np.random.seed(5)
    a = _generator(tmp_path, lines)
    want = [a.boxes(i)[1] for i in range(len(a))]
    state_a = np.random.get_state()
    reads = len(imread_count)
    np.random.seed(5)
    b = _generator(tmp_path, lines)
    got = [b.labels(i) for i in range(len(b))]
    assert len(imread_count) == reads
    assert _same_state(state_a, np.random.get_state())
    for g, w in zip(got, want):
        assert np.array_equal(g.view(np.int32), w.view(np.int32))


def test_image_hw_reads_the_header(tmp_path):
    from yolo4hip import prepost
    _write_dataset(tmp_path, SIZES[:3], BOXES[:3])
    for i, hw in enumerate(SIZES[:3]):
        assert prepost.image_hw(str(tmp_path / f"im{i}.png")) == hw


def test_labels_on_an_augmenting_generator_raise(tmp_path):
    from yolo4hip.augment import AugmentConfig
    lines = _write_dataset(tmp_path, SIZES, BOXES)
    for cfg in (AugmentConfig(), AugmentConfig.identity()):
        gen = _generator(tmp_path, lines, augment=cfg, seed=1)
        with pytest.raises(ValueError, match="augment"):
            gen.labels(0)
