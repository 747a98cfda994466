"""bench.py's --steps / --blocks split and its --dump-outputs writer, on CPU (no engine): the K timed steps are exactly K, and the
dumped arrays are the last step's host block (Engine.alloc_outputs_flat layout) bit for bit, the global batch in rank order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_block_sizes_sum_to_the_timed_steps():
    import bench
    for steps in (1, 2, 3, 7, 20, 101):
        for blocks in (1, 2, 5, 200):
            sizes = bench.block_sizes(steps, blocks)
            assert sum(sizes) == steps and len(sizes) == min(steps, blocks) and max(sizes) - min(sizes) <= 1 and min(sizes) >= 1


def _host_block(boxes, scores, classes, valid, kept):
    return np.concatenate([boxes.ravel().view(np.int32), scores.ravel().view(np.int32), classes.ravel().view(np.int32),
                           valid.astype(np.int32), kept.astype(np.int32).ravel()])


def test_dump_outputs_round_trips_the_host_blocks_of_every_rank(tmp_path):
    import bench
    rng = np.random.default_rng(7)
    T, n = 100, 5
    boxes = rng.standard_normal((n, T, 4)).astype(np.float32)
    scores = rng.random((n, T)).astype(np.float32)
    classes = rng.integers(0, 80, (n, T)).astype(np.float32)
    valid = rng.integers(0, T + 1, n).astype(np.int32)
    kept = rng.integers(0, 22743, (n, T)).astype(np.int32)
    shards = [_host_block(boxes[a:b], scores[a:b], classes[a:b], valid[a:b], kept[a:b]) for a, b in ((0, 3), (3, 5))]
    shapes = bench.dump_outputs(str(tmp_path), shards, T)
    assert shapes == {"boxes": [n, T, 4], "scores": [n, T], "classes": [n, T], "valid": [n], "kept": [n, T]}
    got = {name: np.load(tmp_path / f"{name}.npy") for name in shapes}
    assert all(got[k].dtype in (np.float32, np.float64) for k in got)
    assert sum(a.nbytes for a in got.values()) < 64 << 20
    for name, want in (("boxes", boxes), ("scores", scores), ("classes", classes)):
        assert got[name].dtype == np.float32 and np.array_equal(got[name].view(np.int32), want.view(np.int32)), name
    assert np.array_equal(got["valid"], valid) and np.array_equal(got["kept"], kept)
