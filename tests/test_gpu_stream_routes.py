"""Engine.predict_stream when the frame geometry, the frame count and the input route change between batches and between calls:
every batch is, bit for bit, the batch path (preprocess_u8_batch + predict) on that batch, and an engine whose staging slots were
keyed for another route answers as a fresh engine does."""
import numpy as np
import pytest

from test_gpu_letterbox import _engine, _images, _same_bits

pytestmark = pytest.mark.gpu

HW = (96, 160)
# (frame size, frames): the geometry and the count change between batches; (96, 160) is the network's own size; (90, 200) comes back
SEQUENCE = [((90, 200), 2), ((96, 160), 1), ((90, 200), 2), ((120, 64), 2)]


@pytest.fixture(scope="module")
def eng():
    _, e = _engine(HW, 3, 2, weights=True)
    yield e
    e.close()


@pytest.fixture(scope="module")
def batches():
    return [np.stack(_images([size] * n, seed=20 + i)) for i, (size, n) in enumerate(SEQUENCE)]


@pytest.fixture(scope="module")
def wanted(eng, batches):
    """The batch path on every batch of SEQUENCE, computed once: {letterbox: [five outputs per batch]}."""
    out = {}
    for letterbox in (False, True):
        out[letterbox] = []
        for b in batches:
            u8, bm = eng.preprocess_u8_batch(list(b), letterbox=letterbox, pad_value=100)
            out[letterbox].append(eng.predict(u8, with_indices=True, box_map=bm if letterbox else None))
    return out


@pytest.mark.parametrize("in_flight", [1, 2])
@pytest.mark.parametrize("letterbox", [False, True], ids=["stretch", "letterbox"])
def test_geometry_and_count_change_between_batches(eng, batches, wanted, letterbox, in_flight):
    got = list(eng.predict_stream(batches, with_indices=True, in_flight=in_flight, letterbox=letterbox, pad_value=100))
    assert len(got) == len(batches)
    for b, res, want in zip(batches, got, wanted[letterbox]):
        assert all(len(r) == len(b) for r in res)
        _same_bits(res, want)


def test_slots_rekey_between_calls(eng):
    """Successive calls on one engine switch among stretch, letterbox, nv12 and i420 at one frame size, so that every staging slot is
    keyed again and again; each call answers as an engine that never ran anything else."""
    from yolo4hip import yuv
    fh, fw = 90, 200
    rgb = _images([(fh, fw)] * 5, seed=31)
    rgb_batches = [np.stack(rgb[0:2]), np.stack(rgb[2:4]), np.stack(rgb[4:5])]

    def raw(fmt):
        frames = [yuv.from_rgb(a, fmt).data.reshape(fh + fh // 2, fw) for a in rgb]
        return [np.stack(frames[0:2]), np.stack(frames[2:4]), np.stack(frames[4:5])]

    calls = {
        "stretch": (rgb_batches, dict()),
        "letterbox": (rgb_batches, dict(letterbox=True, pad_value=100)),
        "nv12": (raw("nv12"), dict(yuv="nv12", letterbox=True, pad_value=100, matrix="bt709")),
        "i420": (raw("i420"), dict(yuv="i420", full_range=True)),
    }
    fresh = {}
    for name, (bs, kw) in calls.items():
        _, e = _engine(HW, 3, 2, weights=True)
        fresh[name] = list(e.predict_stream(bs, with_indices=True, in_flight=1, **kw))
        e.close()
    for name in ("stretch", "letterbox", "nv12", "i420", "letterbox", "i420", "nv12", "stretch"):
        bs, kw = calls[name]
        got = list(eng.predict_stream(bs, with_indices=True, in_flight=1, **kw))
        assert len(got) == len(bs)
        for res, want in zip(got, fresh[name]):
            _same_bits(res, want)
