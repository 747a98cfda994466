"""The layer-local checker (tests/layer_local.py) proved without a GPU: the oracle's storage emulation as stand-in device passes at
every layer, and a stand-in with ONE defect injected at a named layer -- everything downstream computed from the defective tensor, as
a device would -- is flagged at that layer and at no other.

Measured here (bf16, 96 x 96, n = 2 unless said): every required mutant is flagged at its own layer only; of the two that need not be
caught, both are: the single element four spacings off at the deepest 3x3 (conv 108, K = 4608) narrowly, at 1.05 x its bound (the
accumulation allowance there is 6.4 half-spacings, the error eight), the residual added after rounding the branch (conv 5) at a fifth
of the layer's elements, up to 1.4 x the bound (the branch's own half-spacing comes on top of the sum's).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_local as LL
from oracle import forward as OF

NCLS = 3
SHAPES = {"96x96n2": ((96, 96), 2), "96x160n1": ((96, 160), 1)}
_CACHE = {}


def _inputs(shape):
    from yolo4hip import weights as W
    from yolo4hip.plan import build_plan
    if shape not in _CACHE:
        hw, n = SHAPES[shape]
        _CACHE[shape] = (W.synth_weights(build_plan(hw, NCLS), seed=0), W.synth_images(n, hw, seed=0))
    return _CACHE[shape]


def _spacing(v, store):
    return 2.0 * LL.half_spacing(v, store)


def _truncate(y, store):
    """float32 -> the storage type, toward zero"""
    if store == "bf16":
        return (y.contiguous().view(torch.int32) & -65536).view(torch.float32)
    r = y.numpy().astype(np.float16)
    r = np.where(np.abs(r.astype(np.float32)) > np.abs(y.numpy()), np.nextafter(r, np.float16(0)), r)
    return torch.from_numpy(r.astype(np.float32))


class _Mutant(OF._Net):
    """oracle.forward's storage emulation with one defect: mut = {conv index: {'input': fn(x), 'cw': fn(ConvWeights), 'store':
    fn(unrounded y) -> stored, 'post': fn(stored) -> stored}, ('add', i): fn(block input, unrounded branch) -> stored}"""

    def __init__(self, weights, storage, mut, start=0, stored=None):
        # start, stored: the convs below `start` are not computed again but taken from `stored`, the taps of the stand-in without a
        # defect (the same numbers: the defect sits at `start` or behind it)
        super().__init__(weights, torch.float32, collect=range(110), storage=storage)
        self.mut, self.start, self.stored = mut, start, stored

    def _take(self, key):
        self.taps[key] = LL._nchw(self.stored[key])
        return self.taps[key]

    def conv(self, x, filters, kernel_size, downsampling=False, activation="leaky", batch_norm=True):
        idx, m = self.i, self.mut.get(self.i)
        if idx < self.start:
            self.i += 1
            return self._take(idx)
        if not m:
            return super().conv(x, filters, kernel_size, downsampling, activation, batch_norm)
        if "input" in m:
            x = m["input"](x)
        saved, defer = self.weights, self._defer_round
        if "cw" in m:
            self.weights = list(saved)
            self.weights[idx] = m["cw"](saved[idx])
        if "store" in m:
            self._defer_round = True
        y = super().conv(x, filters, kernel_size, downsampling, activation, batch_norm)
        self.weights, self._defer_round = saved, defer
        if "store" in m:
            y = m["store"](y)
        if "post" in m:
            y = m["post"](y)
        self.taps[idx] = y
        return y

    def residual_block(self, x, filters1, filters2, activation="leaky"):
        m = self.mut.get(("add", self.i + 1))
        if self.i + 1 < self.start:
            self.i += 2
            self._take(self.i - 2)
            return self._take(("add", self.i - 1))
        if m is None:
            return super().residual_block(x, filters1, filters2, activation)
        y = self.conv(x, filters1, 1, activation=activation)
        self._defer_round = True
        y = self.conv(y, filters2, 3, activation=activation)
        self._defer_round = False
        out = m(x, y)
        self.taps[("add", self.i - 1)] = out
        return out


_TAPS = {}


def _standin(shape, dtype, mut=None, edit=None, start=0):
    """-> the tensors a (defective) device would have stored; `edit(dev)` changes stored tensors whose reader `mut` keeps consistent"""
    ws, imgs = _inputs(shape)
    storage = None if dtype == "f32" else dtype
    if (shape, dtype) not in _TAPS:
        _TAPS[(shape, dtype)] = OF.yolo_model_forward(imgs, ws, NCLS, storage=storage, collect=range(110))
    heads, taps = _TAPS[(shape, dtype)]
    if mut is not None:
        x = OF._round_storage(torch.from_numpy(imgs), storage).permute(0, 3, 1, 2).contiguous()
        net = _Mutant(ws, storage, mut, start, taps)
        with torch.no_grad():
            heads = [LL._nhwc(h) for h in net.yolov4_neck(x, NCLS)]
        taps = {k: LL._nhwc(v) for k, v in net.taps.items()}
    dev = LL.standin_tensors(heads, taps)
    if edit is not None:
        edit(dev)
    return ws, imgs, dev


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_reference_passes_at_every_layer(dtype, shape):
    ws, imgs, dev = _standin(shape, dtype)
    report, failures = LL.check_forward(imgs, ws, NCLS, dtype, dev)
    LL.record("reference_cpu", f"{dtype}_{shape}", LL.summary(report))
    print(LL.one_line(f"{dtype} {shape}", report))
    assert len(report) == 110 and not failures, "\n".join(failures)
    assert sum(r["key"] == "add" for r in report) == 23 and [r["conv"] for r in report if r["store"] == "f32"] == \
        (list(range(110)) if dtype == "f32" else list(LL.HEADS))
    if dtype != "f32":      # the emulation IS a float32 evaluation rounded once, up to the order of the float32 additions
        assert all(0.8 < r["mean_ratio"] < 1.2 for r in report if r["store"] != "f32")


# ---- mutants
def _swap_halves(x):
    c = x.shape[1] // 2
    return torch.cat([x[:, c:], x[:, :c]], dim=1)


def _zero_chunk(cw):
    w = cw.w.copy()
    w[:, 64:128] = 0.0
    return type(cw)(w=w, bn=cw.bn, bias=cw.bias)


def _flip_kernel(cw):
    return type(cw)(w=np.ascontiguousarray(cw.w[:, :, ::-1, ::-1]), bn=cw.bn, bias=cw.bias)


def _spp_window_7(x):
    c = x.shape[1] // 4
    return torch.cat([x[:, :c], F.max_pool2d(x[:, 3 * c:], 7, 1, 3), x[:, 2 * c:]], dim=1)


def _element_off(store, at=(0, 5, 1, 2)):
    def post(y):
        y = y.clone()
        assert y[at] != 0
        y[at] += 4.0 * float(_spacing(float(y[at]), store))
        return y
    return post


_UP_AT, _UP_C = (0, 3, 5), 9        # stored (2x) row / column of conv 78's tensor, channel


def _mutants(store):
    """name -> (shape, mut, edit of the stored tensors, the layer that must be flagged, required)"""
    rnd = lambda t: OF._round_storage(t, store)

    def unreplicate(dev):
        dev[78] = dev[78].copy()
        n, y, x = _UP_AT
        dev[78][n, y, x, _UP_C] += 4.0 * float(_spacing(float(dev[78][n, y, x, _UP_C]), store))

    def read_unreplicated(x):          # conv 80 reads [conv 79, the stored tensor of conv 78]
        x = x.clone()
        n, r, c = _UP_AT
        v = x[n, 256 + _UP_C, r, c]
        x[n, 256 + _UP_C, r, c] = v + 4.0 * float(_spacing(float(v), store))
        return x

    sq = "96x96n2"
    return {
        "store_truncated_conv40": (sq, {40: {"store": lambda y: _truncate(y, store)}}, None, 40, True),
        "k_chunk_zeroed_conv108": (sq, {108: {"cw": _zero_chunk}}, None, 108, True),
        # bottom / right padding of a stride-2 conv == the top / left one on the mirrored image with the mirrored kernel, mirrored back
        "pad_bottom_right_conv8": (sq, {8: {"input": lambda x: x.flip(2, 3), "cw": _flip_kernel, "post": lambda y: y.flip(2, 3)}}, None, 8, True),
        "concat_swapped_conv7": (sq, {7: {"input": _swap_halves}}, None, 7, True),
        "halves_swapped_conv79": (sq, {79: {"input": _swap_halves}}, None, 79, True),
        "concat_swapped_conv80": (sq, {80: {"input": _swap_halves}}, None, 80, True),
        "add_dropped_conv12": (sq, {("add", 12): lambda x, y: rnd(y)}, None, 12, True),
        "spp_window_7_conv75": ("96x160n1", {75: {"input": _spp_window_7}}, None, 75, True),
        "block_not_replicated_conv78": (sq, {80: {"input": read_unreplicated}}, unreplicate, 78, True),
        "images_exchanged_conv20": (sq, {20: {"post": lambda y: y.flip(0)}}, None, 20, True),
        "element_4_spacings_conv3": (sq, {3: {"post": _element_off(store)}}, None, 3, True),
        "element_4_spacings_conv108": (sq, {108: {"post": _element_off(store)}}, None, 108, False),
        "double_rounding_conv5": (sq, {("add", 5): lambda x, y: rnd(x + rnd(y))}, None, 5, False),
    }


_MUTANT_NAMES = list(_mutants("bf16"))


@pytest.mark.parametrize("name", _MUTANT_NAMES)
def test_mutant_is_flagged_at_its_own_layer_only(name):
    store = "bf16"
    shape, mut, edit, layer, required = _mutants(store)[name]
    # the convs in front of the defect hold the stand-in's own tensors, which test_reference_passes_at_every_layer has checked: neither
    # computed nor checked again
    start = min(k if isinstance(k, int) else k[1] - 1 for k in list(mut) + ([78] if edit else []))
    ws, imgs, dev = _standin(shape, store, mut, edit, start)
    full = _standin(shape, store)[2]
    assert all(np.array_equal(dev[k], full[k]) for k in dev if (k if isinstance(k, int) else k[1]) < start)
    report, failures = LL.check_forward(imgs, ws, NCLS, store, dev, start)
    assert [r["conv"] for r in report] == list(range(start, 110))
    got = LL.flagged(report)
    print(f"{name}: flagged {got}" + "".join("\n   " + f[:260] for f in failures))
    LL.record("reference_cpu", "mutant_" + name, {"flagged": got, "required": required})
    if required:
        assert got == [layer], failures
    else:
        assert got in ([], [layer]), failures


def test_truncated_store_is_flagged_in_float16_too():
    ws, imgs, dev = _standin("96x96n2", "f16", {40: {"store": lambda y: _truncate(y, "f16")}})
    report, failures = LL.check_forward(imgs, ws, NCLS, "f16", dev)
    assert LL.flagged(report) == [40], failures
    assert any("mean |err|" in f for f in failures) and report[40]["mean_ratio"] > 1.7     # a truncating store doubles the mean
