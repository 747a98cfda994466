"""Layer-local check of a whole forward (host only): every conv in float64 ON THE TENSORS THE DEVICE ITSELF STORED for its inputs.

The end-to-end comparisons of a 16-bit forward carry 110 layers of rounding noise, against which one wrong border tap, a truncating
store or a dropped K chunk is small.  Teacher forcing removes the depth: `check_forward` walks the oracle's own wiring
(oracle.forward._Net.yolov4_neck) in float64, but every tensor the HIP path stores is taken from a dictionary of "device" tensors
(NHWC float32 arrays):  conv i under key i;  the 3x3 conv of a residual block as conv + Add under ("add", i), the keys
`yolo_model_forward(collect=...)` uses;  convs 78 / 85 as the 2x-upsampled tensor they store.  The stem's input is the image rounded
to the storage type, weights are rounded to the storage type.  At each such tensor, from the forced inputs:

    acc   = the float64 convolution                 S_abs = conv(|x|, |w|)               K = k k cin
    z     = acc * scale + shift                     (scale, shift = ConvWeights.scale_shift(): the float32 numbers)
    want  = act64(z) (+ res, the forced block input of a residual block)

and the device tensor must satisfy, element by element (u = 2^-24),

    |got - want| <= E(z, act64(z), res) + L (|scale| 2 K u S_abs + F) + H

  E   value_range_cases.epilogue_bound with a float32 store: the FMA, the activation's exp / rcp, the rounding of the residual sum
      (derived there; held on the device by tests/test_gpu_value_range.py)
  K u S_abs bounds K float32 additions of exact products IN ANY ORDER (|fl(sum) - sum| <= (K - 1) u sum |terms|, and one more u for
      the float32 path's rounded products), so it covers split-K, every MFMA shape and every tile's K order.  It is DOUBLED because
      nobody here has measured whether the MFMA's internal additions round to nearest or truncate (truncation: 2 u per addition).
  L   the activation's largest slope, which carries an error of z into the result: 1 for linear and LeakyReLU, 1.09 for Mish
      (sup |mish'| = 1.0884, at z = 1.49)
  F   what the device's BatchNorm fold (fold_bn_kernel: s = gamma * (1 / sqrtf(var + 1e-3f)), h = beta - mean * s; built without FMA
      contraction) may differ from scale_shift() (scale = gamma / sqrt(var + 1e-3f), shift = beta - mean * scale), both float32:
      var + eps and the correctly rounded square root are the same number r on both sides; gamma / r rounds once, gamma * fl(1 / r)
      twice, so |s - scale| <= 3 u |scale|; mean * s differs from mean * scale by that and by one rounding on each side,
      (3 + 2) u |mean scale|; the subtraction rounds once on each side, 2 u |shift|:
          F = u (3 |acc scale| + 5 |mean scale| + 2 |shift|)        (0 for the three bias convs: scale = 1 and the bias are exact)
  H   half a spacing of the storage type (0 for a float32 store: convs 93 / 101 / 109 and every tensor of an f32 handle), taken at
      |want| + (the terms above): the device rounds ITS value, which may lie in the next binade -- the same as
      epilogue_bound(z, act64(z), res, store) + L (...) everywhere but within those terms of a power of two.
  float16, |want| > 65504: value_range_cases.f16_overflow_ok, as check_epilogue does.
Nothing in the bound is fitted to a measurement.

Second assertion, 16-bit stores only: the layer's mean |got - want| is at most 1.25 x the same mean of the REFERENCE -- that layer
evaluated by torch in float32 on the same forced inputs and rounded once, to nearest even, into the storage type (1.25: the factor of
test_16bit_error_is_the_storage_floor).  A truncating store doubles that mean.  For float32 stores the ratio is recorded only.

A 16-bit stored tensor must be exactly representable in its type; every 2 x 2 block of convs 78 / 85 must hold four equal values.
SPP, concat and upsampling are exact operations on forced inputs: they are checked through the conv that reads them (75, 80, 87, 95,
103).  The walk continues from the DEVICE tensor, so a failure names its own layer and no other.
"""
import numpy as np
import torch
import torch.nn.functional as F

import value_range_cases as V
from oracle import forward as OF

U = V.EPS24
MISH_SLOPE = 1.09
MEAN_FACTOR = 1.25
HEADS = (93, 101, 109)
UPSAMPLED = (78, 85)


def quantize(a, store):
    """float32 array -> the nearest (even) number of the storage type, as float32 (helpers.quantize, by torch: the weights are many)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if store == "f32" else OF._round_storage(torch.from_numpy(a), store).numpy()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()


def half_spacing(v, store):
    """half a spacing of the storage type at |v| (float32 for 'f32')"""
    if store != "f32":
        return V.storage_half_spacing(v, store)
    return 0.5 * np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


class _Forced(OF._Net):
    def __init__(self, weights, dev, dtype, start=0):
        super().__init__(weights, torch.float64)
        self.dev, self.store, self.start = dev, dtype, start
        self.report, self.failures = [], []
        self._res = None        # the forced input of the residual block whose 3x3 conv comes next
        self._up = None         # (low-res, stored 2x) of conv 78 / 85 until the conv over the concat has read it

    def _fail(self, row, msg):
        row["ok"] = False
        self.failures.append(f"conv {row['conv']} (k{row['k']} s{row['stride']} {row['cin']}->{row['cout']}, map {row['map'][0]}x{row['map'][1]}, "
                             f"{row['store']} store): {msg}")

    def _stored_input(self, x):
        """the conv over [route, upsampled] reads the tensor conv 78 / 85 STORED, whatever its 2 x 2 blocks hold"""
        lo, full = self._up
        c = full.shape[1]
        if x.shape[1] > c and x.shape[2:] == full.shape[2:] and torch.equal(x[:, -c:], F.interpolate(lo, scale_factor=2, mode="nearest")):
            x = torch.cat([x[:, :-c], full], dim=1)
            self._up = None
        return x

    def conv(self, x, filters, kernel_size, downsampling=False, activation="leaky", batch_norm=True):
        idx, cw = self.i, self.weights[self.i]
        self.i += 1
        if self._up is not None:
            x = self._stored_input(x)
        k, cin = kernel_size, x.shape[1]
        res_t, self._res = self._res, None
        if idx < self.start:                # taken as stored, unchecked (check_forward)
            got = np.asarray(self.dev[("add", idx) if res_t is not None else idx], dtype=np.float64)
            out = _nchw(got[:, ::2, ::2] if idx in UPSAMPLED else got)
            if idx in UPSAMPLED:
                self._up = (out, _nchw(got))
            return out
        store = self.store if batch_norm else "f32"
        w = torch.from_numpy(quantize(cw.w, self.store)).to(torch.float64)
        assert w.shape[0] == filters and w.shape[1] == cin and w.shape[2] == k, (idx, w.shape, filters, cin, k)

        def cv(a, b):
            if downsampling:
                return F.conv2d(F.pad(a, (1, 0, 1, 0)), b, None, stride=2, padding=0)
            return F.conv2d(a, b, None, stride=1, padding=k // 2)
        acc, s_abs = _nhwc(cv(x, w)), _nhwc(cv(x.abs(), w.abs()))
        scale, shift = (v.astype(np.float64) for v in cw.scale_shift())
        z = acc * scale + shift
        a = V.act64(z, activation)
        res = None if res_t is None else _nhwc(res_t)
        want = a if res is None else a + res
        fold = U * (3.0 * np.abs(acc * scale) + 5.0 * np.abs(cw.bn[2].astype(np.float64) * scale) + 2.0 * np.abs(shift)) if batch_norm else 0.0
        slope = MISH_SLOPE if activation == "mish" else 1.0
        accum = slope * (np.abs(scale) * 2.0 * (k * k * cin) * U * s_abs + fold)
        before_store = V.epilogue_bound(z, a, res, "f32") + accum
        bound = before_store + V.storage_half_spacing(np.abs(want) + before_store, store)

        key = ("add", idx) if res is not None else idx
        row = dict(conv=idx, key="add" if res is not None else "conv", k=k, stride=2 if downsampling else 1, cin=cin, cout=filters,
                   map=list(want.shape[1:3]), store=store, act=activation or "linear", ok=True)
        self.report.append(row)
        got32 = np.ascontiguousarray(self.dev[key], dtype=np.float32)
        full = None
        if idx in UPSAMPLED:
            assert got32.shape == (want.shape[0], 2 * want.shape[1], 2 * want.shape[2], filters), (idx, got32.shape, want.shape)
            full, got32 = got32, np.ascontiguousarray(got32[:, ::2, ::2])
            blocks = full.reshape(want.shape[0], want.shape[1], 2, want.shape[2], 2, filters)
            same = (blocks == got32[:, :, None, :, None, :]).all(axis=(2, 4))
            if not same.all():
                n_, y_, x_, c_ = (int(v) for v in np.argwhere(~same)[0])
                self._fail(row, f"the 2x2 block of stored element [{n_}, {2 * y_}:{2 * y_ + 2}, {2 * x_}:{2 * x_ + 2}, {c_}] holds "
                                f"{blocks[n_, y_, :, x_, :, c_].ravel().tolist()}, not four equal values ({int((~same).sum())} such blocks)")
        assert got32.shape == want.shape, (idx, got32.shape, want.shape)
        if store != "f32":
            same = quantize(got32, store) == got32
            if not same.all():
                bad = np.argwhere(~same)[0]
                self._fail(row, f"element {bad.tolist()} = {got32[tuple(bad)]!r} is not a {store} number")
        got = got32.astype(np.float64)
        over = (np.abs(want) > V.F16_MAX) if store == "f16" else np.zeros(want.shape, bool)
        with np.errstate(invalid="ignore"):
            err = np.abs(got - want)
            ok = np.isfinite(got) & (err <= bound)
            if over.any():
                ok = np.where(over, V.f16_overflow_ok(got, want), ok)
        held = ~over & np.isfinite(got)
        ratio = np.where(held, err / bound, 0.0)
        worst_of = ratio if ok.all() else np.where(ok, -1.0, np.where(held, ratio, np.inf))      # the worst failing element, if any
        at = np.unravel_index(int(np.argmax(worst_of)), ratio.shape)
        hs = half_spacing(want, store)
        allow = np.quantile(accum / hs, (0.5, 0.99))
        row.update(worst_ratio=float(ratio[at]) if held[at] else float("inf"), worst_index=[int(v) for v in at],
                   allow_median_hs=float(allow[0]), allow_q99_hs=float(allow[1]), mean_err_hs=float((err / hs)[held].mean()))
        if not ok.all():
            self._fail(row, f"{int((~ok).sum())} of {ok.size} elements beyond the bound, worst element {list(map(int, at))}: got {got[at]!r}, "
                            f"want {want[at]!r}, |err| {err[at]:.4e} > bound {bound[at]:.4e} (ratio {err[at] / bound[at]:.3f}; accumulation "
                            f"allowance {accum[at] / hs[at]:.2f} half-spacings)")
        # the reference: this layer by torch in float32 on the same inputs, rounded once into the storage type
        ref_net = OF._Net([cw], torch.float32, storage=None if self.store == "f32" else self.store)
        ref_net._defer_round = res is not None
        with torch.no_grad():
            y = ref_net.conv(x.to(torch.float32), filters, k, downsampling=downsampling, activation=activation, batch_norm=batch_norm)
            if res is not None:
                y = OF._round_storage(res_t.to(torch.float32) + y, ref_net.storage)
        ref_err = np.abs(_nhwc(y).astype(np.float64) - want)
        mean_dev, mean_ref = float(err[held].mean()), float(ref_err[held].mean())
        row.update(mean_err=mean_dev, mean_err_reference=mean_ref, mean_ratio=mean_dev / mean_ref if mean_ref > 0 else float(mean_dev > 0))
        if store != "f32" and not mean_dev <= MEAN_FACTOR * mean_ref:
            self._fail(row, f"mean |err| {mean_dev:.4e} is {mean_dev / mean_ref:.3f} x the float32-then-rounded reference's {mean_ref:.4e} "
                            f"(allowed {MEAN_FACTOR}); worst element {list(map(int, at))}: got {got[at]!r}, want {want[at]!r}")
        out = _nchw(got)
        if full is not None:
            self._up = (out, _nchw(full.astype(np.float64)))
        return out

    def residual_block(self, x, filters1, filters2, activation="leaky"):
        y = self.conv(x, filters1, 1, activation=activation)
        self._res = x
        return self.conv(y, filters2, 3, activation=activation)        # stored as conv + Add: checked and forced as one tensor


def check_forward(imgs, weights, num_classes, dtype, dev, start=0):
    """imgs NHWC float32, `dev` the device's stored tensors (module docstring), dtype 'f32' | 'bf16' | 'f16' of the handle
    -> (report: one dict per layer, failures: one message per failed assertion, each naming its conv).  start > 0: convs below it are
    taken as stored without a check and have no row -- for tensors that a full pass has already held (tests/test_layer_local_cpu.py)."""
    x = _nchw(quantize(imgs, dtype).astype(np.float64))
    net = _Forced(weights, dev, dtype, start)
    with torch.no_grad():
        net.yolov4_neck(x, num_classes)
    assert net.i == len(weights) == 110, net.i
    return net.report, net.failures


def flagged(report):
    return sorted(r["conv"] for r in report if not r["ok"])


COLUMNS = ("conv", "store", "worst_ratio", "mean_ratio", "mean_err_hs", "allow_median_hs", "allow_q99_hs")


def summary(report):
    """the figures a profile keeps per layer, one row of COLUMNS each: worst |err| / bound, mean |err| over the reference's, mean |err|
    and the accumulation allowance (median, 99 % quantile: near want = 0 the
    half-spacing vanishes and the largest says nothing) in half-spacings of the store"""
    return [[(float(f"{r[k]:.4g}") if isinstance(r[k], float) else r[k]) for k in COLUMNS] for r in report]


def one_line(tag, report):
    worst = max(report, key=lambda r: r["worst_ratio"])
    r16 = [r for r in report if r["store"] != "f32"] or report
    return (f"{tag}: worst |err| / bound {worst['worst_ratio']:.3f} at conv {worst['conv']}; mean |err| over the reference's "
            f"{min(r['mean_ratio'] for r in report):.3f}-{max(r['mean_ratio'] for r in report):.3f}; mean |err| {min(r['mean_err_hs'] for r in r16):.3f}-"
            f"{max(r['mean_err_hs'] for r in r16):.3f} half-spacings; accumulation allowance: median of the layers' medians "
            f"{np.median([r['allow_median_hs'] for r in r16]):.2f}, largest 99 % quantile {max(r['allow_q99_hs'] for r in r16):.1f} (conv "
            f"{max(r16, key=lambda r: r['allow_q99_hs'])['conv']}) half-spacings")


def record(name, case, payload):
    """keep `payload` under `case` in $YOLO4HIP_MEASURED_DIR/layer_local/<name>.json; nothing is written where that variable is not
    set (the copies under profiles/layer_local are committed)"""
    import json
    import os
    out = os.environ.get("YOLO4HIP_MEASURED_DIR")
    if not out:
        return
    try:
        path = os.path.join(out, "layer_local", name + ".json")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = {}
        if os.path.exists(path):
            with open(path) as f:
                data = json.load(f)
        data["columns"] = list(COLUMNS)
        data[case] = payload
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(data.items())) + "\n}\n")
    except (OSError, ValueError):
        pass


def standin_tensors(heads, taps):
    """What `yolo_model_forward(..., storage=, collect=range(110))` returned -> the dictionary a device would have stored"""
    dev = {}
    for key, t in taps.items():
        if isinstance(key, tuple):
            dev[key] = t
        elif ("add", key) not in taps:
            dev[key] = t.repeat(2, axis=1).repeat(2, axis=2) if key in UPSAMPLED else t
    for i, h in zip(HEADS, heads):
        assert np.array_equal(dev[i], h)
    return dev


def residual_convs(plan):
    """the 3x3 convs whose stored tensor is conv + Add"""
    return {int(op.srcs[1][1:]) for op in plan.ops if op.kind == "add"}


def device_tensors(eng, n, plan):
    """After one forward of an unfused, non-aliased engine: all 110 `conv_output`s (the three heads from `heads_device`)"""
    adds = residual_convs(plan)
    dev = {(("add", i) if i in adds else i): eng.conv_output(i, n) for i in range(110) if i not in HEADS}
    for i, h in zip(HEADS, eng.heads_device(n)):
        dev[i] = h.cpu().numpy()
    return dev


# ---- forced schedules (GPU tests): one tile family on every layer that accepts it
def tiles_of(lib, codes):
    """the base tile ids whose schedule code (y4_conv_tile_desc(...)[5]: csrc/conv_tiles.h) is in `codes`"""
    from yolo4hip import schedule
    return [t for t in range(1, lib.y4_conv_tile_count() + 1) if schedule.family(lib, t) in codes]


def force_family(eng, imgs_dev, candidates):
    """Put a tile id of `candidates` on every conv that accepts one (conv i tries them from the i-th on, so the family's members
    spread over the layers); a refusal is Y4_EINVAL from the next forward, raised by the launcher before anything runs.  The second
    conv of a CSP pair that runs as one GEMM has no entry of its own (y4_get_tiles shows its partner's): it counts with its partner.
    -> the 110 entries now set (0: the built-in choice stays)."""
    from yolo4hip import ext
    tiles = [0] * 110
    for i in range(1, 110):
        for j in range(len(candidates)):
            tiles[i] = candidates[(i + j) % len(candidates)]
            eng.set_tiles(tiles)
            if eng.get_tiles()[i] != tiles[i]:
                tiles[i] = 0
                break
            try:
                eng.forward_device(imgs_dev)
                break
            except ext.Y4Error as e:
                assert e.code == -22, (i, tiles[i], e)
                tiles[i] = 0
    eng.set_tiles(tiles)
    return tiles
