"""Inputs, float64 references and derived bounds of the value-range tests (tests/test_gpu_value_range.py on the device,
tests/test_value_range_cpu.py without one).

1. The conv epilogue, element by element.  A conv with identity weights (1x1: w[o, i] = delta; 3x3: the delta on the centre tap)
hands every accumulator its input element exactly, so the kernel computes act(fma(x, scale, shift)) (+ residual) on operands the
test chose: `epilogue_case` picks x (multiples of 1/8 in [-16, 16): exact in float32, bfloat16 and float16), and per channel a
scale and a shift, so that z = x * scale + shift visits a dense grid on [-25, 25], log-spaced magnitudes up to 3e4 (float16) or
1e30, and the neighbourhoods -- one float32 spacing apart, and +-1 -- of the places where the activation formulas of
csrc/common.h change behaviour.  BatchNorm rows [beta, gamma, +-0, var1] with var1 + eps == 1 in float32 make
ConvWeights.scale_shift() and the oracle's own fold return scale = gamma and shift = beta exactly.  Every channel with a shift
other than 0 has a scale of at most 12 significant bits, so x * scale is exact in float32 and the oracle's multiply-then-add
rounds once, like the kernel's FMA.

Bound of one element (`epilogue_bound`), z the float64 pre-activation, want the float64 result:
    float32 store   8 * 2^-24 * max(1, |z|, |want|): half a spacing of z from the FMA; about one each from v_exp_f32 and v_rcp_f32
                    (or expf and the division); the rounding of z * log2(e) moves e by |z| 2^-23 relative, which reaches the
                    result only where z^2 e^z <= 0.54; the last FMA x - x r cancels with an absolute error of |z| 2^-24
    residual        + 2^-24 * (|want + res| + the above): one more float32 rounding, of the sum
    16-bit store    + half a spacing of the storage type at want
    float16 store   with |want| beyond 65504: the correctly signed infinity or 65504 (`f16_overflow_ok`), nothing else

2. `WIDE_INPUT_CONVS`: the convs of the backbone at whose inputs tests/helpers.widen_activations must put pre-activations
beyond +-20 (the convs the fused kernels cover: stem, chain, residual blocks, stages).
"""
import numpy as np

EPS24 = 2.0 ** -24
F16_MAX = 65504.0
# (z, what happens there in csrc/common.h)
SPECIAL = [
    (20.0, "float32 Mish returns x above it"), (-20.0, "fast Mish: r rounds to 1"),
    (44.4, "e * e overflows"), (88.8, "e overflows"), (-87.4, "e goes denormal"), (-104.0, "e is zero"),
    (F16_MAX, "the largest float16"), (-F16_MAX, "the largest float16, negative"),
    (65520.0, "float16 rounds to infinity from here"), (-65520.0, "float16 rounds to -infinity from here"),
]
NCH = 64
_VAR1 = np.float32(1.0) - np.float32(1e-3)


def _spacing32(v):
    return float(np.spacing(np.float32(abs(v))))


def channel_table(dtype):
    """-> (scale [64], shift [64], kind [64]) float32 / str: the 64 channel kinds (see the module docstring)."""
    sc, sh, kind = [], [], []

    def add(s, b, k):
        sc.append(s); sh.append(b); kind.append(k)
    for j in range(16):                                      # dense grid on [-25, 25]: 16 interleaved combs of 256 teeth
        add((-1.0) ** j * 25.0 / 16.0, j * 25.0 / 2048.0, "dense25")
    top = 3.0e4 if dtype == "f16" else 1.0e30
    for j, m in enumerate(np.logspace(1.5, np.log10(top), 16)):          # z = x * scale: |z| up to m
        add((-1.0) ** j * (top if j == 15 else float(m)) / 16.0, 0.0, "log")
    for j in range(8):                                       # [-110, 110]: where exp leaves and enters the float32 range
        add((-1.0) ** j * 110.0 / 16.0, (j - 4) * 0.21875, "dense110")
    for z, _ in SPECIAL:
        coarse = 4.0 if abs(z) > 6.0e4 else 2.0 ** -4        # +-1 around the point (+-64 at the float16 limit)
        add(coarse, z, "coarse")
        add(-8.0 * _spacing32(z), z, "fine")                 # 1/8 steps of x = one float32 spacing of z each
    # +-0 and the smallest normals: z = x * scale with scale = 8 * (the smallest normal), shift +0 or -0
    add(8.0 * 2.0 ** -126, 0.0, "tiny"); add(-8.0 * 2.0 ** -126, -0.0, "tiny")
    add(8.0 * 2.0 ** -14, 0.0, "tiny"); add(-8.0 * 2.0 ** -14, -0.0, "tiny")
    assert len(sc) == NCH, len(sc)
    return np.array(sc, np.float32), np.array(sh, np.float32), kind


def epilogue_case(dtype, cout=64, hw=(16, 16), k=1, seed=0):
    """-> dict(x [1, h, w, cout] float32, w [cout, cout, k, k] (identity), bn [4, cout], res [1, h, w, cout]: a residual
    representable in `dtype`, kind [cout]).  Channels 64 .. repeat the table with the scale negated (z mirrored about the shift)."""
    assert cout % NCH == 0 and k in (1, 3)
    s, b, kind = channel_table(dtype)
    reps = cout // NCH
    scale = np.concatenate([s * np.float32((-1.0) ** r) for r in range(reps)])
    shift = np.concatenate([b] * reps)
    h, w_ = hw
    p = np.arange(h * w_)
    rng = np.random.default_rng([seed, 0x5A1])
    x = np.empty((h * w_, cout), np.float32)
    for c in range(cout):                                    # every channel sees all 256 grid values, in its own order
        x[:, c] = ((p * (2 * (c % 8) + 1) + 7 * c) % 256 - 128) / 8.0
    x[0, :] = 0.0                                            # (+0: with a negative scale and shift -0, z = -0)
    wt = np.zeros((cout, cout, k, k), np.float32)
    wt[np.arange(cout), np.arange(cout), k // 2, k // 2] = 1.0
    # shift = beta - mean * scale: a mean of -0 where beta is -0 and the scale negative keeps the shift at -0 (z = -0 at x = 0)
    mean = np.where(np.signbit(shift) & (shift == 0) & (scale < 0), np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    bn = np.stack([shift, scale, mean, np.full(cout, _VAR1, np.float32)]).astype(np.float32)
    res = rng.standard_normal((1, h, w_, cout)) * 3.0
    res = res.astype(np.float32)
    if dtype == "bf16":
        u = res.view(np.uint32).astype(np.uint64)
        res = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    elif dtype == "f16":
        res = res.astype(np.float16).astype(np.float32)
    return dict(x=x.reshape(1, h, w_, cout), w=wt, bn=bn, res=res, kind=kind * reps)


def preact64(x, scale, shift):
    """z in float64 from the float32 operands the kernel gets (channel-last broadcasting)"""
    return np.asarray(x, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)


def act64(z, act):
    z = np.asarray(z, np.float64)
    if act == "mish":
        with np.errstate(over="ignore"):
            e = np.exp(z)
        sp = np.where(np.isinf(e), z, np.log1p(np.where(np.isinf(e), 0.0, e)))
        return z * np.tanh(sp)
    if act == "leaky":
        return np.maximum(z, 0.1 * z)
    return z


def storage_half_spacing(want, store):
    """half the spacing of the storage type at |want| (float64 array); 0 for a float32 store (that rounding is in the 8 * 2^-24)"""
    a = np.abs(np.asarray(want, np.float64))
    if store == "f32":
        return np.zeros_like(a)
    mant, emin = (7, -126) if store == "bf16" else (10, -14)
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - mant)


def epilogue_bound(z, want_act, res, store):
    """The bound of |got - want| per element (module docstring); want = want_act + res"""
    b = 8.0 * EPS24 * np.maximum(1.0, np.maximum(np.abs(z), np.abs(want_act)))
    want = want_act
    if res is not None:
        want = want_act + np.asarray(res, np.float64)
        b = b + EPS24 * (np.abs(want) + b)
    return b + storage_half_spacing(want, store)


def f16_overflow_ok(got, want):
    """float16 store, |want| > 65504: the stored value is the correctly signed infinity or +-65504"""
    pos = np.asarray(want) > 0
    return (got == np.where(pos, np.inf, -np.inf)) | (got == np.where(pos, F16_MAX, -F16_MAX))


def check_epilogue(got, z, want_act, res, store):
    """-> (ok [bool array], c: the measured distance in units of 2^-24 max(1, |z|, |want_act|) over the elements held to the bound,
    after the storage and residual allowances are taken off)"""
    want = want_act if res is None else want_act + np.asarray(res, np.float64)
    got = np.asarray(got, np.float64)
    bound = epilogue_bound(z, want_act, res, store)
    over = (np.abs(want) > F16_MAX) if store == "f16" else np.zeros(want.shape, bool)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
    ok = np.where(over, f16_overflow_ok(got, want), np.isfinite(got) & (err <= bound))
    unit = EPS24 * np.maximum(1.0, np.maximum(np.abs(z), np.abs(want_act)))
    extra = bound - 8.0 * unit
    held = ~over & np.isfinite(got)
    c = float((np.maximum(err - extra, 0.0) / unit)[held].max()) if held.any() else 0.0
    return ok, c


def coverage(z, dtype):
    """Counts of z per region the issue names -> dict; test_value_range_cpu.py asserts each is populated."""
    z = np.asarray(z, np.float64).ravel()
    a = np.abs(z)
    top = 3.0e4 if dtype == "f16" else 1.0e30
    out = {
        "dense_bins_of_0.05_on_[-25,25]_hit": int(np.unique(np.floor(z[a <= 25.0] / 0.05)).size),
        "plus_zero": int(((z == 0) & ~np.signbit(z)).sum()), "minus_zero": int(((z == 0) & np.signbit(z)).sum()),
        "decades": int(np.unique(np.floor(np.log10(a[(a >= 30.0) & (a <= top)]))).size),
        "at_top": int((a >= 0.9 * top).sum()),
        "f32_min_normal": int((a == 2.0 ** -126).sum()), "f16_min_normal": int((a == 2.0 ** -14).sum()),
    }
    for v, _ in SPECIAL:
        name, v = v, float(np.float32(v))
        s = _spacing32(v)
        near = z[np.abs(z - v) <= 130 * s]
        out[f"at_{name}"] = int((near == v).sum())
        out[f"just_below_{name}"] = int(((near < v) & (near >= v - 4 * s)).sum())
        out[f"just_above_{name}"] = int(((near > v) & (near <= v + 4 * s)).sum())
        out[f"within_1_of_{name}"] = int((np.abs(z - v) <= (64.0 if abs(v) > 6e4 else 1.0)).sum())
    return out


# ---- part 2: the convs whose INPUT the wide-range weight set must drive beyond +-20 (conv 1: the stem pair; 2..7: the first stage,
# chain heads and its 64-channel residual block; 11..14: the residual blocks of stage 2; 20..36: the eight blocks of stage 3)
WIDE_INPUT_CONVS = (1,) + tuple(range(2, 8)) + tuple(range(11, 15)) + tuple(range(20, 37))
WIDE_MAX_STORED = 3.0e4
