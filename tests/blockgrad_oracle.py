"""NumPy restatement of the gradient of the 3x3 convs in front of the heads (csrc/block_train.hip).  Per scale, with
g the loss derivative w.r.t. the raw head (tests/lossgrad_oracle.py), Wh [3 (5 + C), cout] the head conv's weights, A the block's
output (the head conv's input), U its input and s = gamma / sqrt(var + eps) the frozen BatchNormalization's scale:

    dA[p, c]        = sum_o g[p, o] Wh[o, c]
    dZ[p, c]        = dA[p, c] * (A[p, c] > 0 ? 1 : 0.1) * s[c]              (TensorFlow's LeakyReLU gradient: 0.1 at exactly 0)
    dK[co,ci,kh,kw] = sum_{n,y,x} dZ[n,y,x,co] U[n, y+kh-1, x+kw-1, ci]      ('same' zero padding)

Everything is evaluated in `dtype` (float64 by default; float32 measures what single precision costs)."""
import numpy as np

BN_EPS = 1e-3          # Keras' BatchNormalization epsilon, the one fold_bn uses (include/yolo4hip.h: y4_pack_weights)


def bn_scale(gamma, var, dtype=np.float64):
    return np.asarray(gamma, dtype=dtype) / np.sqrt(np.asarray(var, dtype=dtype) + dtype(BN_EPS))


def round_bf16(x):
    """Round to the nearest bfloat16 (ties to even), returned as float64."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def block_dz(g, wh, a, s, dtype=np.float64):
    """g [n, gh, gw, nout], wh [nout, cout], a [n, gh, gw, cout], s [cout] -> dZ [n, gh, gw, cout]."""
    g, wh, a, s = (np.asarray(t, dtype=dtype) for t in (g, wh, a, s))
    dA = (g.reshape(-1, g.shape[-1]) @ wh).reshape(a.shape).astype(dtype)
    return (dA * np.where(a > 0, dtype(1.0), dtype(0.1)) * s).astype(dtype)


def block_wgrad(dz, u, dtype=np.float64):
    """dZ [n, gh, gw, cout] and the conv's input u [n, gh, gw, cin] -> dK [cout, cin, 3, 3] summed in `dtype`."""
    dz, u = np.asarray(dz, dtype=dtype), np.asarray(u, dtype=dtype)
    n, gh, gw, cout = dz.shape
    up = np.zeros((n, gh + 2, gw + 2, u.shape[-1]), dtype=dtype)
    up[:, 1:-1, 1:-1] = u
    dk = np.zeros((cout, u.shape[-1], 3, 3), dtype=dtype)
    flat = dz.reshape(-1, cout)
    for kh in range(3):
        for kw in range(3):
            dk[:, :, kh, kw] = flat.T @ up[:, kh:kh + gh, kw:kw + gw].reshape(-1, u.shape[-1])
    return dk


def block_grad(g, wh, a, u, s, dtype=np.float64, round_dz=None):
    """The three formulas in one; `round_dz` (round_bf16) is applied to dZ: the 16-bit MFMA operand."""
    dz = block_dz(g, wh, a, s, dtype)
    if round_dz is not None:
        dz = round_dz(dz).astype(dtype)
    return block_wgrad(dz, u, dtype)
