"""NumPy restatement of the gradient of the 3x3 convs in front of the heads (csrc/block_train.hip).  Per scale, with
g the loss derivative w.r.t. the raw head (tests/lossgrad_oracle.py), Wh [3 (5 + C), cout] the head conv's weights, A the block's
output (the head conv's input), U its input and s = gamma / sqrt(var + eps) the frozen BatchNormalization's scale:

    dA[p, c]        = sum_o g[p, o] Wh[o, c]
    dZ[p, c]        = dA[p, c] * (A[p, c] > 0 ? 1 : 0.1) * s[c]              (TensorFlow's LeakyReLU gradient: 0.1 at exactly 0)
    dK[co,ci,kh,kw] = sum_{n,y,x} dZ[n,y,x,co] U[n, y+kh-1, x+kw-1, ci]      ('same' zero padding)

Everything is evaluated in `dtype` (float64 by default; float32 measures what single precision costs).

`wgrad_geometry` restates how the weight gradient cuts its K axis and sizes its LDS tile ("Weight gradient" and
"Width limit"), `scratch_bytes` the scratch layout that follows from it, and `wgrad_branches` names the paths of the kernel a
geometry takes: the tests say with them which path a shape reaches."""
import numpy as np

BN_EPS = 1e-3          # Keras' BatchNormalization epsilon, the one fold_bn uses (include/yolo4hip.h: y4_pack_weights)
WG_TILE = 64           # a wgrad workgroup owns 64 output x 64 input channels
WG_TARGET = 512        # workgroups a wgrad launch aims at
LDS_DEFAULT = 64 * 1024    # dynamic LDS a launch gets without opting in: a four-row tile above it falls back to two rows
LDS_LIMIT = 160 * 1024     # the compute unit's LDS: a two-row tile above it is refused


def wgrad_geometry(dtype, n, H, W, cin, cout):
    """The weight gradient of one layer for n images of H x W cells, dtype 'f32' or 'bf16' -> dict(R rows of a K slice, Wp padded
    row of dZ, upitch row pitch of U, uchan / dchan channel pitches (elements), strips per image, slices, splits, lds_bytes), or
    None where two rows with their halo do not fit the LDS."""
    es = 4 if dtype == "f32" else 2
    for R in ((2,) if W >= 64 else (4, 2)):
        if dtype == "f32":
            Wp, upitch = W, W + 2                                        # column -1 .. W
            uchan, dchan = ((R + 2) * upitch) | 1, (R * Wp) | 1          # odd dword pitch
        else:
            Wp = -(-W // 8) * 8                                          # whole k-steps of 8 columns
            upitch = Wp + 8                                              # the shifted taps read one dword past the k-step
            uchan, dchan = (R + 2) * upitch, R * Wp
            uchan += 8 * ((uchan // 8) % 2 == 0)                         # an odd number of 16-byte units
            dchan += 8 * ((dchan // 8) % 2 == 0)
        lds = WG_TILE * (uchan + dchan) * es
        if lds <= LDS_DEFAULT:
            break
    if lds > LDS_LIMIT:
        return None
    strips = -(-H // R)
    slices = n * strips
    tiles = (cin // WG_TILE) * (cout // WG_TILE)
    splits = max(1, min(-(-WG_TARGET // tiles), slices))
    return dict(R=R, Wp=Wp, upitch=upitch, uchan=uchan, dchan=dchan, strips=strips, slices=slices, splits=splits, lds_bytes=lds)


def scratch_bytes(dtype, n, grids, channels):
    """What y4_block_grad_scratch_bytes answers: the three dZ planes [n, gh, gw, cout] in the handle's dtype, then the three
    float32 partial buffers [splits, 9, cout, cin], each aligned to 256 bytes.  grids: [(gh, gw)] x 3, channels: [(cin, cout)]
    x 3.  None where a scale's geometry is unsupported."""
    def align(x):
        return (x + 255) & ~255
    es = 4 if dtype == "f32" else 2
    total = sum(align(n * gh * gw * cout * es) for (gh, gw), (_, cout) in zip(grids, channels))
    for (gh, gw), (cin, cout) in zip(grids, channels):
        g = wgrad_geometry(dtype, n, gh, gw, cin, cout)
        if g is None:
            return None
        total += align(g["splits"] * 9 * cout * cin * 4)
    return total


def wgrad_branches(dtype, H, W, g):
    """The paths of block_wgrad_kernel and its geometry that a layer with geometry g (wgrad_geometry) takes, as a set of names."""
    out = {"R2_wide_start" if W >= 64 else ("R2_fall_back" if g["R"] == 2 else "R4")}
    if g["lds_bytes"] > LDS_DEFAULT:
        out.add("lds_above_64k")                                         # the launch has to raise the kernel's LDS limit
    if g["Wp"] > W:
        out.add("Wp_above_W")                                            # 16-bit: columns W .. Wp - 1 are staged as zeros
    if dtype != "f32" and W % 2:
        out.add("odd_W_pair")                                            # 16-bit: the last column's pair partner is outside
    if H % g["R"]:
        out.add(f"R{g['R']}_last_strip_partial")                         # rows of the last strip outside the image
    if g["splits"] < g["slices"] and g["slices"] % g["splits"]:
        out.add("uneven_split")                                          # slice ranges of unequal length
    ranges = [(s * g["slices"] // g["splits"], (s + 1) * g["slices"] // g["splits"]) for s in range(g["splits"])]
    if any(a // g["strips"] != (b - 1) // g["strips"] for a, b in ranges):
        out.add("range_crosses_image")
    return out


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
