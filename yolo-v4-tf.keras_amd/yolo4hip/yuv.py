"""8-bit YUV 4:2:0 video frames (NV12, NV21, I420, YV12): the frame descriptor, the colour rule of `y4_yuv_u8_ragged`
restated in NumPy, and an RGB -> YUV encoder for tests and users.

  YuvFrame   one frame: a contiguous uint8 buffer, its size, its format and its two row pitches
  to_rgb     the device's integer colour rule (include/yolo4hip.h) on the host: uint8 [h,w,3] at source resolution.
             `y4_yuv_u8_ragged` writes the bytes `y4_resize_u8_ragged` writes for this image
  from_rgb   float64 forward matrix, round half up, clamp; chroma is the rounded mean of each 2 x 2 block

The rule: source pixel (y, x) takes chroma sample (y >> 1, x >> 1) (replication: no siting, no interpolation);
C = Y - y0, D = U - 128, E = V - 128; R = clamp8((cy C + crv E + 8192) >> 14), G = clamp8((cy C + cgu D + cgv E + 8192) >> 14),
B = clamp8((cy C + cbu D + 8192) >> 14) in int32 with an arithmetic shift.  Every coefficient is floor(c 2^14 + 0.5) of the real
coefficient from (Kr, Kb); limited range scales luma by 255/219 and chroma by 255/224.
"""
import numpy as np

FORMATS = ("nv12", "nv21", "i420", "yv12")
# (Kr, Kb) of the two matrices
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
# (matrix, full_range) -> (y0, cy, crv, cgu, cgv, cbu): the table of include/yolo4hip.h and csrc/yuv_u8.hip
COEFFS = {
    ("bt601", False): (16, 19077, 26149, -6419, -13320, 33050),
    ("bt601", True): (0, 16384, 22970, -5638, -11700, 29032),
    ("bt709", False): (16, 19077, 29372, -3494, -8731, 34610),
    ("bt709", True): (0, 16384, 25802, -3069, -7670, 30402),
}
FLAG_BT709, FLAG_FULL_RANGE = 1, 2


def flags(matrix="bt601", full_range=False):
    """The matrix / range word of a y4_yuv_desc: bit 0 selects BT.709, bit 1 full range.  ValueError for an unknown matrix."""
    if matrix not in KR_KB:
        raise ValueError(f"matrix must be one of {sorted(KR_KB)}, got {matrix!r}")
    return (FLAG_BT709 if matrix == "bt709" else 0) | (FLAG_FULL_RANGE if full_range else 0)


def _check_fmt(fmt):
    if fmt not in FORMATS:
        raise ValueError(f"fmt must be one of {FORMATS}, got {fmt!r}")
    return fmt


def chroma_size(h, w):
    """Rows and samples per row of a chroma plane: ceil(h / 2), ceil(w / 2)."""
    return (h + 1) // 2, (w + 1) // 2


class YuvFrame:
    """One 8-bit 4:2:0 frame.  `data` is one contiguous uint8 buffer (any shape; a read-only one is fine) that starts with the
    luma plane, h rows of `y_pitch` bytes, followed by the chroma: one interleaved plane of ceil(h/2) rows of `c_pitch` bytes
    (nv12: U V U V ..., nv21: V U V U ...) or two planes of ceil(h/2) rows of `c_pitch` bytes each (i420: U then V, yv12: V then
    U).  The default pitches are the tight ones: w, and 2 ceil(w/2) (interleaved) or ceil(w/2) (planar).  Bytes of the pitch
    padding are never read; the last row of the last plane may end with its last sample.
    With h and w left out, `data` is the rawvideo layout: a 2-D array [h + h // 2, w] with even h, w and tight pitches."""

    def __init__(self, data, h=None, w=None, fmt="nv12", y_pitch=None, c_pitch=None):
        _check_fmt(fmt)
        if not isinstance(data, np.ndarray) or data.dtype != np.uint8:
            raise ValueError(f"a frame's data is a uint8 array, got {getattr(data, 'dtype', type(data))}")
        if (h is None) != (w is None):
            raise ValueError("a frame has both h and w, or neither (the 2-D rawvideo layout)")
        if h is None:
            if data.ndim != 2 or data.shape[0] % 3 or data.shape[1] % 2 or data.size == 0:
                raise ValueError(f"a frame without h, w is a 2-D array [h + h // 2, w] with even h, w, got shape {data.shape}")
            h, w = data.shape[0] // 3 * 2, data.shape[1]
            if y_pitch is not None or c_pitch is not None:
                raise ValueError("a 2-D rawvideo frame has the tight pitches")
        if not data.flags.c_contiguous:
            raise ValueError("a frame's data is one contiguous buffer")
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"frame of {h} x {w}")
        ch, cw = chroma_size(h, w)
        self.c_step = 2 if fmt in ("nv12", "nv21") else 1
        self.y_pitch = w if y_pitch is None else int(y_pitch)
        self.c_pitch = self.c_step * cw if c_pitch is None else int(c_pitch)
        if self.y_pitch < w or self.c_pitch < self.c_step * cw:
            raise ValueError(f"pitches ({self.y_pitch}, {self.c_pitch}) below the minimum ({w}, {self.c_step * cw}) of a "
                             f"{h} x {w} {fmt} frame")
        self.h, self.w, self.fmt = h, w, fmt
        first = h * self.y_pitch
        if self.c_step == 2:
            u, v = (first, first + 1) if fmt == "nv12" else (first + 1, first)
            last_plane = first
        else:
            second = first + ch * self.c_pitch
            u, v = (first, second) if fmt == "i420" else (second, first)
            last_plane = second
        self.y_offset, self.u_offset, self.v_offset = 0, u, v
        # what the layout needs: every plane in full, the last one up to the last sample of its last row
        self.nbytes = last_plane + (ch - 1) * self.c_pitch + self.c_step * cw
        self.data = data.reshape(-1)
        if self.data.size < self.nbytes:
            raise ValueError(f"a {h} x {w} {fmt} frame with pitches ({self.y_pitch}, {self.c_pitch}) needs {self.nbytes} bytes, "
                             f"the buffer has {self.data.size}")

    def planes(self):
        """(Y [h,w], U [ch,cw], V [ch,cw]) as views of the buffer, without the pitch padding."""
        ch, cw = chroma_size(self.h, self.w)
        d = self.data

        def plane(off, rows, pitch, cols, step):
            idx = off + np.arange(rows)[:, None] * pitch + np.arange(cols)[None, :] * step
            return d[idx]
        return (plane(0, self.h, self.y_pitch, self.w, 1), plane(self.u_offset, ch, self.c_pitch, cw, self.c_step),
                plane(self.v_offset, ch, self.c_pitch, cw, self.c_step))

    def fill_desc(self, d, base=0, flag_word=0):
        """The frame's fields of a y4_yuv_desc row `d`, for a buffer that lies at byte `base` of the source buffer."""
        d.y_offset, d.u_offset, d.v_offset = base + self.y_offset, base + self.u_offset, base + self.v_offset
        d.y_pitch, d.c_pitch, d.c_step, d.h, d.w, d.flags = self.y_pitch, self.c_pitch, self.c_step, self.h, self.w, flag_word


def as_frame(frame, fmt="nv12"):
    """A YuvFrame as it is; a 2-D uint8 array [h + h // 2, w] (even h, w: the rawvideo layout) as a frame of format `fmt`."""
    if isinstance(frame, YuvFrame):
        return frame
    return YuvFrame(frame, fmt=fmt)


def as_frames(frames, fmt="nv12"):
    """One frame or a list of them -> a non-empty list of YuvFrame, or ValueError."""
    if isinstance(frames, YuvFrame) or (isinstance(frames, np.ndarray) and frames.ndim == 2):
        frames = [frames]
    frames = [as_frame(f, fmt) for f in frames]
    if not frames:
        raise ValueError("no frames")
    return frames


def convert_px(Y, U, V, matrix="bt601", full_range=False):
    """The colour rule on integer arrays of equal shape (values 0..255) -> uint8 [..., 3]."""
    flags(matrix, full_range)
    y0, cy, crv, cgu, cgv, cbu = COEFFS[(matrix, bool(full_range))]
    C = np.asarray(Y, np.int32) - np.int32(y0)
    D = np.asarray(U, np.int32) - np.int32(128)
    E = np.asarray(V, np.int32) - np.int32(128)
    luma = np.int32(cy) * C + np.int32(8192)
    rgb = np.stack([luma + np.int32(crv) * E, luma + np.int32(cgu) * D + np.int32(cgv) * E, luma + np.int32(cbu) * D], axis=-1)
    return np.clip(rgb >> 14, 0, 255).astype(np.uint8)          # (>> on a signed NumPy integer is arithmetic)


def to_rgb(frame, matrix="bt601", full_range=False, fmt="nv12"):
    """The RGB image [h,w,3] of a frame at source resolution under the device's rule, integer arithmetic."""
    f = as_frame(frame, fmt)
    Y, U, V = f.planes()
    ys, xs = np.arange(f.h) >> 1, np.arange(f.w) >> 1
    return convert_px(Y, U[ys][:, xs], V[ys][:, xs], matrix, full_range)


def forward_matrix(matrix="bt601", full_range=False):
    """(M [3,3], offset [3]) in float64: [Y, U, V] = M @ [R, G, B] + offset for RGB in 0..255."""
    flags(matrix, full_range)
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    m = np.array([[kr, kg, kb],
                  [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5],
                  [0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]], np.float64)
    if full_range:
        return m, np.array([0.0, 128.0, 128.0])
    return m * np.array([[219.0 / 255.0], [224.0 / 255.0], [224.0 / 255.0]]), np.array([16.0, 128.0, 128.0])


def from_rgb(img, fmt="nv12", matrix="bt601", full_range=False, y_pitch=None, c_pitch=None, fill=0):
    """uint8 RGB [h,w,3] -> YuvFrame: the float64 forward matrix, round half up, clamp to 0..255.  A chroma sample is the rounded
    mean of the unrounded chroma of its 2 x 2 block; the edge blocks of an odd size are averaged over the pixels that exist.
    `fill` is the byte that goes into the pitch padding."""
    _check_fmt(fmt)
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"expected a uint8 [h,w,3] image, got {img.dtype} {img.shape}")
    h, w = img.shape[:2]
    ch, cw = chroma_size(h, w)
    m, off = forward_matrix(matrix, full_range)
    yuv = img.astype(np.float64) @ m.T + off

    def quant(a):
        return np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)

    rows, cols = np.arange(0, h, 2), np.arange(0, w, 2)
    sums = np.add.reduceat(np.add.reduceat(yuv[:, :, 1:], rows, axis=0), cols, axis=1)
    count = np.add.reduceat(np.add.reduceat(np.ones((h, w)), rows, axis=0), cols, axis=1)
    chroma = quant(sums / count[:, :, None])
    step = 2 if fmt in ("nv12", "nv21") else 1
    y_pitch = w if y_pitch is None else int(y_pitch)
    c_pitch = step * cw if c_pitch is None else int(c_pitch)
    if y_pitch < w or c_pitch < step * cw:
        raise ValueError(f"pitches ({y_pitch}, {c_pitch}) below the minimum ({w}, {step * cw}) of a {h} x {w} {fmt} frame")
    buf = np.full(h * y_pitch + (1 if step == 2 else 2) * ch * c_pitch, int(fill), np.uint8)
    buf[:h * y_pitch].reshape(h, y_pitch)[:, :w] = quant(yuv[:, :, 0])
    first = h * y_pitch
    if step == 2:
        plane = buf[first:].reshape(ch, c_pitch)
        plane[:, 0:2 * cw:2] = chroma[:, :, 0 if fmt == "nv12" else 1]
        plane[:, 1:2 * cw:2] = chroma[:, :, 1 if fmt == "nv12" else 0]
    else:
        planes = buf[first:].reshape(2, ch, c_pitch)
        planes[0, :, :cw] = chroma[:, :, 0 if fmt == "i420" else 1]
        planes[1, :, :cw] = chroma[:, :, 1 if fmt == "i420" else 0]
    return YuvFrame(buf, h, w, fmt, y_pitch, c_pitch)
