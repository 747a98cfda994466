"""The float64 statement of the four YUV -> RGB matrices (BT.601 / BT.709, limited / full range), from (Kr, Kb) alone: what
`yolo4hip.yuv.to_rgb` and `y4_yuv_u8_ragged` approximate with 14-bit integer coefficients.

  Y' = (Y - y0) ys,  Pb = (U - 128) cs,  Pr = (V - 128) cs        ys = 255/219, cs = 255/224, y0 = 16 (limited range);  1, 1, 0 (full)
  R = Y' + 2 (1 - Kr) Pr
  G = Y' - (2 Kb (1 - Kb) / Kg) Pb - (2 Kr (1 - Kr) / Kg) Pr      Kg = 1 - Kr - Kb
  B = Y' + 2 (1 - Kb) Pb
"""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
CASES = [(m, f) for m in ("bt601", "bt709") for f in (False, True)]


def real_coeffs(matrix, full_range):
    """(y0, cy, crv, cgu, cgv, cbu) as real numbers."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full_range else 16, ys, 2 * (1 - kr) * cs, -2 * kb * (1 - kb) / kg * cs, -2 * kr * (1 - kr) / kg * cs,
            2 * (1 - kb) * cs)


def exact_rgb(Y, U, V, matrix, full_range):
    """float64 [..., 3], not rounded and not clamped."""
    y0, cy, crv, cgu, cgv, cbu = real_coeffs(matrix, full_range)
    C = np.asarray(Y, np.float64) - y0
    D = np.asarray(U, np.float64) - 128.0
    E = np.asarray(V, np.float64) - 128.0
    return np.stack([cy * C + crv * E, cy * C + cgu * D + cgv * E, cy * C + cbu * D], axis=-1)
