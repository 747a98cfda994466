"""tests/blockgrad_oracle.py against torch autograd in float64: conv2d(padding 1) -> frozen-BN affine -> leaky_relu(0.1) -> 1x1 conv
-> the project's float64 loss gradient (tests/lossgrad_oracle.py) injected at the raw heads.  Exact math on both sides: 1e-10
relative to the largest magnitude."""
import numpy as np
import pytest

import blockgrad_oracle as BO
import loss_cases as LC
import lossgrad_oracle as GO
from helpers import ROOT  # noqa: F401  (puts the package on sys.path)


@pytest.mark.parametrize("hw,seed", [((96, 96), 3), ((64, 128), 5), ((128, 64), 7)])
def test_block_grad_oracle_vs_autograd(hw, seed):
    import torch
    import torch.nn.functional as F
    from yolo4hip.data import preprocess_true_boxes
    ncls, n, nout = 3, 4, 3 * (3 + 5)
    rng = np.random.default_rng(seed)
    boxes = LC.make_boxes(hw, ncls, n, seed=seed)
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    w = np.array([0.4, 0.1, 0.3, 0.2])
    heads, parts = [], []
    for s, stride in enumerate(LC.STRIDES):
        gh, gw, cin, cout = hw[0] // stride, hw[1] // stride, 4 + s, 6 + 2 * s
        u = rng.normal(size=(n, gh, gw, cin))
        k = torch.tensor(rng.normal(size=(cout, cin, 3, 3)) * 0.3, requires_grad=True)
        gamma, beta, mean, var = rng.uniform(0.5, 1.5, cout), rng.normal(size=cout) * 0.1, rng.normal(size=cout) * 0.1, rng.uniform(0.5, 2.0, cout)
        wh, bh = rng.normal(size=(nout, cout)) * 0.3, rng.normal(size=nout) * 0.1
        sc = BO.bn_scale(gamma, var)
        z = F.conv2d(torch.tensor(u).permute(0, 3, 1, 2), k, padding=1)
        z = z * torch.tensor(sc).view(1, -1, 1, 1) + torch.tensor(beta - mean * sc).view(1, -1, 1, 1)
        a = F.leaky_relu(z, 0.1)
        head = F.conv2d(a, torch.tensor(wh).view(nout, cout, 1, 1), torch.tensor(bh)).permute(0, 2, 3, 1)
        heads.append(head.detach().numpy())
        parts.append((u, k, a.detach().permute(0, 2, 3, 1).numpy(), wh, sc, head))
    g = GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw, img_weight=w)
    for s, (u, k, a, wh, sc, head) in enumerate(parts):
        head.backward(gradient=torch.tensor(g[s]))
        want = k.grad.numpy()
        got = BO.block_grad(g[s], wh, a, u, sc)
        assert got.shape == want.shape and np.abs(want).max() > 0
        dist = GO.rel_to_max(got, want)
        print(f"scale {s}: rel_to_max {dist:.3e}")
        assert dist <= 1e-10, (s, dist)


def test_wgrad_geometry_restatement_gives_the_hand_computed_tiles():
    """LDS bytes = 64 channels x (uchan + dchan) x element size, worked out by hand from DESIGN.md 7e for the 12-row stride-8 grid
    of convs 92 (128 -> 256)."""
    def geo(dtype, W, n=2, H=12, cin=128, cout=256):
        return BO.wgrad_geometry(dtype, n, H, W, cin, cout)
    # bf16 at 52 cells: four rows are 64 x (392 + 232) x 2 = 79,872 bytes, so two: Wp 56, upitch 64, 64 x (264 + 120) x 2
    g = geo("bf16", 52)
    assert (g["R"], g["Wp"], g["upitch"], g["uchan"], g["dchan"], g["lds_bytes"]) == (2, 56, 64, 264, 120, 49152)
    assert (g["strips"], g["slices"], g["splits"]) == (6, 12, 12)          # 8 tiles -> 64 splits, clamped to the slice count
    # float32: 64 x ((4 (W + 2) | 1) + (2 W | 1)) x 4
    for W, want in ((44, 70144), (52, 82432), (76, 119296), (100, 156160), (105, 163840)):
        g = geo("f32", W)
        assert (g["R"], g["Wp"], g["upitch"], g["lds_bytes"]) == (2, W, W + 2, want), W
    assert geo("f32", 106) is None and geo("f32", 108) is None
    assert geo("bf16", 108)["lds_bytes"] == 92160 and geo("bf16", 176)["lds_bytes"] == 141312
    assert geo("bf16", 200)["lds_bytes"] == 159744 and geo("bf16", 201) is None
    # the four-row tile: float32 up to 24 cells (65,024 bytes), two rows from 25 (four would be 67,584); a grid of 64 starts at two
    assert (geo("f32", 24)["R"], geo("f32", 24)["lds_bytes"], geo("f32", 25)["R"]) == (4, 65024, 2)
    assert (geo("bf16", 38)["R"], geo("bf16", 38)["lds_bytes"], geo("bf16", 44)["R"]) == (4, 59392, 2)
    assert geo("f32", 63, H=3)["R"] == 2 and geo("bf16", 64)["R"] == 2 and geo("bf16", 64)["lds_bytes"] < BO.LDS_DEFAULT
    # splits: 512 / tiles, at most the slices; 6 slices over 4 ranges are 1, 2, 1, 2 long and two of them cross an image
    g = BO.wgrad_geometry("f32", 3, 3, 25, 512, 1024)
    assert (g["R"], g["strips"], g["slices"], g["splits"]) == (2, 2, 6, 4)
    assert {"R2_fall_back", "R2_last_strip_partial", "uneven_split", "range_crosses_image"} <= BO.wgrad_branches("f32", 3, 25, g)
    assert BO.wgrad_branches("bf16", 3, 19, BO.wgrad_geometry("bf16", 3, 3, 19, 512, 1024)) == {"R4", "Wp_above_W", "odd_W_pair", "R4_last_strip_partial"}
    # scratch: dZ planes, then partials, each a multiple of 256 bytes
    grids, chans = [(12, 52), (6, 26), (3, 13)], [(128, 256), (256, 512), (512, 1024)]
    dz = [((2 * 12 * 52 * 256 * 2 + 255) // 256) * 256, ((2 * 6 * 26 * 512 * 2 + 255) // 256) * 256, ((2 * 3 * 13 * 1024 * 2 + 255) // 256) * 256]
    parts = [12 * 9 * 256 * 128 * 4, 4 * 9 * 512 * 256 * 4, 2 * 9 * 1024 * 512 * 4]      # slices 12 / 4 / 2 clamp the splits
    assert BO.scratch_bytes("bf16", 2, grids, chans) == sum(dz) + sum(parts)
    assert BO.scratch_bytes("f32", 2, [(12, 108), (6, 54), (3, 27)], chans) is None


def test_geometry_cases_reach_every_path_of_the_weight_gradient():
    """The case table of tests/test_gpu_fit_geometry.py as a whole: every path of wgrad_branches for float32, and for bf16 the
    two that only 16-bit staging has beside them; every case reaches what it is listed for."""
    import test_gpu_fit_geometry as FG
    paths = {"R2_wide_start", "R2_fall_back", "R4", "lds_above_64k", "R2_last_strip_partial", "R4_last_strip_partial", "uneven_split",
             "range_crosses_image"}
    want = {"f32": paths, "bf16": paths | {"Wp_above_W", "odd_W_pair"}}
    seen = {"f32": set(), "bf16": set()}
    assert sorted(FG.REACHES) == sorted(FG.BLOCK_CASES)
    for hw, dtype in FG.BLOCK_CASES:
        assert hw[0] % 32 == 0 and hw[1] % 32 == 0
        hit = FG.reached(hw, dtype, FG.CASES[hw][1])
        assert set(FG.REACHES[(hw, dtype)]) <= set(hit), (hw, dtype, hit)
        seen[dtype] |= {b for _, b in FG.REACHES[(hw, dtype)]}
    assert seen == want
    # the widths the 416 and 608 workloads have at the three scales, in 16-bit staging
    assert {52, 26, 13, 76, 38, 19} <= {gw for hw, dt in FG.BLOCK_CASES if dt == "bf16" for _, gw in FG.grids(hw)}


def test_round_bf16_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 0.0], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7, 0.0])
    assert np.array_equal(BO.round_bf16(x), want)
