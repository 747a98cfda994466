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


def test_round_bf16_is_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 0.0], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, -1.0, 1.0 + 2.0 ** -7, 0.0])
    assert np.array_equal(BO.round_bf16(x), want)
