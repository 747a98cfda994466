"""The loss gradient without a GPU: the float64 restatement (tests/lossgrad_oracle.py) against the reference-generated
fixtures (autograd through the reference's own loss.py, tests/golden/make_lossgrad_fixtures.py) and against central finite
differences of the loss restatement; the fixture files themselves; the Adam restatement against torch.optim.Adam.

Budget of a comparison with a float64 gradient: 4 x d_ref with a floor of 1e-6, relative to the largest magnitude of the tensor,
where d_ref (in the fixture, per scale) is the distance of the reference's OWN float32 gradient from its float64 one."""
import os

import numpy as np
import pytest

import loss_cases as LC
import loss_oracle as LO
import lossgrad_cases as GC
import lossgrad_oracle as GO
from helpers import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASE_NAMES = sorted(GC.CASES)
FLOOR = 1e-6
# The largest d_ref a fixture may carry: round-off of float32, so that 4 x d_ref is no vacuous budget.  1e-6 for heads of order 1.
# The wide case holds confidence logits t near 17 on non-responsible lanes, where the float32 sigmoid q sits one spacing (2^-24)
# below 1: its gradient K (2 q^2 (1 - q) BCE + q^3), BCE ~ t, then carries the error of 1 - q, at most 2^-24 (for t > 17.33 =
# 25 ln 2 the float32 q is 1 and the dropped term 2 t e^-t is below 2 t 2^-25), times 2 t, plus three half-spacings of q^3:
# (2 x 17.33 + 3) 2^-24 of K, and the tensor's largest magnitude is at least K.
D_REF_MAX = {"160_wide_g": (2 * 17.33 + 3) * 2.0 ** -24}


def load_grad_fixture(name):
    """-> (case inputs, dense labels, true_xywh, fixture dict with g32 / g64: per scale [n, gh, gw, 3, 5 + C], and d_ref [3])."""
    from yolo4hip.data import preprocess_true_boxes
    case = GC.make_case(name)
    fx = np.load(os.path.join(GOLDEN, f"lossgrad_{name}.npz"))
    assert str(fx["sha"]) == case["sha"], "the seeded inputs drifted from the ones the fixture was generated with"
    labels, xywh = preprocess_true_boxes(case["boxes"], case["hw"], LC.ANCHORS, case["ncls"])
    out = {"d_ref": fx["d_ref"], "g32": [], "g64": []}
    for s, stride in enumerate(LC.STRIDES):
        shape = (case["n"], case["hw"][0] // stride, case["hw"][1] // stride, 3, 5 + case["ncls"])
        for key, dt in (("32", np.float32), ("64", np.float64)):
            g = np.zeros(shape, dtype=dt)
            g.reshape(-1)[fx[f"idx_{s}"]] = fx[f"val{key}_{s}"]
            g[..., 4] = fx[f"conf{key}_{s}"]
            out["g" + key].append(g)
    return case, labels, xywh, out


def budget(d_ref):
    return max(4.0 * float(d_ref), FLOOR)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_gradient_equals_reference_autograd(name):
    case, labels, xywh, fx = load_grad_fixture(name)
    g = GO.loss_grad(case["heads"], labels, xywh, LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH, case["hw"])
    for s in range(3):
        assert g[s].shape == case["heads"][s].shape
        got = g[s].reshape(fx["g64"][s].shape)
        assert fx["g32"][s].dtype == np.float32 and np.isfinite(fx["g64"][s]).all()
        # the stored d_ref is what the two stored gradients give
        assert GO.rel_to_max(fx["g32"][s], fx["g64"][s]) == pytest.approx(float(fx["d_ref"][s]), rel=1e-9)
        assert 1e-8 < fx["d_ref"][s] < D_REF_MAX.get(name, 1e-6)
        d32, d64 = GO.rel_to_max(got, fx["g32"][s]), GO.rel_to_max(got, fx["g64"][s])
        print(name, s, "oracle vs reference f32:", d32, "f64:", d64, "budget:", budget(fx["d_ref"][s]))
        assert d32 <= budget(fx["d_ref"][s])
        assert d64 <= 1e-12                                                  # float64 against float64: the same function
        # the structure the training kernels rely on: outside the confidence columns only responsible lanes carry a gradient
        rest = fx["g64"][s].copy()
        rest[..., 4] = 0
        assert not rest[labels[s][..., 4] == 0].any()
        assert (fx["g64"][s][..., 4] != 0).mean() > 0.9


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_gradient_equals_finite_differences(name):
    case, labels, xywh, _ = load_grad_fixture(name)
    ncls, n = case["ncls"], case["n"]
    heads = [h.astype(np.float64) for h in case["heads"]]
    w = np.array([0.4, 0.1, 0.3, 0.2])[:n]                                   # unequal image weights: img_weight is exercised
    g = GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, LC.IOU_LOSS_THRESH, case["hw"], img_weight=w)

    anchors3 = LC.ANCHORS.reshape(3, 3, 2).astype(np.float64)
    area = float(case["hw"][0] * case["hw"][1])

    def objective(s, b):
        """Image b's weighted loss of scale s: the only summand a logit of that image and scale moves (keeps the round-off of
        the difference small)."""
        terms = LO.scale_terms(heads[s][b:b + 1], labels[s][b:b + 1], xywh[b:b + 1], anchors3[s], LC.STRIDES[s], ncls,
                               LC.IOU_LOSS_THRESH, area)[0]
        return float((terms[0] * np.array(LO.WEIGHTS)).sum() * w[b])
    rng = np.random.default_rng(5)
    step, checked = 1e-6, 0
    for s in range(3):
        sh = heads[s].shape[:3] + (3, 5 + ncls)
        resp = np.argwhere(labels[s][..., 4] == 1)
        picks = []
        for lane in resp[rng.permutation(len(resp))[:12]]:                   # responsible lanes: every kind of logit
            for j in list(range(5)) + list(rng.integers(5, 5 + ncls, size=3)):
                picks.append(tuple(lane) + (int(j),))
        for _ in range(40):                                                  # any lane: the confidence logit
            picks.append(tuple(int(rng.integers(0, d)) for d in sh[:4]) + (4,))
        for idx in picks:
            flat = heads[s].reshape(sh)
            keep = flat[idx]
            flat[idx] = keep + step
            up = objective(s, idx[0])
            flat[idx] = keep - step
            down = objective(s, idx[0])
            flat[idx] = keep
            fd = (up - down) / (2 * step)
            an = g[s].reshape(sh)[idx]
            # relative 1e-5, plus what the subtraction of two float64 sums of this size can carry: a few ulp of the objective
            # (its terms are summed in an order that differs between the two evaluations by nothing, so 4 ulp is generous)
            noise = 4 * np.finfo(np.float64).eps * abs(up) / (2 * step)
            assert abs(fd - an) <= 1e-5 * max(abs(an), abs(fd)) + noise, (name, s, idx, fd, an, noise)
            checked += 1
    assert checked >= 300


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_files(name):
    path = os.path.join(GOLDEN, f"lossgrad_{name}.npz")
    assert os.path.getsize(path) < 1 << 20
    assert str(np.load(path)["sha"]) == GC.make_case(name)["sha"]


def test_adam_restatement_is_keras_rule_via_torch():
    """torch.optim.Adam divides by sqrt(v) / sqrt(1 - b2^t) + eps; with the group's eps set each step to eps / sqrt(1 - b2^t)
    its update is lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps): Keras' rule, checked here independently of NumPy."""
    import torch
    rng = np.random.default_rng(2)
    w0 = rng.normal(size=200)
    grads = [rng.normal(size=200) * 10.0 ** rng.integers(-4, 1) for _ in range(5)]
    w, m, v = w0.copy(), np.zeros(200), np.zeros(200)
    p = torch.tensor(w0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.999), eps=1e-7)
    for t, g in enumerate(grads, 1):
        w, m, v = GO.adam_step(w, m, v, g, t, lr=1e-2)
        opt.param_groups[0]["eps"] = 1e-7 / np.sqrt(1.0 - 0.999 ** t)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        assert np.abs(p.detach().numpy() - w).max() < 1e-12
