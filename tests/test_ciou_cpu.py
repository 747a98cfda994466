"""The CIoU box term without a GPU: the float64 restatement (tests/ciou_oracle.py) against the reference-generated fixtures
(the reference's own loss.py with bbox_ciou switched in, tests/golden/make_ciou_fixtures.py) and against torch autograd of the
restatement's own forward; the fixture files; the host-only ABI of y4_set_box_loss / y4_get_box_loss.

Float64 against float64 is held to 1e-10 relative to the largest magnitude, the bar blockgrad_oracle is held to against autograd."""
import ctypes as C
import os

import numpy as np
import pytest

import ciou_oracle as CO
import loss_cases as LC
import loss_oracle as LO
import lossgrad_cases as GC
import lossgrad_oracle as GO
from helpers import ROOT
from test_lossgrad_cpu import D_REF_MAX, load_grad_fixture

GOLDEN = os.path.join(ROOT, "tests", "golden")
CASE_NAMES = sorted(GC.CASES)
F64_BAR = 1e-10


def load_ciou_fixture(name):
    """-> (case inputs, dense labels, true_xywh, fixture dict: g32 / g64 per scale [n, gh, gw, 3, 5 + C], d_ref [3], terms32 /
    terms64 [n, 3, 3], terms_d_ref [3, 3], total32, total64)."""
    from yolo4hip.data import preprocess_true_boxes
    case = GC.make_case(name)
    fx = np.load(os.path.join(GOLDEN, f"ciou_{name}.npz"))
    assert str(fx["sha"]) == case["sha"], "the seeded inputs drifted from the ones the fixture was generated with"
    labels, xywh = preprocess_true_boxes(case["boxes"], case["hw"], LC.ANCHORS, case["ncls"])
    out = {k: fx[k] for k in ("d_ref", "terms32", "terms64", "terms_d_ref", "total32", "total64")}
    out["g32"], out["g64"] = [], []
    for s, stride in enumerate(LC.STRIDES):
        shape = (case["n"], case["hw"][0] // stride, case["hw"][1] // stride, 3, 5 + case["ncls"])
        for key, dt in (("32", np.float32), ("64", np.float64)):
            g = np.zeros(shape, dtype=dt)
            g.reshape(-1)[fx[f"idx_{s}"]] = fx[f"val{key}_{s}"]
            g[..., 4] = fx[f"conf{key}_{s}"]
            out["g" + key].append(g)
    return case, labels, xywh, out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oracle_terms_and_gradient_equal_the_reference(name):
    case, labels, xywh, fx = load_ciou_fixture(name)
    args = (case["heads"], labels, xywh, LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH, case["hw"])
    terms = CO.loss_terms(*args)
    assert np.isfinite(fx["terms64"]).all() and fx["terms32"].dtype == np.float32
    for s in range(3):
        for c in range(3):
            d = GO.rel_to_max(terms[:, s, c], fx["terms64"][:, s, c])
            print(name, "terms", s, c, d)
            assert d <= F64_BAR
    assert abs(LO.total(terms) - float(fx["total64"])) <= F64_BAR * float(fx["total64"])
    # the stored d_ref of the terms is what the two stored runs give, and it is float32 round-off
    assert np.allclose(LO.rel_dist(fx["terms32"], fx["terms64"]).max(axis=0), fx["terms_d_ref"], rtol=1e-9, atol=0)
    assert fx["terms_d_ref"].max() < 2e-6
    g = CO.loss_grad(*args)
    for s in range(3):
        got = g[s].reshape(fx["g64"][s].shape)
        assert fx["g32"][s].dtype == np.float32 and np.isfinite(fx["g64"][s]).all()
        assert GO.rel_to_max(fx["g32"][s], fx["g64"][s]) == pytest.approx(float(fx["d_ref"][s]), rel=1e-9)
        assert 1e-8 < fx["d_ref"][s] < D_REF_MAX.get(name, 1e-6)
        d64 = GO.rel_to_max(got, fx["g64"][s])
        box = GO.rel_to_max(got[..., 0:4], fx["g64"][s][..., 0:4])       # the four box columns on their own scale
        print(name, s, "oracle vs reference f64:", d64, "box columns:", box)
        assert d64 <= F64_BAR and box <= F64_BAR
        rest = fx["g64"][s].copy()
        rest[..., 4] = 0
        assert not rest[labels[s][..., 4] == 0].any()
    d_min, c2_min = CO.lane_conditions(*args[:2], *args[3:6], case["hw"])
    assert d_min >= 0.01 and c2_min >= 1.0


@pytest.mark.parametrize("name", CASE_NAMES)
def test_analytic_gradient_equals_autograd_of_the_oracles_forward(name):
    import torch
    case, labels, _, _ = load_ciou_fixture(name)
    anchors3 = LC.ANCHORS.reshape(3, 3, 2).astype(np.float64)
    area = float(case["hw"][0] * case["hw"][1])
    for s in range(3):
        _, t4, grid, anc, lab = CO.lanes(case["heads"][s], labels[s], anchors3[s], case["ncls"])
        assert len(t4) > 0
        want = CO.lane_grad(t4, grid, anc, lab, float(LC.STRIDES[s]), area)
        leaf = torch.tensor(t4, dtype=torch.float64, requires_grad=True)
        f = CO.forward(leaf, torch.tensor(grid), torch.tensor(anc), torch.tensor(lab), float(LC.STRIDES[s]), area, xp=torch)
        assert np.abs(f["term"].detach().numpy() - CO.forward(t4, grid, anc, lab, float(LC.STRIDES[s]), area)["term"]).max() <= 1e-12
        f["term"].sum().backward()
        d = GO.rel_to_max(want, leaf.grad.numpy())
        print(name, s, "analytic vs autograd:", d)
        assert d <= F64_BAR


@pytest.mark.parametrize("name", CASE_NAMES)
def test_fixture_files_and_the_swap_took(name):
    path = os.path.join(GOLDEN, f"ciou_{name}.npz")
    largest = max(os.path.getsize(os.path.join(GOLDEN, f"lossgrad_{n}.npz")) for n in CASE_NAMES)
    assert os.path.getsize(path) <= largest < 1 << 20
    case, labels, xywh, fx = load_ciou_fixture(name)
    _, _, _, giou = load_grad_fixture(name)
    giou_terms = LO.loss_terms(case["heads"], labels, xywh, LC.ANCHORS, LC.STRIDES, case["ncls"], LC.IOU_LOSS_THRESH, case["hw"])
    for s in range(3):
        # another box term: its sums and its four gradient columns differ, the confidence and class parts are the same numbers
        assert np.all(LO.rel_dist(fx["terms64"][:, s, 0], giou_terms[:, s, 0])[giou_terms[:, s, 0] != 0] > 1e-3)
        assert GO.rel_to_max(fx["terms64"][:, s, 1:], giou_terms[:, s, 1:]) <= F64_BAR
        assert GO.rel_to_max(fx["g64"][s][..., 0:4], giou["g64"][s][..., 0:4]) > 1e-2
        assert np.array_equal(fx["g64"][s][..., 4:], giou["g64"][s][..., 4:])


def test_box_loss_abi_host_only():
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    lib = ext.load()
    cfg = _cfg_struct(make_config(64), 2, 1, "f16")
    h, h2 = C.c_void_p(), C.c_void_p()
    assert lib.y4_create(C.byref(cfg), C.byref(h)) == 0 and lib.y4_create(C.byref(cfg), C.byref(h2)) == 0
    assert lib.y4_get_box_loss(h) == 0                                       # a fresh handle: GIoU
    a0, w0 = C.c_size_t(), C.c_size_t()
    assert lib.y4_workspace_bytes(h, C.byref(a0), C.byref(w0)) == 0
    assert lib.y4_set_box_loss(h, 1) == 0 and lib.y4_get_box_loss(h) == 1
    for bad in (2, -1):
        assert lib.y4_set_box_loss(h, bad) == -22
        assert b"y4_set_box_loss" in lib.y4_last_error() and b"CIoU" in lib.y4_last_error()
        assert lib.y4_get_box_loss(h) == 1                                   # a refused kind changes nothing
    a1, w1 = C.c_size_t(), C.c_size_t()
    assert lib.y4_workspace_bytes(h, C.byref(a1), C.byref(w1)) == 0
    assert (a0.value, w0.value) == (a1.value, w1.value)                      # no workspace effect
    assert lib.y4_copy_schedule(h, h2) == 0 and lib.y4_get_box_loss(h2) == 0  # not a scheduling choice
    assert lib.y4_set_box_loss(h, 0) == 0 and lib.y4_get_box_loss(h) == 0
    assert lib.y4_set_box_loss(None, 1) < 0 and lib.y4_get_box_loss(None) < 0
    assert lib.y4_destroy(h) == 0 and lib.y4_destroy(h2) == 0


def test_facade_refuses_an_unknown_box_loss_before_touching_the_device():
    from yolo4hip.api import Yolov4
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from helpers import CLASS_DIR
    with pytest.raises(ValueError, match="box_loss"):
        Yolov4(None, os.path.join(CLASS_DIR, "bccd_classes.txt"), make_config(160), box_loss="xiou", tune=False)
    with pytest.raises(ValueError, match="box_loss"):
        Engine(3, make_config(160), max_batch=1, box_loss="xiou")
