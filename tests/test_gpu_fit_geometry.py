"""y4_block_grad and y4_head_grad (csrc/block_train.hip, csrc/head_train.hip) after a real forward at the grid shapes and class
counts that training runs at: the two-row strip of the weight gradient by both routes, launches with more than 64 KB of dynamic
LDS, 16-bit staging of rows that are no multiple of 8 or odd, strips and slice ranges that end outside an image, the refusal of
a grid row that does not fit the LDS, and 80 classes.  Rectangular inputs of 96 rows keep every case small: only the width has to
reach the path.

tests/blockgrad_oracle.py restates the geometry (wgrad_geometry, scratch_bytes); y4_block_grad_scratch_bytes must equal it for
every case, which pins the restatement to the library, and every case asserts from it which paths it reaches (REACHES), so that a
later change of a constant cannot turn a case into a copy of another one.  tests/test_blockgrad_cpu.py asserts that the table as
a whole reaches every path.

Budget of every comparison: the rule of tests/test_gpu_fit.py and tests/test_gpu_fit_blocks.py, rel_to_max <= max(4 x d_ref, 1e-6),
d_ref from the oracle alone (float32 evaluation for a float32 handle, dZ rounded to bf16 for a bf16 handle).  dK is held to it as
a whole and tap by tap -- distance, d_ref and largest magnitude taken over the [:, :, kh, kw] slice alone: a corner tap has fewer
terms than the centre, and an error confined to it can hide under the whole tensor's maximum.  Every distance goes to
profiles/fit/parity_measured.json beside its budget.

Batches: images 1 .. 3 of loss_cases.make_boxes (the one with max_boxes boxes and the one with two records on one cell and
anchor are in every batch), unequal image weights.  (96, 1408) runs three images: a bf16 handle reaches 6 slices over 4 ranges
at no smaller shape (its stride-32 grid keeps four rows up to 43 cells)."""
import ctypes as C

import numpy as np
import pytest

import blockgrad_oracle as BO
import loss_cases as LC
import lossgrad_oracle as GO
from test_gpu_fit import _bits, _engine, _note, _unpack, _within
from test_gpu_fit_blocks import BLOCK_IN, HEAD_IN, _layer_params, _unpack_k

pytestmark = pytest.mark.gpu
CHANNELS = ((128, 256), (256, 512), (512, 1024))                             # (cin, cout) of convs 92 / 100 / 108
# hw -> classes, images, seed, dtypes of the block gradient, dtypes of the head gradient
CASES = {
    (96, 352): (3, 2, 21, ("f32", "bf16"), ("f32", "bf16")),
    (96, 416): (80, 2, 22, ("f32", "bf16"), ("f32", "bf16", "f16")),           # the 416 workload's widths 52 / 26 / 13, 80 classes
    (96, 608): (3, 3, 23, ("f32", "bf16"), ("f32", "bf16")),
    (96, 800): (3, 3, 24, ("f32",), ("f32",)),                                  # 100 cells: the largest float32 tile
    (96, 864): (3, 2, 25, ("bf16",), ("bf16",)),                                # 108 cells: float32 refuses (test_refusal_...)
    (96, 1408): (3, 3, 26, ("bf16",), ("bf16",)),
}
# (hw, dtype) -> [(scale, path of blockgrad_oracle.wgrad_branches)] the case is there for
REACHES = {
    ((96, 352), "f32"): [(0, "R2_fall_back"), (0, "lds_above_64k"), (1, "R4")],
    ((96, 352), "bf16"): [(0, "R2_fall_back"), (0, "Wp_above_W"), (1, "Wp_above_W"), (2, "odd_W_pair")],
    ((96, 416), "f32"): [(0, "R2_fall_back"), (0, "lds_above_64k"), (1, "R2_fall_back")],
    ((96, 416), "bf16"): [(0, "R2_fall_back"), (0, "Wp_above_W"), (1, "R4"), (1, "Wp_above_W"), (2, "odd_W_pair")],
    ((96, 608), "f32"): [(0, "R2_wide_start"), (0, "lds_above_64k"), (1, "R2_fall_back"), (2, "R4_last_strip_partial")],
    ((96, 608), "bf16"): [(0, "R2_wide_start"), (0, "lds_above_64k"), (0, "Wp_above_W"), (1, "R4_last_strip_partial"), (1, "Wp_above_W"),
                          (2, "R4_last_strip_partial"), (2, "odd_W_pair")],
    ((96, 800), "f32"): [(0, "R2_wide_start"), (0, "lds_above_64k"), (2, "R2_fall_back"), (2, "R2_last_strip_partial"), (2, "uneven_split"),
                         (2, "range_crosses_image")],
    ((96, 864), "bf16"): [(0, "R2_wide_start"), (0, "lds_above_64k"), (0, "Wp_above_W")],
    ((96, 1408), "bf16"): [(0, "R2_wide_start"), (0, "lds_above_64k"), (2, "R2_fall_back"), (2, "R2_last_strip_partial"), (2, "uneven_split"),
                          (2, "range_crosses_image")],
}
# the dynamic LDS of the stride-8 scale's launch, computed by hand from DESIGN.md 7e
LDS_SCALE0 = {((96, 352), "f32"): 70144, ((96, 416), "f32"): 82432, ((96, 416), "bf16"): 49152, ((96, 608), "f32"): 119296,
              ((96, 800), "f32"): 156160, ((96, 864), "bf16"): 92160, ((96, 1408), "bf16"): 141312}
BLOCK_CASES = [(hw, dt) for hw, c in CASES.items() for dt in c[3]]
HEAD_CASES = [(hw, dt) for hw, c in CASES.items() for dt in c[4]]
WEIGHTS = np.array([0.4, 0.1, 0.3, 0.2], np.float32)


def grids(hw):
    return [(hw[0] // s, hw[1] // s) for s in LC.STRIDES]


def geometries(hw, dtype, n):
    return [BO.wgrad_geometry(dtype, n, gh, gw, cin, cout) for (gh, gw), (cin, cout) in zip(grids(hw), CHANNELS)]


def reached(hw, dtype, n):
    """[(scale, path)] of the three weight-gradient launches of a case"""
    return [(s, b) for s, ((gh, gw), g) in enumerate(zip(grids(hw), geometries(hw, dtype, n))) for b in sorted(BO.wgrad_branches(dtype, gh, gw, g))]


def _boxes(hw, ncls, n, seed):
    return np.ascontiguousarray(LC.make_boxes(hw, ncls, 4, seed)[{2: [1, 3], 3: [1, 2, 3]}[n]])


def _scratch_bytes(eng, n):
    from yolo4hip import ext
    size = C.c_size_t()
    ext.check(eng.lib.y4_block_grad_scratch_bytes(eng.handle, n, C.byref(size)))
    return size.value


def _forward(hw, dtype, level):
    """Two engines after a forward of the case's batch: the one under test (aliased workspace, fused chains, retention `level`)
    and the non-aliased unfused one the taps are read from.  -> dict"""
    import torch
    from yolo4hip.data import preprocess_true_boxes
    ncls, n, seed = CASES[hw][:3]
    eng, flat = _engine(hw, ncls, n, dtype, alias_workspace=True, retain_head_inputs=level)
    ref, _ = _engine(hw, ncls, n, dtype)
    if dtype != "f32":
        assert eng.set_chain_fusion(True) > 0
    imgs = torch.from_numpy(np.random.default_rng(4).uniform(0, 1, size=(n,) + tuple(hw) + (3,)).astype(np.float32)).to(eng.device)
    boxes = _boxes(hw, ncls, n, seed)
    eng.forward_device(imgs)
    ref.forward_device(imgs)
    heads = [h.cpu().numpy() for h in eng.heads_device(n)]
    for a, b in zip(heads, ref.heads_device(n)):
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    labels, xywh = preprocess_true_boxes(boxes, hw, LC.ANCHORS, ncls)
    assert sorted(int((b[:, 2] > b[:, 0]).sum()) for b in boxes)[-1] == LC.MAX_BOXES

    def g64(w):
        return GO.loss_grad(heads, labels, xywh, LC.ANCHORS, LC.STRIDES, ncls, 0.5, hw, img_weight=w)
    return dict(eng=eng, ref=ref, flat=flat, imgs=imgs, boxes_dev=torch.from_numpy(boxes).to(eng.device), ncls=ncls, n=n, w=WEIGHTS[:n].copy(),
                g64=g64, torch=torch)


def _block_oracle(c, dtype, g64):
    """-> per scale (float64 dK, the oracle's own evaluation at the handle's precision)"""
    U = [c["ref"].conv_output(i, c["n"]) for i in BLOCK_IN]
    A = [c["ref"].conv_output(i, c["n"]) for i in HEAD_IN]
    out = []
    for s, (wh, _, _, bn) in enumerate(_layer_params(c["eng"], c["flat"], dtype)):
        sc = BO.bn_scale(bn[1], bn[3])
        dk64 = BO.block_grad(g64[s], wh, A[s], U[s], sc)
        if dtype == "f32":
            other = BO.block_grad(g64[s].astype(np.float32), wh, A[s], U[s], BO.bn_scale(bn[1], bn[3], np.float32), np.float32)
        else:
            other = BO.block_grad(g64[s], wh, A[s], U[s], sc, round_dz=BO.round_bf16)
        assert dk64.shape == (CHANNELS[s][1], CHANNELS[s][0], 3, 3)
        out.append((dk64, other))
    return out


def _hold_dk(tag, eng, dk, oracle):
    """dK of the three scales against the oracle: as a whole, then each of the nine taps on its own"""
    for s, (got, (want, other)) in enumerate(zip(_unpack_k(eng, dk), oracle)):
        assert got.shape == want.shape
        _within(f"{tag}_scale{s}_dK", got, want, GO.rel_to_max(other, want))
        for kh in range(3):
            for kw in range(3):
                t = want[:, :, kh, kw]
                assert np.abs(t).max() > 0
                _within(f"{tag}_scale{s}_dK_tap{kh}{kw}", got[:, :, kh, kw], t, GO.rel_to_max(other[:, :, kh, kw], t))


# ---- 1. the kernel gradient
@pytest.mark.parametrize("hw,dtype", BLOCK_CASES)
def test_block_grad_at_training_geometry(hw, dtype):
    c = _forward(hw, dtype, 2)
    eng, n, w, torch = c["eng"], c["n"], c["w"], c["torch"]
    lt = eng.layer_table()
    assert tuple((lt[i]["cin"], lt[i]["cout"]) for i in eng.BLOCK_CONVS) == CHANNELS
    # the paths this case is there for, and the restatement against the library for every batch size the test runs
    geo, hit = geometries(hw, dtype, n), reached(hw, dtype, n)
    for s, g in enumerate(geo):
        print(f"wgrad geometry {hw} {dtype} n={n} scale {s} grid {grids(hw)[s]}: {g}")
    print("reaches:", hit)
    _note(f"block_grad_{hw[0]}x{hw[1]}_{dtype}_geometry", {"n": n, "scales": geo, "reaches": [f"{s}:{b}" for s, b in hit]})
    assert set(REACHES[(hw, dtype)]) <= set(hit), (REACHES[(hw, dtype)], hit)
    if (hw, dtype) in LDS_SCALE0:
        assert geo[0]["lds_bytes"] == LDS_SCALE0[(hw, dtype)]
    for m in sorted({1, n - 1, n}):
        assert _scratch_bytes(eng, m) == BO.scratch_bytes(dtype, m, grids(hw), CHANNELS), m
    oracle = _block_oracle(c, dtype, c["g64"](w))
    tag = f"block_grad_{hw[0]}x{hw[1]}_c{c['ncls']}_{dtype}"
    dk = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    _hold_dk(tag, eng, dk.cpu().numpy(), oracle)
    again = eng.block_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    assert np.array_equal(_bits([dk])[0], _bits([again])[0])

    # two accumulated calls of unequal size: one image, then the rest
    def chunked():
        acc = torch.empty_like(dk)
        w_dev = torch.from_numpy(w).to(eng.device)
        for i0, i1 in ((0, 1), (1, n)):
            eng.forward_device(c["imgs"][i0:i1])
            eng.block_grad_device(i1 - i0, boxes_dev=c["boxes_dev"][i0:i1], img_weight=w_dev[i0:i1], dk=acc, accumulate=i0 > 0)
        return acc.cpu().numpy()
    two = chunked()
    assert np.array_equal(two.view(np.int32), chunked().view(np.int32))
    _hold_dk(tag + "_chunks", eng, two, oracle)
    if hw == (96, 608):
        # the position of an image in the batch changes the slice order, not the value: with weights of one the batch in order
        # and the reversed batch are both within the budget of the same float64 gradient
        ones = np.ones(n, np.float32)
        oracle1 = _block_oracle(c, dtype, c["g64"](ones))
        rev = list(range(n))[::-1]
        for name, order in (("in_order", list(range(n))), ("reversed", rev)):
            eng.forward_device(c["imgs"][order].contiguous())
            dk1 = eng.block_grad_device(n, boxes_dev=c["boxes_dev"][order].contiguous(), img_weight=ones)
            _hold_dk(f"{tag}_ones_{name}", eng, dk1.cpu().numpy(), oracle1)
    eng.close()
    c["ref"].close()


# ---- 2. the head gradient
def _hold_dw(tag, eng, dw, g64, X):
    for s, (db, dW) in enumerate(_unpack(eng, dw)):
        db64, dW64 = GO.head_wgrad(g64[s], X[s])
        db32, dW32 = GO.head_wgrad(g64[s].astype(np.float32), X[s], np.float32)
        _within(f"{tag}_scale{s}_dW", dW, dW64, GO.rel_to_max(dW32, dW64))
        _within(f"{tag}_scale{s}_db", db, db64, GO.rel_to_max(db32, db64))


def _head_grad_checks(c, tag):
    eng, n, w, torch = c["eng"], c["n"], c["w"], c["torch"]
    X = [c["ref"].conv_output(i, n) for i in HEAD_IN]
    g64 = c["g64"](w)
    dw = eng.head_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    assert dw.numel() == sum(3 * (5 + c["ncls"]) * (1 + cout) for _, cout in CHANNELS)
    _hold_dw(tag, eng, dw.cpu().numpy(), g64, X)
    again = eng.head_grad_device(n, boxes_dev=c["boxes_dev"], img_weight=w)
    assert np.array_equal(_bits([dw])[0], _bits([again])[0])

    def chunked():
        acc = torch.empty_like(dw)
        w_dev = torch.from_numpy(w).to(eng.device)
        for i0, i1 in ((0, 1), (1, n)):
            eng.forward_device(c["imgs"][i0:i1])
            eng.head_grad_device(i1 - i0, boxes_dev=c["boxes_dev"][i0:i1], img_weight=w_dev[i0:i1], dw=acc, accumulate=i0 > 0)
        return acc.cpu().numpy()
    two = chunked()
    assert np.array_equal(two.view(np.int32), chunked().view(np.int32))
    _hold_dw(tag + "_chunks", eng, two, g64, X)


@pytest.mark.parametrize("hw,dtype", HEAD_CASES)
def test_head_grad_at_training_geometry(hw, dtype):
    c = _forward(hw, dtype, True)
    _head_grad_checks(c, f"head_grad_{hw[0]}x{hw[1]}_c{c['ncls']}_{dtype}")
    c["eng"].close()
    c["ref"].close()


# ---- 3. a grid row that does not fit the LDS
def test_refusal_of_a_grid_row_that_does_not_fit():
    """108 cells at the stride-8 scale, float32: the two-row tile is 64 x (4 x 110 | 1 + 2 x 108 | 1) x 4 = 168,448 bytes, above the
    160 KB of a compute unit.  y4_block_grad_scratch_bytes refuses it on the host, and Engine.block_grad_device asks it for the
    scratch before it calls y4_block_grad (which checks the same before its first launch): nothing of the block gradient runs.
    (A bf16 handle at this shape needs 92,160 bytes and computes: the (96, 864) case above.)"""
    from yolo4hip import ext
    hw = (96, 864)
    assert grids(hw)[0][1] == 108 and 64 * (((4 * 110) | 1) + ((2 * 108) | 1)) * 4 == 168448 > BO.LDS_LIMIT
    assert geometries(hw, "f32", 2)[0] is None and BO.scratch_bytes("f32", 2, grids(hw), CHANNELS) is None
    c = _forward(hw, "f32", 2)
    eng, n = c["eng"], c["n"]
    triple = eng.assign_device(c["boxes_dev"])                              # labels first: the refused call launches nothing
    with pytest.raises(ext.Y4Error) as err:
        _scratch_bytes(eng, n)
    assert err.value.code == -22 and "grid row of 108 cells" in str(err.value)
    with pytest.raises(ext.Y4Error) as err:
        eng.block_grad_device(n, records=triple, img_weight=c["w"])
    assert err.value.code == -22 and "grid row of 108 cells" in str(err.value)
    # the head gradient of the same engine is untouched by the refusal
    _head_grad_checks(c, "head_grad_96x864_c3_f32_after_refusal")
    eng.close()
    c["ref"].close()
