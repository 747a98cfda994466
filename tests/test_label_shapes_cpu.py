"""The label cases of loss_cases.LABEL_CASES (max_boxes 1 .. 256, 1 .. 65 classes) without a GPU: every case holds the conditions it
is there for (loss_cases.check_case), the host assignment is the reference's own (fixtures written by
tests/golden/make_loss_fixtures.py), the float64 restatements of the loss and of its gradient run on them, and the table as a whole
reaches every piece of the label and training kernels that 100 rows and {3, 80} classes never touch.

What a case reaches is computed from its inputs (`reached`), never listed by hand alone: REACHES says what a case is there for,
the test asserts that it does reach it and that the union is PATHS, so that a later change of a constant or a seed cannot turn a
case into a copy of another one."""
import os

import numpy as np
import pytest

import loss_cases as LC
import loss_oracle as LO
import lossgrad_oracle as GO
from helpers import GOLDEN
from test_loss_cpu import load_fixture

NAMES = list(LC.LABEL_CASES)
ROUND = 256                                                                  # LOSS_THREADS: rows of a workgroup, slots of a sparse round
OLD_SHA = {
    "416_bccd": "aadfdc64a549535da4de7325068be26ff7108bb6ce458c17072d7924b656a227",
    "160_coco": "af8ed2478692b314584852f2d88e62da3d0fea673145c9eb1ecb6bf96b37e805",
    "160_wide": "d34ac56ff1af2aa9762472358d37b35952c17bda5d32f85b9be0bb4ae1a82b5f",
}
# Every path below but one is one that max_boxes = 100 with 3 or 80 classes does not take (test_the_old_geometry_...): bit 31 of a
# mask word is set by class 31 of the 80-class case too; what is new here is bit 31 as the LAST bit of a word (C = 32, 64).
PATHS = {
    "valid_rows_in_wave_2", "valid_rows_in_wave_3",                          # compact_valid: the per-wave base and the four-term total
    "row_shift_crosses_a_wave", "equal_keys_in_three_waves", "more_than_128_valid_rows",      # loss_assign_kernel
    "one_row", "zero_tail_has_nothing_to_do", "more_than_192_records",       # the zero tail of the records
    "records_in_wave_2", "records_in_wave_3",                                # map_records
    "sparse_round_is_one_image", "sparse_round_holds_n_images",              # head_sparse_wgrad_kernel
    "nf_6", "nf_37", "nf_38", "nf_69", "nf_70",                              # block_dgrad_kernel's LDS rows; cout and hcs are 3 nf
    "one_class", "mask_word_exactly_full", "first_bit_of_a_new_word", "bit_31_set", "three_mask_words_in_one_record",
}
REACHES = {
    "mb1_c1": ["one_row", "zero_tail_has_nothing_to_do", "sparse_round_holds_n_images", "nf_6", "one_class"],
    "mb64_c32": ["nf_37", "mask_word_exactly_full", "bit_31_set"],
    "mb65_c33": ["row_shift_crosses_a_wave", "nf_38", "first_bit_of_a_new_word"],
    "mb129_c64": ["valid_rows_in_wave_2", "row_shift_crosses_a_wave", "equal_keys_in_three_waves", "more_than_128_valid_rows", "nf_69",
                  "mask_word_exactly_full", "bit_31_set"],
    "mb256_c65": ["valid_rows_in_wave_2", "valid_rows_in_wave_3", "row_shift_crosses_a_wave", "equal_keys_in_three_waves",
                  "more_than_128_valid_rows", "more_than_192_records", "records_in_wave_2", "records_in_wave_3",
                  "sparse_round_is_one_image", "nf_70", "first_bit_of_a_new_word", "bit_31_set", "three_mask_words_in_one_record"],
}


def reached(max_boxes, ncls, boxes, records, hw=(160, 160)):
    """The paths a batch of boxes with its host records takes, from the inputs alone -> set of names of PATHS"""
    out = set()
    valid = boxes[..., 2] - boxes[..., 0] > 0
    rw = 8 + (ncls + 31) // 32
    for v, rec in zip(valid, records):
        vidx = np.flatnonzero(v)
        for w in (2, 3):
            if (vidx // LC.WAVE == w).any():
                out.add(f"valid_rows_in_wave_{w}")
            if len(rec) > w * LC.WAVE:
                out.add(f"records_in_wave_{w}")
        if (vidx // LC.WAVE > np.arange(len(vidx)) // LC.WAVE).any():
            out.add("row_shift_crosses_a_wave")
        if len(vidx) > 2 * LC.WAVE:
            out.add("more_than_128_valid_rows")
        if len(rec) > 3 * LC.WAVE:
            out.add("more_than_192_records")
        if len(rec) * rw >= max_boxes * rw:                                  # for (i = count * rw + tid; i < mb * rw; ...) never enters
            out.add("zero_tail_has_nothing_to_do")
        for r in rec:
            words = r[8:].view(np.uint32)
            if any(int(w) >> 31 for w in words):
                out.add("bit_31_set")
            if ncls > 32 and any(int(w) & 1 for w in words[1:]):
                out.add("first_bit_of_a_new_word_set")
            if len(words) == 3 and all(int(w) for w in words):
                out.add("three_mask_words_in_one_record")
    rows = LC.trio_rows(max_boxes)
    if rows and valid[3].all():
        keys = [LC._key_of_row(boxes[3, k], hw, ncls) for k in rows]
        if keys[0] == keys[1] == keys[2] and len({k // LC.WAVE for k in rows}) == 3:
            out.add("equal_keys_in_three_waves")
    if max_boxes == 1:
        out.add("one_row")
    if max_boxes == ROUND:
        out.add("sparse_round_is_one_image")
    if max_boxes == 1 and len(boxes) > 1:
        out.add("sparse_round_holds_n_images")
    out.add(f"nf_{5 + ncls}")
    if ncls == 1:
        out.add("one_class")
    if ncls % 32 == 0:
        out.add("mask_word_exactly_full")
    if ncls % 32 == 1 and ncls > 1 and "first_bit_of_a_new_word_set" in out:
        out.add("first_bit_of_a_new_word")
    out.discard("first_bit_of_a_new_word_set")
    return out


def label_fixture(name):
    """-> (case of loss_cases.make_label_case, fixture arrays, the reference's dense labels)"""
    case = LC.make_label_case(name)
    fx = np.load(os.path.join(GOLDEN, f"loss_{name}.npz"))
    assert str(fx["sha"]) == case["sha"], "the seeded inputs drifted from the ones the fixture was generated with"
    labels = []
    for s, stride in enumerate(LC.STRIDES):
        y = np.zeros((case["n"], case["hw"][0] // stride, case["hw"][1] // stride, 3, 5 + case["ncls"]), dtype=np.float32)
        y.reshape(-1)[fx[f"label{s}_idx"]] = fx[f"label{s}_val"]
        labels.append(y)
    return case, fx, labels


@pytest.mark.parametrize("name", NAMES)
def test_case_holds_what_it_is_there_for(name):
    c = LC.LABEL_CASES[name]
    assert name == f"mb{c['max_boxes']}_c{c['ncls']}" and c["n"] == 4 and c["hw"] == (160, 160)
    facts = LC.check_case(name)
    print(name, facts)
    assert facts["valid"][1] == c["max_boxes"]


def test_the_old_cases_keep_their_inputs():
    assert sorted(LC.CASES) == sorted(OLD_SHA)
    for name, sha in OLD_SHA.items():
        case, fx, _ = load_fixture(name)
        assert case["sha"] == sha == str(fx["sha"])
        assert case["boxes"].shape == (4, LC.MAX_BOXES, 5)


@pytest.mark.parametrize("name", NAMES)
def test_host_records_equal_the_reference_assignment(name):
    from yolo4hip.data import dense_from_records, pad_records, preprocess_true_boxes, record_words, records_from_dense
    case, fx, labels = label_fixture(name)
    mb, ncls = case["max_boxes"], case["ncls"]
    assert case["true_xywh"].dtype == np.float32 and np.array_equal(case["true_xywh"], fx["true_xywh"])
    assert fx["true_xywh"].shape == (case["n"], mb, 4)
    recs = records_from_dense(labels, ncls)
    for a, b in zip(recs, case["records"]):
        assert a.dtype == np.int32 and a.shape[1] == record_words(ncls) == 8 + (ncls + 31) // 32 and np.array_equal(a, b)
        keys = [tuple(r[0:4]) for r in a]
        assert keys == sorted(set(keys))
    for y, ref in zip(dense_from_records(case["records"], case["hw"], ncls), labels):
        assert np.array_equal(y, ref)
    y_true, xywh = preprocess_true_boxes(case["boxes"], case["hw"], LC.ANCHORS, ncls)
    assert np.array_equal(xywh, fx["true_xywh"]) and all(np.array_equal(y, ref) for y, ref in zip(y_true, labels))
    padded, counts = pad_records(case["records"], mb, ncls)
    assert padded.shape == (case["n"], mb, record_words(ncls)) and counts.tolist() == [len(r) for r in case["records"]]
    assert os.path.getsize(os.path.join(GOLDEN, f"loss_{name}.npz")) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_the_oracles_run_on_the_case(name):
    case, fx, labels = label_fixture(name)
    hw, ncls = case["hw"], case["ncls"]
    terms = LO.loss_terms(case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, ncls, LC.IOU_LOSS_THRESH, hw)
    # the rule of test_loss_cpu: float32 results of sums of float32 terms, 2e-6 relative is ~16 ulp
    assert LO.rel_dist(fx["ref_img"], terms).max() < 2e-6
    assert np.array_equal(LO.rel_dist(fx["ref_img"], terms).max(axis=0), fx["d_ref"])
    assert LO.rel_dist(fx["ref_batch"], terms.mean(axis=0)).max() < 2e-6
    assert abs(LO.total(terms) - float(fx["ref_total"])) < 2e-6 * float(fx["ref_total"])
    assert np.all(terms[0, :, 0] == 0) and np.all(terms[0, :, 2] == 0) and np.all(terms[0, :, 1] > 0)   # the image without boxes
    assert np.all(fx["ignore_count"] > 0)
    # the gradient: float64, and the float32 evaluation the GPU test takes its budget from -- round-off, so that 4 x d_ref is no
    # vacuous budget (the bound of test_lossgrad_cpu for heads of order 1)
    w = np.array([0.4, 0.1, 0.3, 0.2])
    g64 = GO.loss_grad(case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, ncls, LC.IOU_LOSS_THRESH, hw, img_weight=w)
    g32 = GO.loss_grad(case["heads"], labels, fx["true_xywh"], LC.ANCHORS, LC.STRIDES, ncls, LC.IOU_LOSS_THRESH, hw, img_weight=w,
                       dtype=np.float32)
    for s in range(3):
        assert g64[s].shape == case["heads"][s].shape and g64[s].dtype == np.float64 and g32[s].dtype == np.float32
        assert np.isfinite(g64[s]).all() and np.abs(g64[s]).max() > 0
        d = GO.rel_to_max(g32[s], g64[s])
        print(name, "scale", s, "float32 evaluation of the gradient oracle:", d)
        assert 1e-8 < d < 1e-6
        # outside the confidence columns only responsible lanes carry a gradient, and a class logit's sign is its label's
        g = g64[s].reshape(labels[s].shape)
        rest = g.copy()
        rest[..., 4] = 0
        assert not rest[labels[s][..., 4] == 0].any()
        on = labels[s][..., 4] == 1
        assert np.all(g[on][:, 5:][labels[s][on][:, 5:] == 1] < 0) and np.all(g[on][:, 5:][labels[s][on][:, 5:] == 0] > 0)
        # a float64 central difference on a class logit of every class id the case is there for
        heads = [h.astype(np.float64) for h in case["heads"]]
        sh = labels[s].shape
        for cls in set(LC.LABEL_CASES[name]["classes"]) | set(LC.LABEL_CASES[name].get("trio", ())):
            lanes = np.argwhere(on & (labels[s][..., 5 + cls] == 1))
            for lane in lanes[:1]:
                idx = tuple(lane) + (5 + cls,)
                b = idx[0]

                def objective():
                    t = LO.scale_terms(heads[s][b:b + 1], labels[s][b:b + 1], fx["true_xywh"][b:b + 1], LC.ANCHORS.reshape(3, 3, 2)[s],
                                       LC.STRIDES[s], ncls, LC.IOU_LOSS_THRESH, float(hw[0] * hw[1]))[0]
                    return float((t[0] * np.array(LO.WEIGHTS)).sum() * w[b])
                flat = heads[s].reshape(sh)
                keep = flat[idx]
                flat[idx] = keep + 1e-6
                up = objective()
                flat[idx] = keep - 1e-6
                down = objective()
                flat[idx] = keep
                fd, an = (up - down) / 2e-6, g[idx]
                assert abs(fd - an) <= 1e-5 * max(abs(an), abs(fd)) + 4 * np.finfo(np.float64).eps * abs(up) / 2e-6, (name, s, idx, fd, an)


def test_the_table_reaches_every_path():
    seen = set()
    assert sorted(REACHES) == sorted(NAMES)
    for name in NAMES:
        case = LC.make_label_case(name)
        hit = reached(case["max_boxes"], case["ncls"], case["boxes"], case["records"])
        print(name, sorted(hit))
        assert hit <= PATHS and set(REACHES[name]) <= hit, (name, set(REACHES[name]) - hit)
        seen |= set(REACHES[name])
    assert seen == PATHS
    # the head convs' cout and the head channel stride the cases bring: 3 (5 + C)
    assert sorted(3 * (5 + c["ncls"]) for c in LC.LABEL_CASES.values()) == [18, 111, 114, 207, 210]
    # every size at which the row count changes the number of waves is there: 1, a full wave, one more, two waves and one, four waves
    assert [c["max_boxes"] for c in LC.LABEL_CASES.values()] == [1, LC.WAVE, LC.WAVE + 1, 2 * LC.WAVE + 1, ROUND]


def test_the_old_geometry_reaches_none_of_them_but_bit_31():
    """max_boxes = 100 with 3 and 80 classes: what every GPU test of the label path ran at before"""
    from yolo4hip.data import records_from_boxes
    for name, c in LC.CASES.items():
        case = LC.make_case(name)
        recs, _ = records_from_boxes(case["boxes"], case["hw"], LC.ANCHORS, case["ncls"])
        hit = reached(LC.MAX_BOXES, case["ncls"], case["boxes"], recs, case["hw"])
        assert hit & PATHS <= {"bit_31_set"}, (name, hit & PATHS)
