"""The activation workspace's layout, held on the host (no GPU): y4_workspace_map / y4_conv_output_view over every size, class
count, batch, dtype, aliasing switch and retention level the suite and the benchmark use.

The map's own shape: rows sorted, ZERO / TAIL / SCRATCH rows pairwise disjoint, every ACT row between the zero page and the first
TAIL row, [0, act_bytes) covered up to alignment gaps, per-image rows of max_batch images.

The aliased layout's SAFETY PROPERTY, stated from the graph of yolo4hip/plan.py (the separate restatement of the reference that
tests/test_gpu_forward.py::test_plan_matches_python_plan pins to the library) and not from the library's own lifetimes: for every
edge producer conv i -> consumer conv j (conv inputs, residual operands, the SPP input, concat slices, upsampled tensors) and every
conv k that executes strictly between them, the memory conv k stores into must not overlap the memory of conv i's output -- unless
both are channel slices of ONE row, which must then be disjoint channel ranges.  Memory of an output = the whole ACT row it lives
in: rows are what the layout places.  The raw heads overlap nothing stored after them; at retention >= 1 neither do the head convs'
inputs (convs 92 / 100 / 108), at retention 2 neither do the inputs of those convs (convs 91 / 99 / 107).

The ZERO regions are bounded: nothing may be declared library-zeroed to make a poisoned-workspace GPU test pass.
"""
import ctypes as C
import itertools

import pytest

SIZES = ((96, 96), (96, 160), (416, 416), (608, 608))
HEADS = (93, 101, 109)
ZERO_BUDGET = lambda nb: 32 * 1024 + 256 * nb


def _edges():
    """(producer conv, consumer conv) pairs of the plan's graph; the stored tensor of add(x, conv) is that conv's output"""
    from yolo4hip.plan import build_plan
    plan = build_plan(96, 3)
    stored = {"input": set()}          # tensor name -> convs whose outputs hold it
    edges = set()
    for op in plan.ops:
        if op.kind == "conv":
            edges |= {(i, op.conv) for i in stored[op.srcs[0]]}
            stored[op.dst] = {op.conv}
        elif op.kind == "add":         # (x, y = 3x3 conv): the conv's epilogue reads x and stores the sum as its own output
            x, y = op.srcs
            (conv,) = stored[y]
            edges |= {(i, conv) for i in stored[x]}
            stored[op.dst] = {conv}
        elif op.kind == "concat":
            stored[op.dst] = set().union(*(stored[s] for s in op.srcs))
        else:                          # maxpool / upsample: stored by (or beside) the conv that produced the source
            assert op.kind in ("maxpool", "upsample"), op.kind
            stored[op.dst] = set(stored[op.srcs[0]])
    assert len(edges) >= 130 and (74, 75) in edges and (58, 79) in edges and (77, 103) in edges and (3, 5) in edges, len(edges)
    return sorted(edges)


EDGES = _edges()


def _handle(lib, hw, ncls, nb, dtype, alias, retain):
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    cfg = _cfg_struct(make_config(hw), ncls, nb, dtype)
    h = C.c_void_p()
    ext.check(lib.y4_create_hw(C.byref(cfg), hw[0], hw[1], C.byref(h)))
    if alias:
        ext.check(lib.y4_set_workspace_aliasing(h, 1))
    if retain:
        ext.check(lib.y4_set_retain_head_inputs(h, retain))
    return h


def _overlap(a, b):
    return a["offset"] < b["offset"] + b["bytes"] and b["offset"] < a["offset"] + a["bytes"]


def _check(lib, hw, ncls, nb, dtype, alias, retain):
    from yolo4hip import ext
    tag = (hw, ncls, nb, dtype, alias, retain)
    h = _handle(lib, hw, ncls, nb, dtype, alias, retain)
    try:
        rows = ext.workspace_map(lib, h)
        a, w = C.c_size_t(), C.c_size_t()
        ext.check(lib.y4_workspace_bytes(h, C.byref(a), C.byref(w)))
        act_bytes = a.value
        views = [ext.conv_output_view(lib, h, i) for i in range(110)]
        layers = []
        for i in range(110):
            d = ext.y4_layer_desc()
            ext.check(lib.y4_layer_info(h, i, C.byref(d)))
            layers.append(d.cout)
    finally:
        lib.y4_destroy(h)
    # ---- the map itself
    assert [(r["offset"], -r["bytes"]) for r in rows] == sorted((r["offset"], -r["bytes"]) for r in rows), tag
    assert all(r["bytes"] > 0 and r["offset"] + r["bytes"] <= act_bytes for r in rows), tag
    assert len({r["name"] for r in rows}) == len(rows), tag
    fixed = [r for r in rows if r["kind"] != "act"]
    for x, y in itertools.combinations(fixed, 2):
        assert not _overlap(x, y), (tag, x, y)
    acts = [r for r in rows if r["kind"] == "act"]
    zero_page = rows[0]
    assert zero_page["kind"] == "zero" and zero_page["offset"] == 0 and zero_page["name"] == "zero_page", tag
    first_tail = min(r["offset"] for r in rows if r["kind"] == "tail")
    for r in acts:
        assert zero_page["bytes"] <= r["offset"] and r["offset"] + r["bytes"] <= first_tail, (tag, r)
        assert 0 <= r["first_op"] <= r["last_op"], (tag, r)
    covered = 0                                            # the rows cover [0, act_bytes): no hole of 256 bytes or more
    for r in rows:
        assert r["offset"] - covered <= 255, (tag, r, covered)
        covered = max(covered, r["offset"] + r["bytes"])
    assert 0 <= act_bytes - covered <= 255, (tag, covered, act_bytes)
    for r in rows:
        if r["image_bytes"]:
            assert r["bytes"] == nb * r["image_bytes"], (tag, r)
    assert all(r["image_bytes"] > 0 for r in acts), tag
    assert {r["name"] for r in rows if r["kind"] == "tail" and r["image_bytes"]} == {"boxes", "keys", "objectness"}, tag
    assert {r["name"] for r in rows if r["kind"] == "zero"} == {"zero_page", "counts", "status", "splitk_counters"}, tag
    assert [r["name"] for r in rows if r["kind"] == "scratch"] == ["splitk_partials"], tag
    # **Condition**: what the library itself keeps zero stays small
    zero_bytes = sum(r["bytes"] for r in rows if r["kind"] == "zero")
    assert zero_bytes <= ZERO_BUDGET(nb), (tag, zero_bytes)
    assert zero_bytes == 256 + 256 * nb + 256 + 16384, (tag, zero_bytes)
    # ---- every conv's view: an ACT row wide enough for it, the heads float32
    es = {"f32": 4, "bf16": 2, "f16": 2}[dtype]
    for i, (ri, coff, cstride, stored) in enumerate(views):
        r = rows[ri]
        assert r["kind"] == "act" and 0 <= coff and coff + layers[i] <= cstride, (tag, i, r, coff, cstride)
        assert r["image_bytes"] % (cstride * (4 if i in HEADS else es)) == 0, (tag, i, r, cstride)
        assert stored, (tag, i)                            # no fusion switch is on

    def clash(i, k):
        """does what conv k stores overlap what conv i stored?"""
        (ri, ci), (rk, ck) = views[i][:2], views[k][:2]
        if ri == rk:                                       # channel slices of one row: disjoint channel ranges
            return ci < ck + layers[k] and ck < ci + layers[i]
        return _overlap(rows[ri], rows[rk])

    if not alias:
        for x, y in itertools.combinations(acts, 2):
            assert not _overlap(x, y), (tag, x, y)
    # ---- the safety property (with aliasing off it follows from the rows being disjoint: checked all the same)
    for i, j in EDGES:
        for k in range(i + 1, j):
            assert not clash(i, k), f"{tag}: conv {k} stores over conv {i}'s output, which conv {j} still reads"
    keep = list(HEADS)
    if retain >= 1:
        keep += [92, 100, 108]
    if retain == 2:
        keep += [91, 99, 107]
    for i in keep:
        for k in range(i + 1, 110):
            assert not clash(i, k), f"{tag}: conv {k} stores over conv {i}'s output, which outlives the forward"
    return len(rows)


@pytest.mark.parametrize("hw", SIZES, ids=lambda hw: f"{hw[0]}x{hw[1]}")
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_workspace_map_and_aliasing_safety(hw, dtype):
    from yolo4hip import ext
    lib = ext.load()
    n = 0
    for ncls, nb, alias, retain in itertools.product((3, 80), (1, 5, 32), (0, 1), (0, 1, 2)):
        n += _check(lib, hw, ncls, nb, dtype, alias, retain) > 0
    assert n == 36


def test_aliasing_shares_bytes_and_the_check_can_fail():
    """Non-vacuity: the aliased layout really does put ACT rows on top of each other (so the safety property has something to
    hold), and `clash` semantics catch an overlap: two rows that share bytes are told apart from two that do not."""
    from yolo4hip import ext
    lib = ext.load()
    h = _handle(lib, (416, 416), 80, 5, "bf16", 1, 0)
    rows = ext.workspace_map(lib, h)
    views = [ext.conv_output_view(lib, h, i) for i in range(110)]
    lib.y4_destroy(h)
    acts = [r for r in rows if r["kind"] == "act"]
    shared = [(x["name"], y["name"]) for x, y in itertools.combinations(acts, 2) if _overlap(x, y)]
    assert len(shared) > 50, len(shared)
    for x, y in itertools.combinations(acts, 2):           # rows that share bytes were never alive together
        if _overlap(x, y):
            assert x["last_op"] < y["first_op"] or y["last_op"] < x["first_op"], (x, y)
    # some pair of convs far apart in the graph lands on shared bytes: the property above is not trivially true
    assert any(views[i][0] != views[k][0] and _overlap(rows[views[i][0]], rows[views[k][0]])
               for i in range(0, 40) for k in range(60, 110))


def test_workspace_map_argument_checks():
    from yolo4hip import ext
    lib = ext.load()
    h = _handle(lib, (96, 96), 3, 2, "f16", 0, 0)
    count = C.c_int()
    assert lib.y4_workspace_map(h, None, 0, None) == -22
    assert lib.y4_workspace_map(h, None, 4, C.byref(count)) == -22
    assert lib.y4_workspace_map(h, None, 0, C.byref(count)) == 0 and count.value > 80
    two = (ext.y4_workspace_row * 2)()
    assert lib.y4_workspace_map(h, two, 2, C.byref(count)) == 0 and two[0].name == b"zero_page" and two[1].kind == ext.WS_ACT
    r, c, s = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.y4_conv_output_view(h, 110, C.byref(r), C.byref(c), C.byref(s), None) == -22
    assert lib.y4_conv_output_view(h, 0, None, C.byref(c), C.byref(s), None) == -22
    assert lib.y4_conv_output_view(h, 8, C.byref(r), C.byref(c), C.byref(s), None) == 0
    # which convs a forward writes, under every fusion (host state): the taps tests/test_gpu_forward.py names as still written are,
    # conv 0, convs 2 .. 6, the residual blocks' 1x1 convs and the convs inside a run are not
    assert all(ext.conv_output_view(lib, h, i)[3] for i in range(110))
    assert lib.y4_set_chain_fusion(h, 1) == 26
    kept = {i for i in range(110) if not ext.conv_output_view(lib, h, i)[3]}
    assert kept == {5, 6, 8, 14, 15, 17, 35, 56, 88, 90, 92}, sorted(kept)
    assert lib.y4_set_stem_fusion(h, 1) == 0 and lib.y4_set_stage_fusion(h, 1) == 1 and lib.y4_set_res_fusion(h, 1) == 10
    kept = {i for i in range(110) if not ext.conv_output_view(lib, h, i)[3]}
    assert {0, 2, 3, 4, 5, 6, 8, 11, 13, 15, 17, 20, 34, 88, 90, 92} <= kept and not kept & {1, 7, 12, 14, 16, 21, 35, 36, 37, 93}, sorted(kept)
    assert C.sizeof(ext.y4_workspace_row) == 64
    lib.y4_destroy(h)
