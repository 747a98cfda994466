"""Retention level 2 of y4_set_retain_head_inputs (what y4_block_grad needs) leaves levels 0 and 1 where they were.  The workspace
layout is pure host work (liveness over the plan, interval placement), so this runs without a GPU.

PINNED holds y4_workspace_bytes of the commit before level 2 existed, taken from a library built from that commit: the numbers
are arithmetic on the plan, the same on every machine."""
import ctypes as C

import pytest

# (size, classes, max_batch, dtype) -> ((act, wts) with aliasing and no retention, the same with y4_set_retain_head_inputs(h, 1))
PINNED = {
    (160, 3, 2, "bf16"): ((44370176, 225353728), (44370176, 225353728)),
    (608, 80, 32, "bf16"): ((2975455488, 225815552), (2975455488, 225815552)),
    (416, 80, 2, "f32"): ((147340288, 261969920), (147340288, 261969920)),
}


def _sizes(lib, ext, cfg, calls):
    h = C.c_void_p()
    ext.check(lib.y4_create(C.byref(cfg), C.byref(h)))
    ext.check(lib.y4_set_workspace_aliasing(h, 1))
    for level in calls:
        ext.check(lib.y4_set_retain_head_inputs(h, level))
    a, w = C.c_size_t(), C.c_size_t()
    ext.check(lib.y4_workspace_bytes(h, C.byref(a), C.byref(w)))
    lib.y4_destroy(h)
    return a.value, w.value


@pytest.mark.parametrize("shape", sorted(PINNED))
def test_levels_0_and_1_keep_their_workspace(shape):
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    lib = ext.load()
    size, ncls, nb, dt = shape
    cfg = _cfg_struct(make_config(size), ncls, nb, dt)
    off, on = PINNED[shape]
    assert _sizes(lib, ext, cfg, ()) == off                       # the setter never called
    assert _sizes(lib, ext, cfg, (0,)) == off
    assert _sizes(lib, ext, cfg, (1,)) == on
    assert _sizes(lib, ext, cfg, (3,)) == on                      # any other non-zero value is level 1, as it always was
    # level 2 leaves nothing behind when it is taken back, and costs activation memory only
    assert _sizes(lib, ext, cfg, (2, 0)) == off
    assert _sizes(lib, ext, cfg, (2, 1)) == on
    two = _sizes(lib, ext, cfg, (2,))
    assert two[0] >= on[0] and two[1] == on[1]
    assert _sizes(lib, ext, cfg, (1, 2)) == two
