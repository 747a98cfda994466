"""yolo4hip/schedule.py (the tile-entry codec) and the handle's `Schedule` (csrc/runtime.hip), host only: entries decode as the
library encodes them, the halo2 / split-K questions agree with the shipped files and with the library's tile table, and
y4_copy_schedule / y4_autotune_pair copy and compare every scheduling choice."""
import ctypes as C
import glob
import json
import os

import pytest

from helpers import ROOT


def _lib():
    from yolo4hip import ext
    return ext.load()


def _shipped():
    files = sorted(glob.glob(os.path.join(ROOT, "yolo-v4-tf.keras_amd", "yolo4hip", "schedules", "*.json")))
    assert len(files) >= 7
    return [(os.path.basename(f), json.load(open(f))) for f in files]


def _families(lib):
    from yolo4hip import ext
    out = {}
    for t in range(1, lib.y4_conv_tile_count() + 1):
        cfg = (C.c_int32 * 6)()
        ext.check(lib.y4_conv_tile_desc(t, cfg))
        out[t] = cfg[5]
    return out


def test_decode_encode_base_split():
    from yolo4hip import schedule as S
    assert [S.decode(e) for e in (0, 7, 207, -5, -(5 + 1000 * 61), -(5 + 1000 * 207))] == \
        [(0, 0), (0, 7), (0, 207), (5, 0), (5, 61), (5, 207)]
    for run, own in ((5, 0), (5, 61), (0, 7), (5, 207), (62, 362)):
        assert S.decode(S.encode(run, own)) == (run, own)
    assert [(S.base(t), S.split(t)) for t in (0, 7, 61, 107, 207, 362)] == [(0, 0), (7, 0), (61, 0), (7, 1), (7, 2), (62, 3)]


def test_uses_halo2_is_the_librarys_family_21_in_either_half():
    from yolo4hip import schedule as S
    lib = _lib()
    fam = _families(lib)
    h2 = sorted(t for t, f in fam.items() if f == S.HALO2)
    assert h2 and h2 == list(range(h2[0], h2[-1] + 1))              # today one contiguous block of ids at the table's end
    assert S.family(lib, 0) is None and all(S.family(lib, t) == f and S.family(lib, t + 200) == f for t, f in fam.items())
    plain = next(t for t, f in fam.items() if f != S.HALO2)
    for t in fam:
        want = t in h2
        assert S.uses_halo2(lib, [t]) == want                               # a plain entry
        assert S.uses_halo2(lib, [plain, S.encode(plain, t)]) == want       # the stand-alone half of a run head's entry
        assert S.uses_halo2(lib, [0, S.encode(t, plain), plain]) == want    # its run half
        assert S.uses_halo2(lib, [S.encode(0, t)]) == want                  # (chained with the heuristic tile)
    assert not S.uses_halo2(lib, []) and not S.uses_halo2(lib, [0, plain, -plain])


def test_flags_of_the_shipped_schedules():
    from yolo4hip import schedule as S
    lib = _lib()
    for name, s in _shipped():
        assert S.uses_halo2(lib, s["tiles"]) == bool(s.get("halo2")), name
        assert S.uses_splitk(s["tiles"]) == bool(s.get("splitk")), name
    assert S.uses_splitk([0, 5, -(5 + 1000 * 207)]) and S.uses_splitk([107]) and not S.uses_splitk([0, 61, -(5 + 1000 * 61)])


def _handle(lib, nb=4):
    from yolo4hip import ext
    from yolo4hip.config import make_config
    from yolo4hip.engine import _cfg_struct
    cfg = _cfg_struct(make_config(416), 80, nb, "bf16")
    h = C.c_void_p()
    ext.check(lib.y4_create(C.byref(cfg), C.byref(h)))
    return h


def _state(lib, h):
    from yolo4hip import ext
    tiles = (C.c_int32 * 110)()
    ext.check(lib.y4_get_tiles(h, tiles, 110))
    convs, total = C.c_int32(), C.c_int32()
    ext.check(lib.y4_launch_counts(h, C.byref(convs), C.byref(total)))
    return list(tiles), lib.y4_get_stage_fusion(h), lib.y4_get_res_fusion(h), (convs.value, total.value)


def test_copy_schedule_copies_and_autotune_pair_compares_every_choice():
    """h: every switch on, sub-batches of 2 up to conv 16, residual mask 2, one run head with a run tile AND a tile of its own."""
    from yolo4hip import ext, schedule as S
    lib = _lib()
    h, h2 = _handle(lib), _handle(lib)
    ext.check(lib.y4_set_stem_fusion(h, 1))
    assert lib.y4_set_chain_fusion(h, 1) > 0
    assert lib.y4_set_stage_fusion(h, 1) == 1
    assert lib.y4_set_res_fusion(h, 1) > 0
    ext.check(lib.y4_set_res_fusion_mask(h, 2))
    ext.check(lib.y4_set_subbatch(h, 2, 16))
    tiles = _state(lib, h)[0]
    tiles[15] = S.encode(5, 7)                                    # conv 15 heads a run (y4_set_tiles refuses the entry otherwise)
    tiles[100] = 3
    ext.check(lib.y4_set_tiles(h, (C.c_int32 * 110)(*tiles), 110))
    want = _state(lib, h)
    assert want[0] == tiles and want[1:3] == (1, 2)
    assert _state(lib, h2) != want
    ext.check(lib.y4_copy_schedule(h, h2))
    assert _state(lib, h2) == want
    assert lib.y4_set_workspace_aliasing(h2, 1) < 0 and b"sub-batching" in lib.y4_last_error()     # the sub-batch came along

    def pair():
        return lib.y4_autotune_pair(h, h2, 4, 1, None, None, 15), lib.y4_last_error()

    # equal schedules pass the comparison (it comes first); the unbound handles then fail the readiness check
    rc, msg = pair()
    assert rc < 0 and b"workspace not bound" in msg and b"differ" not in msg
    changes = {"stem": lambda: lib.y4_set_stem_fusion(h2, 0), "chain": lambda: lib.y4_set_chain_fusion(h2, 0),
               "stage": lambda: lib.y4_set_stage_fusion(h2, 0), "res": lambda: lib.y4_set_res_fusion(h2, 0),
               "sub-batch images": lambda: lib.y4_set_subbatch(h2, 1, 16), "sub-batch end": lambda: lib.y4_set_subbatch(h2, 2, 7),
               "sub-batch off": lambda: lib.y4_set_subbatch(h2, 0, 16)}
    for what, change in changes.items():
        assert change() >= 0, what
        rc, msg = pair()
        assert rc < 0 and b"differ" in msg, (what, msg)
        ext.check(lib.y4_copy_schedule(h, h2))
        assert _state(lib, h2) == want and b"workspace not bound" in pair()[1], what
    # the tuner's verdicts and the tiles are what a pair run writes: they may differ beforehand
    ext.check(lib.y4_set_res_fusion_mask(h2, 3))
    ext.check(lib.y4_set_tiles(h2, (C.c_int32 * 110)(*([0] * 110)), 110))
    assert b"workspace not bound" in pair()[1]
    # handles of another configuration are no siblings
    other = _handle(lib, nb=2)
    assert lib.y4_copy_schedule(h, other) < 0 and b"same configuration" in lib.y4_last_error()
    for x in (h, h2, other):
        lib.y4_destroy(x)
