"""The tile entries of a schedule, read in one place (host only: no GPU, no torch).

`Engine.get_tiles` / `set_tiles` and the schedule files hold one entry per conv (y4_get_tiles, csrc/runtime.hip: TileEntry).
A plain conv's entry is its tile id, 0 for the library's heuristic.  The head of a fused run carries two ids in one entry,
-(run tile + 1000 * stand-alone tile), while the run executes as one kernel.  A tile id is base + 100 e: base tile `base` with
its K loop split 2^e ways (split-K, e = 0: unsplit).  What kind of kernel a base tile is, its family, is the library's to say:
y4_conv_tile_desc(...)[5].
"""
import ctypes as C
import functools

HALO2 = 21      # family of the halo2 tiles (conv_halo2_kernel.h: v_mfma_32x32x16, another fixed fp32 summation order)


def decode(entry):
    """entry -> (run tile, stand-alone tile); a plain entry has run tile 0."""
    e = int(entry)
    return ((-e) % 1000, (-e) // 1000) if e < 0 else (0, e)


def encode(run_tile, own_tile):
    """The entry of a run head that executes chained with `run_tile` and keeps `own_tile` for when it does not."""
    return -(int(run_tile) + 1000 * int(own_tile))


def base(tile):
    return int(tile) % 100


def split(tile):
    return int(tile) // 100


@functools.lru_cache(maxsize=None)
def family(lib, tile):
    """Family code of tile id `tile` (its split-K part ignored); None for 0, the heuristic."""
    from . import ext
    if base(tile) == 0:
        return None
    cfg = (C.c_int32 * 6)()
    ext.check(lib.y4_conv_tile_desc(base(tile), cfg))
    return cfg[5]


def _ids(tiles):
    return (t for e in tiles for t in decode(e))


def uses_halo2(lib, tiles):
    """Does either half of any entry name a halo2 tile?"""
    return any(family(lib, t) == HALO2 for t in _ids(tiles))


def uses_splitk(tiles):
    """Does either half of any entry name a split-K id?"""
    return any(split(t) > 0 for t in _ids(tiles))


def describe(engine):
    """The schedule `engine` runs now, as the dict the schedule files hold and `Engine.apply_schedule` takes.  `"splitk"` and
    `"halo2"` say whether the ids change the fp32 summation order: they are derived from the ids alone."""
    tiles = engine.get_tiles()
    fused = engine.dtype != "f32"
    return {"size": engine.img_size if isinstance(engine.img_size, int) else list(engine.img_size),
            "classes": engine.num_classes, "batch": engine.max_batch, "dtype": engine.dtype, "tiles": tiles,
            "stage_fusion": bool(engine.stage_fusion_active()) if fused else False,
            "res_fusion_mask": int(engine.res_fusion_mask()) if fused else 0, "in_flight": 1,
            "splitk": uses_splitk(tiles), "halo2": uses_halo2(engine.lib, tiles)}
