"""Inputs for the decode + NMS tests, each with a WITNESS that it reaches the code path it is meant for (NumPy only; the GPU is
touched by `_engine` / `_compare` alone, which import it when called).

Which of decode_nms.hip's kernels, selectors, sorts and greedy passes runs cannot be observed from outside, and the library has no
knob or counter for it.  The witnesses are therefore properties of the INPUT, computed from the oracle alone
(tests/test_decode_nms_cases_cpu.py asserts them without a GPU; tests/test_gpu_decode_nms_paths.py then holds the kernels to the
oracle on the same inputs):

  * `candidate_order` is an image's candidates in the order both sides define (score desc, box index asc, class asc) and
    `rank_of_last_kept` the position in it of the last box the oracle kept: the greedy rule is sequential in that order, so no
    implementation can return the oracle's answer without having visited that many candidates;
  * the chunk bounds below say, from the candidate count alone, how many keys each chunk of the NMS kernel can hold;
  * `wave_flushes` replays which 16-cell groups of the cell decode fill their staging slice or cross an image boundary.

The literals are the kernel's constants (decode_nms.hip), restated: a change there must be made here by hand, and the CPU tests
then say which cases no longer pin their path."""
import functools

import numpy as np

NMS_THREADS = 1024      # decode_nms.hip NMS_THREADS: keys in the first chunk, at most
SORT_CAP = 4096         # decode_nms.hip SORT_CAP: keys in a later chunk, at most
PAR_MAX_C = 1024        # decode_nms.hip PAR_MAX_C: class count up to which the first chunk is decided round-parallel
DC_STAGE = 512          # decode_nms.hip DC_STAGE: keys a wave stages before it must flush
DC_SCREEN = 16          # decode_nms.hip DC_SCREEN: cells per wave of the large variant
DC_SCREEN_MIN_WAVES = 8192   # decode_launch: the 16-cell variant runs once N * cells_per_img >= DC_SCREEN * 8192
CELL_KERNEL_MAX_VALUES = 256  # decode_launch: 3 * (5 + C) <= 256 takes the cell kernels, more the generic decode_kernel


# ------------------------------------------------------------------------------------------------ engine and comparison
def _engine(size, ncls, n, **caps):
    """A bare engine (decode / NMS read no weights).  size: side, or (H, W); caps: max_per_class / max_total."""
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    cfg = make_config(size)
    eng = Engine(ncls, cfg, max_batch=n, dtype="bf16", **caps)
    eng.adopt_packed()          # decode/NMS do not read weights
    return cfg, eng


def boxes_and_scores(heads, ncls, cfg, size):
    """The oracle's decode: boxes [n, nbox, 4] (normalised), scores [n, nbox, C]."""
    from oracle import decode_nms as OD
    head = OD.yolov4_head(heads, ncls, cfg["anchors"], cfg["xyscale"])
    return OD.flatten_for_nms(head, size, ncls)


def reference(heads, ncls, cfg, size, iou=-1.0, score=-1.0, per_class=100, total=100):
    """The oracle on raw heads with the two caps explicit (oracle.decode_nms.inference_from_heads fixes per_class at 100)."""
    from oracle import decode_nms as OD
    with np.errstate(over="ignore", invalid="ignore"):
        b, s = boxes_and_scores(heads, ncls, cfg, size)
        return OD.combined_nms(b, s, per_class, total, cfg["iou_threshold"] if iou < 0 else iou,
                               cfg["score_threshold"] if score < 0 else score)


def assert_same_detections(got, ref):
    """The project's bars: decisions identical, boxes within 1e-5, scores within 1e-6."""
    assert np.array_equal(got[3], ref[3]), (got[3], ref[3])
    assert np.array_equal(got[4], ref[4])
    assert np.array_equal(got[2], ref[2])
    assert np.abs(got[0] - ref[0]).max() < 1e-5
    assert np.abs(got[1] - ref[1]).max() < 1e-6


def _compare(eng, cfg, heads, size, ncls, iou=-1.0, score=-1.0, per_class=100, total=100, ref=None):
    """Decode + NMS of `heads` on the engine against the oracle (`ref`: its outputs when the caller has them already)."""
    n = eng.set_heads(heads)
    got = [o.cpu().numpy() for o in eng.decode_nms_device(n, None, iou, score)]
    if ref is None:
        ref = reference(heads, ncls, cfg, size, iou, score, per_class, total)
    assert_same_detections(got, ref)
    return got, ref


# ------------------------------------------------------------------------------------------------ generators
def _random_heads(rng, n, size, ncls, obj_bias, cls_bias, gain=1.5):
    heads = []
    nf = 5 + ncls
    for s in (8, 16, 32):
        g = size // s
        h = (rng.standard_normal((n, g, g, 3, nf)) * gain).astype(np.float32)
        h[..., 2:4] *= 0.3
        h[..., 4] += obj_bias
        h[..., 5:] += cls_bias
        heads.append(h.reshape(n, g, g, 3 * nf))
    return heads


def _heads_with(size, ncls, n, boxes):
    """Logits that are hugely negative everywhere except the listed (image, scale, gy, gx, anchor, class, obj_logit, cls_logit,
    txywh) cells: exactly those boxes are candidates."""
    nf = 5 + ncls
    heads = [np.full((n, size // s, size // s, 3, nf), -20.0, np.float32) for s in (8, 16, 32)]
    for h in heads:
        h[..., :4] = 0.0
    for (b, sc, gy, gx, a, c, lo, lc, t) in boxes:
        heads[sc][b, gy, gx, a, :4] = t
        heads[sc][b, gy, gx, a, 4] = lo
        heads[sc][b, gy, gx, a, 5 + c] = lc
    return [h.reshape(n, h.shape[1], h.shape[2], 3 * nf) for h in heads]


def stack_boxes(size, n_stack, seed, image=0, ncls=2, stack_cls=0, disjoint_cls=1, n_disjoint=0):
    """The box list of `stack_and_disjoint` for one image of a batch (see there)."""
    g = size // 8
    rng = np.random.default_rng(seed)
    slots = [(gy, gx, a) for gy in range(g) for gx in range(g) for a in (1, 2)]
    assert n_stack <= len(slots) and n_disjoint <= g * g
    boxes = []
    for gy, gx, a in slots[:n_stack]:
        boxes.append((image, 0, gy, gx, a, stack_cls, 8.0, float(rng.uniform(0.0, 3.0)), (0.0, 0.0, 6.0, 6.0)))
    pick = rng.permutation(g * g)[:n_disjoint]
    for j, ci in enumerate(pick):
        lc = 5.0 + 0.01 * j if j % 3 == 0 else -0.5 - 0.002 * j
        boxes.append((image, 0, int(ci) // g, int(ci) % g, 0, disjoint_cls, 8.0, lc, (0.0, 0.0, -1.0, -1.0)))
    return boxes


def stack_and_disjoint(size, n_stack, n_disjoint, seed, ncls=2, stack_cls=0, disjoint_cls=1):
    """One image whose NMS must walk past a long run of suppressed candidates before it has its max_total boxes.

    The STACK: `n_stack` boxes of class `stack_cls` on the stride-8 cells in row-major order, anchors 1 and 2, t_wh = 6 (some
    400 times the anchor: each covers the whole image after the clip, any two overlap with IoU > 0.7), objectness logit 8, class
    logits uniform in [0, 3]: the best one suppresses every other.  The DISJOINT part: `n_disjoint` boxes of class `disjoint_cls`
    on anchor 0 of distinct random stride-8 cells with t_wh = -1 (a 4 x 6 pixel box in an 8 x 8 cell: no two overlap); every
    third one scores above the whole stack (class logit 5 + 0.01 j), the others below it (-0.5 - 0.002 j).  In the candidate
    order the stack thus lies BETWEEN kept boxes: the kept list is complete only after the last stack box has been visited."""
    return _heads_with(size, ncls, 1, stack_boxes(size, n_stack, seed, 0, ncls, stack_cls, disjoint_cls, n_disjoint))


def grid_of_equal_boxes(size, ncls, cls, lo=6.0, lc=3.0):
    """Anchor 0 of EVERY stride-8 cell, t_wh = -1, one class, one score: (size / 8)^2 disjoint candidates that tie; the order is
    the box index alone."""
    g = size // 8
    return _heads_with(size, ncls, 1, [(0, 0, gy, gx, 0, cls, lo, lc, (0.0, 0.0, -1.0, -1.0)) for gy in range(g) for gx in range(g)])


# ------------------------------------------------------------------------------------------------ witnesses
def candidate_order(scores, score_thr):
    """scores [nbox, C] of one image -> int array [T, 2] of (box, class), the candidates (score > threshold, strict) in the
    defined global order: score desc, box index asc, class asc."""
    sc = np.asarray(scores, np.float32)
    bi, ci = np.nonzero(sc > np.float32(score_thr))
    order = np.lexsort((ci, bi, -sc[bi, ci].astype(np.float64)))
    return np.stack([bi[order], ci[order]], axis=1)


def ranks_of_kept(order, kept_idx, classes, valid):
    """Positions in `order` of the oracle's kept boxes of one image (kept_idx [T], classes [T], valid scalar), in output order."""
    where = {(int(b), int(c)): i for i, (b, c) in enumerate(order)}
    return [where[(int(kept_idx[k]), int(classes[k]))] for k in range(int(valid))]


def rank_of_last_kept(order, kept_idx, classes, valid):
    """Position in `order` of the last box the oracle kept (-1 when it kept none)."""
    r = ranks_of_kept(order, kept_idx, classes, valid)
    return r[-1] if r else -1


def first_chunk_bounds(T):
    """(lo, hi) keys in the NMS kernel's first chunk for T candidates: everything when T <= NMS_THREADS; else the histogram pivot
    is accepted only with a suffix of at least half a chunk, and the exact select otherwise takes exactly NMS_THREADS."""
    return (T, T) if T <= NMS_THREADS else (NMS_THREADS // 2, NMS_THREADS)


def second_chunk_bounds(T):
    """(lo, hi) keys that remain for the second chunk."""
    lo, hi = first_chunk_bounds(T)
    return T - hi, T - lo


def chunk_witness(scores, score_thr, ref_img):
    """dict of the figures the chunk cases are judged by, for one image: candidates T, rank of the last kept box, the bounds of
    what remains after the first chunk, and how many boxes are certainly kept before the 64-candidate batch that holds the last
    kept one begins (a batch is 64 consecutive positions, wherever it starts)."""
    order = candidate_order(scores, score_thr)
    kept_idx, classes, valid = ref_img
    ranks = ranks_of_kept(order, kept_idx, classes, valid)
    r = ranks[-1] if ranks else -1
    lo, hi = second_chunk_bounds(len(order))
    return {"T": len(order), "rank": r, "rem_lo": lo, "rem_hi": hi, "valid": int(valid),
            "kept_before_last_batch": sum(1 for x in ranks if x <= r - 64)}


def cell_counts(scores, score_thr, ncls):
    """scores [n, nbox, C] -> candidates per grid cell [n * cells_per_img] in the decode kernels' cell order (image, then the
    cells of scale 0, 1, 2 row-major: box index // 3)."""
    n, nbox, _ = scores.shape
    return (scores > np.float32(score_thr)).reshape(n, nbox // 3, 3 * ncls).sum(axis=2).reshape(-1)


def wave_flushes(counts, cells_per_img, ncls, group=DC_SCREEN):
    """Replays the staging of decode_cell_kernel<group> on per-cell candidate counts: a wave takes `group` consecutive cells and,
    in front of a cell that has candidates to add, writes its staged keys out when the image changes or when the slice could not
    take a full cell (fill + 3 C > DC_STAGE).  Returns per group (slice-full flushes, image-change flushes), counting only flushes
    that had something staged.  (A cell without candidates stages nothing: whether the kernel visits it -- its objectness alone
    may pass -- changes no flush that had something to write, only when it happens.)"""
    out = []
    for g0 in range(0, len(counts), group):
        fill, img, full, change = 0, -1, 0, 0
        for cell in range(g0, min(g0 + group, len(counts))):
            if counts[cell] == 0:
                continue
            n = cell // cells_per_img
            if n != img or fill + 3 * ncls > DC_STAGE:
                if fill:
                    if n != img:
                        change += 1
                    else:
                        full += 1
                fill, img = 0, n
            fill += int(counts[cell])
        out.append((full, change))
    return out


def n16(cells_per_img):
    """The smallest batch that takes the 16-cell decode variant: N * cells_per_img >= DC_SCREEN * 8192."""
    return -(-DC_SCREEN * DC_SCREEN_MIN_WAVES // cells_per_img)


# ------------------------------------------------------------------------------------------------ the cases
SIZE_CHUNK = 416
N_DISJOINT = 160
# name -> (n_stack, n_disjoint): the first four are the measured constructions (candidates 1460 / 2660 / 4660 / 5560, last kept at
# rank 1398 / 2598 / 4598 / 5498); "s4400" leaves at most 4048 keys after ANY first chunk, so its second chunk is the 4096-key
# sort with no select in front; "s2500d200" has 67 disjoint boxes above the stack, so every batch of the later chunk starts from
# a kept list longer than 64
CHUNK_CASES = {"s1300": (1300, N_DISJOINT), "s2500": (2500, N_DISJOINT), "s4500": (4500, N_DISJOINT), "s5400": (5400, N_DISJOINT),
               "s4400": (4400, N_DISJOINT), "s2500d200": (2500, 200)}


@functools.lru_cache(maxsize=None)
def chunk_case(name):
    """-> (heads, boxes, scores) of a CHUNK_CASES image at 416^2, C = 2 (arrays shared by every test: do not write to them)."""
    from yolo4hip.config import make_config
    n_stack, n_dis = CHUNK_CASES[name]
    heads = stack_and_disjoint(SIZE_CHUNK, n_stack, n_dis, seed=n_stack)
    b, s = boxes_and_scores(heads, 2, make_config(SIZE_CHUNK), SIZE_CHUNK)
    return heads, b, s


@functools.lru_cache(maxsize=None)
def chunk_reference(name, per_class=100, total=100):
    from oracle import decode_nms as OD
    from yolo4hip.config import make_config
    cfg = make_config(SIZE_CHUNK)
    _, b, s = chunk_case(name)
    return OD.combined_nms(b, s, per_class, total, cfg["iou_threshold"], cfg["score_threshold"])


# ---- caps.  (max_per_class, max_total, input); the inputs are built by `cap_input`
CAP_PAIRS = [(1, 100), (3, 10), (5, 7), (100, 1), (2, 1024), (1024, 1024)]
CAP_CASES = ([(pc, tot, inp) for pc, tot in CAP_PAIRS for inp in ("small6", "s2500")] +
             [(2, 1024, "dense6"), (1024, 1024, "grid2704")])
# (1024, 1024) on "small6" and "s2500": neither input has 1024 survivors, so no cap can bind there; those two runs check the
# max_total = 1024 layout (LDS carve-up, output stride) and, on s2500, a kept list of 161 boxes -- the witness for them is that
# the result has MORE than 100 boxes (s2500) resp. equals the uncapped one
CAP_CANNOT_BIND = {(1024, 1024, "small6"), (1024, 1024, "s2500")}


@functools.lru_cache(maxsize=None)
def cap_input(name):
    """-> (size, ncls, heads, boxes, scores).  small6: under 1024 candidates (one chunk, the round-parallel pass), all six classes
    crowded and class 0 ahead of the others; s2500: the 2500-stack (the wave-0 pass of a later chunk); dense6: thousands of candidates in every one of six classes;
    grid2704: 2704 disjoint boxes of one class with one score."""
    from yolo4hip.config import make_config
    if name == "small6":
        size, ncls = 160, 6
        heads = _random_heads(np.random.default_rng(66), 1, size, ncls, -0.5, -1.5, gain=1.0)
        for h in heads:                            # class 0 leads: a cap of 3 or 5 shows in the first 10 or 7 results
            h.reshape(h.shape[:3] + (3, 5 + ncls))[..., 5] += 2.5
    elif name == "dense6":
        size, ncls = 224, 6
        heads = _random_heads(np.random.default_rng(67), 1, size, ncls, 3.0, 2.0, gain=0.7)
    elif name == "grid2704":
        size, ncls = 416, 2
        heads = grid_of_equal_boxes(size, ncls, 1)
    else:
        size, ncls = SIZE_CHUNK, 2
        return (size, ncls) + chunk_case(name)
    b, s = boxes_and_scores(heads, ncls, make_config(size), size)
    return size, ncls, heads, b, s


@functools.lru_cache(maxsize=None)
def cap_reference(name, per_class, total):
    """The oracle on a cap input; per_class = total = None: uncapped (every survivor of every class, all of them returned)."""
    from oracle import decode_nms as OD
    from yolo4hip.config import make_config
    size, ncls, _, b, s = cap_input(name)
    cfg = make_config(size)
    if per_class is None:
        per_class = total = int((s > np.float32(cfg["score_threshold"])).sum()) + 1
    return OD.combined_nms(b, s, per_class, total, cfg["iou_threshold"], cfg["score_threshold"])


# ---- the 16-cell decode variant
SIZE_DENSE = 96
CELLS_DENSE = sum((SIZE_DENSE // s) ** 2 for s in (8, 16, 32))       # 144 + 36 + 9 = 189: not a multiple of 16
DENSE_CASES = {80: (-3.0, -3.0), 3: (-2.0, -1.0)}                    # C -> (objectness bias, class bias) of the sparse images


def dense_positions(n):
    return (0, 1, n // 2, n - 1)


@functools.lru_cache(maxsize=None)
def dense_case(ncls):
    """-> (heads, ref, counts): N16 images at 96^2, sparse but for four dense ones (obj +3, cls +2, gain 0.7) at positions 0, 1,
    the middle and the last; the oracle's five outputs; candidates per cell.  Computed once per session (the C = 80 oracle takes
    several seconds)."""
    from yolo4hip.config import make_config
    n = n16(CELLS_DENSE)
    cfg = make_config(SIZE_DENSE)
    ob, cb = DENSE_CASES[ncls]
    rng = np.random.default_rng(1000 + ncls)
    heads = _random_heads(rng, n, SIZE_DENSE, ncls, ob, cb)
    for i in dense_positions(n):
        d = _random_heads(rng, 1, SIZE_DENSE, ncls, 3.0, 2.0, gain=0.7)
        for s in range(3):
            heads[s][i] = d[s][0]
    from oracle import decode_nms as OD
    b, s = boxes_and_scores(heads, ncls, cfg, SIZE_DENSE)
    counts = cell_counts(s, cfg["score_threshold"], ncls)
    ref = OD.combined_nms(b, s, 100, 100, cfg["iou_threshold"], cfg["score_threshold"])
    return heads, ref, counts


# ---- more classes than PAR_MAX_C, and the generic decode kernel
def generic_heads(size, ncls, n, dense_image=1, seed=0):
    """Sparse random heads (obj -2, cls -2.5) with ONE dense image (obj +3, cls +2, gain 0.7).  size: side or (H, W)."""
    H, W = (size, size) if isinstance(size, int) else size
    rng = np.random.default_rng([seed, H, W, ncls])
    nf = 5 + ncls
    heads = []
    for st in (8, 16, 32):
        h = (rng.standard_normal((n, H // st, W // st, 3, nf)) * 1.5).astype(np.float32)
        h[..., 2:4] *= 0.3
        h[..., 4] += -2.0
        h[..., 5:] += -2.5
        d = (rng.standard_normal((H // st, W // st, 3, nf)) * 0.7).astype(np.float32)
        d[..., 2:4] *= 0.3
        d[..., 4] += 3.0
        d[..., 5:] += 2.0
        h[dense_image] = d
        heads.append(h.reshape(n, H // st, W // st, 3 * nf))
    return heads


def many_class_heads(ncls=PAR_MAX_C + 1, size=96):
    """n = 2: image 0 random (obj -2, cls -4: about a thousand candidates per image over 1025 classes), image 1 a
    stack-and-disjoint image with the stack on the LAST class and the disjoint boxes on class 0, so that suppression and order
    matter in a first chunk that C > PAR_MAX_C sends through the wave-0 pass."""
    heads = _random_heads(np.random.default_rng(1025), 2, size, ncls, -2.0, -4.0)
    g = size // 8
    planted = _heads_with(size, ncls, 1, stack_boxes(size, 2 * g * g, 7, 0, ncls, ncls - 1, 0, 100))
    for s in range(3):
        heads[s][1] = planted[s][0]
    return heads


# ---- arithmetic edges
def overflow_heads():
    """96^2, C = 3, n = 1: objectness +1 random heads; wh logits of 95 (expf overflows: inf corners, NaN IoU between two such
    boxes, clipped to (0, 0, 1, 1)) on a 3 x 3 block of stride-8 cells and of -110 (expf underflows to 0: a zero-area box, which
    neither suppresses nor is suppressed) on a 2 x 2 block."""
    heads = _random_heads(np.random.default_rng(3), 1, 96, 3, 1.0, 0.0)
    h0 = heads[0].reshape(1, 12, 12, 3, 8)
    h0[0, 2:5, 2:5, :, 2:4] = 95.0
    h0[0, 7:9, 7:9, :, 2:4] = -110.0
    return heads


# ---- iou_threshold = 0: any overlap suppresses, the kept list never fills and every candidate is visited
SIZE_IOU0 = 224


@functools.lru_cache(maxsize=None)
def iou_zero_case():
    """-> (heads, ref, witness): dense random heads (224^2, C = 3, everything passes) at iou_threshold = 0.0.  On their own they
    fill max_total from the first few hundred candidates (small disjoint boxes), so one stack box (t_wh = 6: it covers the
    image) with the best score of every class is added -- everything of its class overlaps it and is suppressed -- and three
    ZERO-AREA boxes (t_wh = -110) with scores just above the threshold: IoU with them is 0 by definition, so they are kept
    wherever they sit -- and they sit at the very end of the candidate order, behind more than two chunks."""
    from oracle import decode_nms as OD
    from yolo4hip.config import make_config
    size, ncls = SIZE_IOU0, 3
    cfg = make_config(size)
    heads = _random_heads(np.random.default_rng(11), 1, size, ncls, 3.0, 2.0, gain=0.7)
    h0 = heads[0].reshape(1, size // 8, size // 8, 3, 5 + ncls)
    h0[0, 0, 0, 2, :] = (0.0, 0.0, 6.0, 6.0, 12.0, 12.0, 12.0, 12.0)
    for k, (gy, gx) in enumerate([(3, 4), (11, 20), (25, 9)]):
        h0[0, gy, gx, 1, 2:4] = -110.0
        h0[0, gy, gx, 1, 4] = 0.0                 # sigmoid 0.5
        h0[0, gy, gx, 1, 5:] = -20.0
        h0[0, gy, gx, 1, 5 + k] = 0.45 + 0.01 * k     # 0.5 * sigmoid(0.45) = 0.305: above 0.3, below every dense score
    b, s = boxes_and_scores(heads, ncls, cfg, size)
    ref = OD.combined_nms(b, s, 100, 100, 0.0, cfg["score_threshold"])
    w = chunk_witness(s[0], cfg["score_threshold"], (ref[4][0], ref[2][0], ref[3][0]))
    return heads, ref, w
