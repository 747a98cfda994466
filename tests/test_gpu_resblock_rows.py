"""Residual-block kernel with exact-row tiles and dealt tile lists (csrc/resblock.hip): bit-identical to the unfused path on stage
sides that give every tile height and every mix of heights in a column, three ways -- as the library runs it; with Y4_RB_SLOTS=8, so
that every list holds several tiles of mixed heights; and with Y4_RB_ROWS=0, the static walk of 16-row tiles with part tiles in a
second launch.  The two switches are read once per process: each of them runs all cases in ONE fresh child process (this file as a
script), which reports per case.

Stage sides (C = 128 side / C = 64 side) of the cases: 96 -> 12 / 24, 160 -> 20 / 40, 224 -> 28 / 56, 288 -> 36 / 72, 608 -> 76 / 152,
288 x 416 -> 36 x 52 / 72 x 104.  At C = 128 that is a single short tile, 16+4, 16+12, 16+16+4 and 16*4+12 rows per column; at C = 64
16+8, 16*2+8, 16*3+8, 16*4+8 and 16*9+8."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TAPS = (10, 12, 14, 16, 19, 21, 23, 29, 35, 36, 37)
SMALL = [(96, 5), (160, 3), (224, 2), (288, 2)]
CASES = [(size, n, dtype) for size, n in SMALL + [(608, 2), ((288, 416), 2)] for dtype in ("bf16", "f16")]


def case_id(size, n, dtype):
    return "%s-%d-%s" % ("x".join(map(str, size)) if isinstance(size, tuple) else size, n, dtype)


def run_case(size, n, dtype):
    """The recipe of test_gpu_forward.test_res_fusion_is_bit_identical: materialised tensors, heads and detections of the unfused
    path against the same with the residual blocks fused, alone, with the other fusions, per image and per channel group."""
    from yolo4hip import weights as W
    from yolo4hip.config import make_config
    from yolo4hip.engine import Engine
    from yolo4hip.plan import build_plan
    plan = build_plan(size, 3)
    imgs = W.synth_images(n, size, 9)
    eng = Engine(3, make_config(size), max_batch=n, dtype=dtype)
    eng.load_weight_blob(W.flatten(W.synth_weights(plan, 9)))
    heads = eng.forward_heads(imgs)
    ref = {i: eng.conv_output(i, n) for i in TAPS}
    base = eng.predict(imgs, with_indices=True)

    def check():
        for a, b in zip(heads, eng.forward_heads(imgs)):
            assert np.array_equal(a, b)
        for i in TAPS:
            assert np.array_equal(ref[i], eng.conv_output(i, n)), i
        for a, b in zip(base, eng.predict(imgs, with_indices=True)):
            assert np.array_equal(a, b)

    assert eng.set_res_fusion(True) == 10 and eng.res_fusion_mask() == 3
    check()
    if not isinstance(size, tuple):
        eng.set_stem_fusion(True)
    eng.set_chain_fusion(True)
    eng.set_stage_fusion(True)
    check()
    eng.set_subbatch(1, 16)                  # the early blocks one image at a time: another table, fewer tiles than lists
    check()
    eng.set_subbatch(0)
    for mask in (1, 2):                      # one channel group fused, the other on its chains
        eng.set_res_fusion_mask(mask)
        check()
    eng.set_res_fusion(False)
    check()
    eng.close()


@pytest.mark.parametrize("size,n,dtype", CASES, ids=[case_id(*c) for c in CASES])
def test_rows_bit_identical(size, n, dtype):
    run_case(size, n, dtype)


_children = {}


def child_report(name, value):
    """All SMALL cases, both dtypes, in one fresh process with the switch set -> {case id: "ok" | what failed}"""
    if name not in _children:
        # the child runs ONCE per switch: what it ended with -- also a crash or the time limit -- is kept, so that the other cases
        # of the switch fail from here and start nothing more on the device
        env = dict(os.environ)
        env[name] = value
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=900)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("REPORT ")]
            if r.returncode == 0 and lines:
                _children[name] = json.loads(lines[-1][len("REPORT "):])
            else:
                _children[name] = {"error": "child ended with %s: %s %s" % (r.returncode, r.stdout[-1000:], r.stderr[-2000:])}
        except subprocess.TimeoutExpired as e:
            _children[name] = {"error": "child did not end within %s s" % e.timeout}
    return _children[name]


@pytest.mark.parametrize("switch", ["Y4_RB_SLOTS=8", "Y4_RB_ROWS=0"])
@pytest.mark.parametrize("size,n", SMALL)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_rows_bit_identical_under_switch(dtype, size, n, switch):
    report = child_report(*switch.split("="))
    assert "error" not in report, report["error"]
    assert report[case_id(size, n, dtype)] == "ok"


if __name__ == "__main__":
    for p in (os.path.join(ROOT, "yolo-v4-tf.keras_amd"), ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import traceback
    report = {case_id(size, n, dtype): "not run: an earlier case failed" for size, n in SMALL for dtype in ("bf16", "f16")}
    for key in report:
        size, n, dtype = key.split("-")
        try:
            run_case(int(size), int(n), dtype)
            report[key] = "ok"
        except Exception:                    # the first failure ends the run: nothing more is started on a device that may have faulted
            report[key] = traceback.format_exc()[-1500:]
            break
    print("REPORT " + json.dumps(report))
