"""The NMS keywords of Engine and Yolov4 as one bundle, and the validation the two score-decay modes share (`Engine._decay_mode`).
No GPU: nothing here creates a handle."""
import inspect

import pytest

from yolo4hip.api import Yolov4
from yolo4hip.engine import Engine

nan, inf = float("nan"), float("inf")

# what `set_nms_soft` / `set_nms_matrix` must refuse: the lists of the two contract tests (tests/test_gpu_soft_nms.py,
# tests/test_gpu_matrix_nms.py: test_contract_round_trip_refusals_and_siblings), restated
BAD = {
    "soft": ({"method": "exp"}, {"method": 1}, {"method": "gaussian", "sigma": 0.0}, {"method": None, "sigma": nan},
             {"method": "linear", "sigma": "x"}, {"method": "gaussian", "min_score": 1.0}, {"method": "gaussian", "min_score": -0.1},
             {"method": "gaussian", "min_score": nan}, {"method": "hard", "top_k": 0}, {"method": "hard", "top_k": 4097},
             {"method": "hard", "top_k": 64.0}, {"method": "hard", "top_k": True}),
    "matrix": ({"method": "exp"}, {"method": "hard"}, {"method": 1}, {"method": "gaussian", "sigma": 0.0}, {"method": None, "sigma": nan},
               {"method": "linear", "sigma": "x"}, {"method": "gaussian", "min_score": 1.0}, {"method": "gaussian", "min_score": -0.1},
               {"method": "gaussian", "min_score": nan}, {"method": "linear", "top_k": 0}, {"method": "linear", "top_k": 4097},
               {"method": "linear", "top_k": 64.0}, {"method": "linear", "top_k": True}),
}
# the keyword each value arrives under, which is what the message names
NAMED = {"soft": "nms_soft", "matrix": "nms_matrix", "sigma": "nms_sigma", "min_score": "nms_soft_min_score", "top_k": "nms_top_k"}


class _Attrs:
    """An object with the given attributes: `nms_options` reads nothing else."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def test_nms_options_are_the_nms_keywords_of_build():
    params = inspect.signature(Engine._build).parameters
    names = [k for k in params if k.startswith("nms_")]
    assert len(names) >= 9 and all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names)
    values = {k: object() for k in names}
    for cls in (Engine, Yolov4):
        got = cls.nms_options(_Attrs(other=1, **values))
        assert list(got) == names and all(got[k] is values[k] for k in names), cls
    # ... and Engine's constructor hands every keyword on, so `_build` is the one place of the defaults
    assert [p.kind for p in inspect.signature(Engine.__init__).parameters.values()][-1] is inspect.Parameter.VAR_KEYWORD
    assert not [k for k in inspect.signature(Engine.__init__).parameters if k.startswith("nms_")]


@pytest.mark.parametrize("family", ["soft", "matrix"])
def test_decay_mode_refuses_what_the_contract_tests_list(family):
    for kw in BAD[family]:
        args = {"method": None, "sigma": 0.5, "min_score": None, "top_k": 4096, **kw}
        with pytest.raises(ValueError) as e:
            Engine._decay_mode(family, args["method"], args["sigma"], args["min_score"], args["top_k"])
        bad_key = [k for k in kw if k != "method"] or [family]
        assert str(e.value).startswith(NAMED[bad_key[0]] + " must be"), (kw, str(e.value))
    methods = {"soft": Engine.SOFT_METHODS, "matrix": Engine.MATRIX_METHODS}[family]
    for number, method in enumerate(methods):
        assert Engine._decay_mode(family, method, 0.25, 0.125, 77) == (number, 0.25, 0.125, 77)
        assert Engine._decay_mode(family, method, 1, None, 1) == (number, 1.0, None, 1)
    assert Engine.SOFT_TOP_K_MAX == 4096 and Engine._decay_mode(family, None, 0.5, 0.0, 4096) == (0, 0.5, 0.0, 4096)
