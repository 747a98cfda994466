"""yolo4hip/loss_scale.py: the LossScale state machine against a restatement of the rule of Keras' LossScaleOptimizer -- an
overflow halves the scale (not below the minimum), resets the growth counter and skips the step; `growth_interval` applied steps
in a row double it (not above the maximum).  No GPU."""
import random

import pytest

from yolo4hip.loss_scale import LossScale, is_power_of_two, make_loss_scale


def restated(flags, scale, interval, lo, hi, dynamic=True):
    """-> [(applies, scale after the step)] for the overflow flags of a run"""
    out, good = [], 0
    for f in flags:
        if f:
            good = 0
            if dynamic:
                scale = max(scale / 2, lo)
        else:
            good += 1
            if dynamic and good == interval:
                scale, good = min(scale * 2, hi), 0
        out.append((not f, scale))
    return out


def run(policy, flags):
    return [(policy.update(f), policy.scale) for f in flags]


def test_defaults_are_keras_defaults():
    p = LossScale()
    assert (p.scale, p.growth_interval, p.factor, p.minimum, p.maximum) == (2.0 ** 15, 2000, 2.0, 1.0, 2.0 ** 24)
    assert run(p, [False] * 1999)[-1] == (True, 2.0 ** 15)
    assert p.update(False) and p.scale == 2.0 ** 16 and p.good_steps == 0


def test_halving_and_the_floor_at_minimum():
    p = LossScale(initial=8, minimum=2)
    assert run(p, [True] * 4) == [(False, 4.0), (False, 2.0), (False, 2.0), (False, 2.0)]
    assert p.skipped == 4


def test_an_overflow_resets_the_growth_counter():
    p = LossScale(initial=16, growth_interval=3)
    flags = [False, False, True, False, False, False, False]
    assert run(p, flags) == [(True, 16.0), (True, 16.0), (False, 8.0), (True, 8.0), (True, 8.0), (True, 16.0), (True, 16.0)]
    assert run(LossScale(initial=16, growth_interval=3), flags) == restated(flags, 16.0, 3, 1.0, 2.0 ** 24)


def test_the_cap_at_maximum():
    p = LossScale(initial=2 ** 23, growth_interval=1)
    assert run(p, [False] * 3) == [(True, 2.0 ** 24)] * 3
    p = LossScale(initial=4, growth_interval=2, maximum=8)
    assert [s for _, s in run(p, [False] * 6)] == [4.0, 8.0, 8.0, 8.0, 8.0, 8.0]


@pytest.mark.parametrize("seed", range(4))
def test_random_runs_follow_the_restatement(seed):
    rng = random.Random(seed)
    interval, lo, hi, start = rng.choice([1, 2, 5]), 2.0 ** rng.choice([0, 3]), 2.0 ** rng.choice([10, 24]), 2.0 ** rng.choice([4, 9])
    flags = [rng.random() < 0.3 for _ in range(200)]
    p = LossScale(initial=start, growth_interval=interval, minimum=lo, maximum=hi)
    assert run(p, flags) == restated(flags, start, interval, lo, hi)
    assert p.skipped == sum(flags)
    assert all(is_power_of_two(s) and lo <= s <= hi for _, s in restated(flags, start, interval, lo, hi))


def test_a_static_number_never_changes():
    p = make_loss_scale(256)
    assert isinstance(p, LossScale) and not p.dynamic and p.scale == 256.0
    flags = [False, True, True] + [False] * 5000
    got = run(p, flags)
    assert got == restated(flags, 256.0, 2000, 256.0, 256.0, dynamic=False)
    assert {s for _, s in got} == {256.0} and p.skipped == 2
    assert make_loss_scale(0.5).scale == 0.5 and make_loss_scale(2.0 ** 20).scale == 2.0 ** 20


def test_what_fit_accepts():
    assert make_loss_scale("dynamic").scale == 2.0 ** 15 and make_loss_scale("dynamic").dynamic
    own = LossScale(initial=2 ** 10, growth_interval=7)
    assert make_loss_scale(own) is own
    for bad in (3, 100.0, 0, -2, float("inf"), float("nan"), 2.0 ** 200, 2.0 ** -130, "static", None, True, [8]):
        with pytest.raises(ValueError):
            make_loss_scale(bad)


def test_rejection_of_non_powers_of_two():
    for kw in (dict(initial=3), dict(initial=0), dict(initial=-4), dict(initial=float("inf")), dict(factor=3), dict(factor=1),
               dict(minimum=0), dict(maximum=1000), dict(growth_interval=0), dict(growth_interval=1.5),
               dict(initial=2, minimum=4), dict(initial=2 ** 25)):
        with pytest.raises(ValueError):
            LossScale(**kw)
    assert is_power_of_two(1) and is_power_of_two(2.0 ** -14) and is_power_of_two(2 ** 24)
    assert not any(is_power_of_two(x) for x in (0, -1, 6, 0.3, float("inf"), float("nan"), "8"))
