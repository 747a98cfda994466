"""Loss-scale policy of fp16 training: the rule of Keras' LossScaleOptimizer (the framework the reference runs on), pure Python.

The scale S multiplies the gradient before its rounding to fp16 (y4_block_grad_scaled) and is divided out of the float32 sum.  It
is always a power of two, so that both products are exact.  A step whose gradient overflowed is skipped: no Adam step, no step
count.  With the dynamic rule the scale is then halved, and after `growth_interval` steps without an overflow it doubles."""
import math


def is_power_of_two(x):
    """A finite positive power of two (2**k, k any integer) that a float32 holds as a normal number?"""
    if isinstance(x, (str, bytes)):
        return False
    try:
        x = float(x)
    except (TypeError, ValueError):
        return False
    if not math.isfinite(x) or x <= 0.0:
        return False
    m, e = math.frexp(x)
    return m == 0.5 and -125 <= e <= 128           # 2**-126 .. 2**127


class LossScale:
    """LossScale() is Keras' dynamic loss scale with its defaults: initial 2**15, doubled every 2000 applied steps, halved on
    an overflow.  `update(overflow)` is called once per step with that step's overflow flag and returns whether the step
    applies.  `scale` is the value the NEXT step runs with, `skipped` counts the skipped steps.

    LossScale.static(s) never changes its scale; an overflow still skips the step and is counted."""

    def __init__(self, initial=2 ** 15, growth_interval=2000, factor=2, minimum=1, maximum=2 ** 24, dynamic=True):
        for name, v in (("initial", initial), ("factor", factor), ("minimum", minimum), ("maximum", maximum)):
            if not is_power_of_two(v):
                raise ValueError(f"LossScale: {name} {v!r} is not a finite positive power of two")
        if factor <= 1:
            raise ValueError(f"LossScale: factor {factor!r} must be above 1")
        if int(growth_interval) != growth_interval or growth_interval < 1:
            raise ValueError(f"LossScale: growth_interval {growth_interval!r} must be a positive integer")
        if not minimum <= initial <= maximum:
            raise ValueError(f"LossScale: initial {initial!r} outside [{minimum!r}, {maximum!r}]")
        self.scale = float(initial)
        self.growth_interval, self.factor = int(growth_interval), float(factor)
        self.minimum, self.maximum = float(minimum), float(maximum)
        self.dynamic = bool(dynamic)
        self.good_steps = 0          # applied steps since the last change of the scale or the last overflow
        self.skipped = 0

    @classmethod
    def static(cls, scale):
        if not is_power_of_two(scale):
            raise ValueError(f"loss_scale {scale!r} is not a finite positive power of two")
        return cls(initial=scale, minimum=scale, maximum=scale, dynamic=False)

    def update(self, overflow):
        if overflow:
            self.skipped += 1
            self.good_steps = 0
            if self.dynamic:
                self.scale = max(self.scale / self.factor, self.minimum)
            return False
        self.good_steps += 1
        if self.dynamic and self.good_steps >= self.growth_interval:
            self.scale = min(self.scale * self.factor, self.maximum)
            self.good_steps = 0
        return True


def make_loss_scale(value):
    """fit's `loss_scale` argument -> LossScale: 'dynamic', a LossScale (used as it is, so its state carries over), or a power
    of two (a static scale)."""
    if isinstance(value, LossScale):
        return value
    if isinstance(value, str):
        if value == "dynamic":
            return LossScale()
        raise ValueError(f"loss_scale {value!r}: 'dynamic', a LossScale or a power of two")
    if isinstance(value, bool) or not is_power_of_two(value):
        raise ValueError(f"loss_scale {value!r}: 'dynamic', a LossScale or a power of two")
    return LossScale.static(value)
