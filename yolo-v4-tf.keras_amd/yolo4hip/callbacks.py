"""Callbacks `Yolov4.fit` understands.  A callback may have `on_epoch_end(epoch, logs)` and / or `schedule(epoch, lr)`: `fit` calls
`schedule` at the start of every epoch with the epoch index and the current learning rate, and trains that epoch at the rate it
returns (what Keras' LearningRateScheduler does with its schedule function)."""
import math


class CosineAnnealingScheduler:
    """Cosine annealing with warm restarts: inside a cycle of `epochs_per_cycle` epochs the rate falls from `lr_max` along half a
    cosine wave towards `lr_min`, then jumps back:  lr(e) = lr_min + (lr_max - lr_min) * (1 + cos(pi * p)) / 2  with
    p = (e mod epochs_per_cycle) / epochs_per_cycle the position in the cycle."""

    def __init__(self, epochs_per_cycle, lr_min, lr_max, verbose=0):
        if int(epochs_per_cycle) < 1:
            raise ValueError("epochs_per_cycle must be at least 1")
        self.epochs_per_cycle, self.lr_min, self.lr_max, self.verbose = int(epochs_per_cycle), float(lr_min), float(lr_max), verbose

    def schedule(self, epoch, lr=None):
        position = (int(epoch) % self.epochs_per_cycle) / self.epochs_per_cycle
        rate = self.lr_min + 0.5 * (self.lr_max - self.lr_min) * (1.0 + math.cos(math.pi * position))
        if self.verbose:
            print(f"Epoch {int(epoch) + 1}: learning rate {rate:.6g}")
        return rate
