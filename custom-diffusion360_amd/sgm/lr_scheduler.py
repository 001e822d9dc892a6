"""Learning-rate multipliers as functions of the step number: the YAML targets `sgm.lr_scheduler.*` a `scheduler_config` names
(DiffusionEngine.configure_optimizers, sgm/models/diffusion.py:362-374, hands `.schedule` to LambdaLR).  Use with a base lr of 1.0, or
through cd360.finetune.LRSchedule, which multiplies each group's initial lr.  Host arithmetic in float64 only; numpy's cosine, so the
values are those of the reference on the same host.

  LambdaWarmUpCosineScheduler    one linear warm-up lr_start -> lr_max over warm_up_steps, then a half cosine down to lr_min at max_decay_steps
  LambdaWarmUpCosineScheduler2   the same per cycle, the cycles listed (warm_up_steps, f_min, f_max, f_start, cycle_lengths: equal-length lists)
  LambdaLinearScheduler          per cycle: linear warm-up, then a straight line from f_max at the cycle's start towards f_min at its end
"""
from __future__ import annotations

import numpy as np


def _warm_up(start, peak, steps, n):
    return (peak - start) / steps * n + start


def _half_cosine(low, peak, t):
    return low + 0.5 * (peak - low) * (1 + np.cos(min(t, 1.0) * np.pi))


class _Schedule:
    verbosity_interval = 0

    def _report(self, n, last, extra=""):
        if self.verbosity_interval > 0 and n % self.verbosity_interval == 0:
            print(f"current step: {n}, recent lr-multiplier: {last}{extra}")

    def __call__(self, n, **kwargs):
        return self.schedule(n, **kwargs)


class LambdaWarmUpCosineScheduler(_Schedule):
    def __init__(self, warm_up_steps, lr_min, lr_max, lr_start, max_decay_steps, verbosity_interval=0):
        self.lr_warm_up_steps, self.lr_start, self.lr_min, self.lr_max = warm_up_steps, lr_start, lr_min, lr_max
        self.lr_max_decay_steps, self.verbosity_interval, self.last_lr = max_decay_steps, verbosity_interval, 0.0

    def schedule(self, n, **kwargs):
        self._report(n, self.last_lr)
        if n < self.lr_warm_up_steps:
            lr = _warm_up(self.lr_start, self.lr_max, self.lr_warm_up_steps, n)
        else:
            lr = _half_cosine(self.lr_min, self.lr_max, (n - self.lr_warm_up_steps) / (self.lr_max_decay_steps - self.lr_warm_up_steps))
        self.last_lr = lr
        return lr


class LambdaWarmUpCosineScheduler2(_Schedule):
    """Repeated cycles.  Step n belongs to the first cycle whose cumulative end is >= n (a boundary step closes its cycle), and is counted
    from that cycle's start."""

    def __init__(self, warm_up_steps, f_min, f_max, f_start, cycle_lengths, verbosity_interval=0):
        if not len(warm_up_steps) == len(f_min) == len(f_max) == len(f_start) == len(cycle_lengths):
            raise ValueError("warm_up_steps, f_min, f_max, f_start and cycle_lengths must have one length")
        self.lr_warm_up_steps, self.f_start, self.f_min, self.f_max = warm_up_steps, f_start, f_min, f_max
        self.cycle_lengths = cycle_lengths
        self.cum_cycles = np.cumsum([0] + list(cycle_lengths))
        self.verbosity_interval, self.last_f = verbosity_interval, 0.0

    def find_in_interval(self, n):
        for cycle, end in enumerate(self.cum_cycles[1:]):
            if n <= end:
                return cycle
        raise ValueError(f"step {n} lies behind the last cycle, which ends at {self.cum_cycles[-1]}")

    def _local(self, n):
        cycle = self.find_in_interval(n)
        n = n - self.cum_cycles[cycle]
        self._report(n, self.last_f, f", current cycle {cycle}")
        return cycle, n

    def _decay(self, c, n):
        return _half_cosine(self.f_min[c], self.f_max[c], (n - self.lr_warm_up_steps[c]) / (self.cycle_lengths[c] - self.lr_warm_up_steps[c]))

    def schedule(self, n, **kwargs):
        c, n = self._local(n)
        if n < self.lr_warm_up_steps[c]:
            f = _warm_up(self.f_start[c], self.f_max[c], self.lr_warm_up_steps[c], n)
        else:
            f = self._decay(c, n)
        self.last_f = f
        return f


class LambdaLinearScheduler(LambdaWarmUpCosineScheduler2):
    def _decay(self, c, n):
        return self.f_min[c] + (self.f_max[c] - self.f_min[c]) * (self.cycle_lengths[c] - n) / self.cycle_lengths[c]
