"""Learning-rate schedules of basicsr/models/lr_scheduler.py -- the one the shipped option files use and the four others the
reference's ``setup_schedulers`` builds: host-side arithmetic only."""
import bisect
import math
from collections import Counter

from torch.optim.lr_scheduler import _LRScheduler


class CosineAnnealingRestartCyclicLR(_LRScheduler):
    """Cosine annealing with restarts and a minimum learning rate per cycle:
    lr = eta_min_i + w_i/2 (base_lr - eta_min_i) (1 + cos(pi (t - start_i) / period_i)) inside cycle i."""

    def __init__(self, optimizer, periods, restart_weights=(1,), eta_mins=(0,), last_epoch=-1):
        if len(periods) != len(restart_weights):
            raise AssertionError("periods and restart_weights should have the same length.")
        self.periods, self.restart_weights, self.eta_mins = list(periods), list(restart_weights), list(eta_mins)
        self.ends = [sum(self.periods[:i + 1]) for i in range(len(self.periods))]
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        i = bisect.bisect_left(self.ends, self.last_epoch)          # first cycle whose end is >= t (lr_scheduler.py:8-23)
        start = 0 if i == 0 else self.ends[i - 1]
        w, lo, per = self.restart_weights[i], self.eta_mins[i], self.periods[i]
        c = 1 + math.cos(math.pi * (self.last_epoch - start) / per)
        return [lo + w * 0.5 * (b - lo) * c for b in self.base_lrs]


class MultiStepRestartLR(_LRScheduler):
    """Step decay with restarts (``MultiStepLR`` in an option file builds this class too).  At iteration t: a restart sets
    lr = initial_lr * restart_weights[its index]; a milestone multiplies lr by gamma once per time it is listed; otherwise lr stands."""

    def __init__(self, optimizer, milestones, gamma=0.1, restarts=(0,), restart_weights=(1,), last_epoch=-1):
        if len(restarts) != len(restart_weights):
            raise AssertionError("restarts and their weights do not match.")
        self.milestones, self.gamma = Counter(milestones), gamma
        self.restarts, self.restart_weights = list(restarts), list(restart_weights)
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        t = self.last_epoch
        if t in self.restarts:
            w = self.restart_weights[self.restarts.index(t)]
            return [g["initial_lr"] * w for g in self.optimizer.param_groups]
        if t not in self.milestones:
            return [g["lr"] for g in self.optimizer.param_groups]
        return [g["lr"] * self.gamma ** self.milestones[t] for g in self.optimizer.param_groups]


class CosineAnnealingRestartLR(_LRScheduler):
    """Cosine annealing with restarts and one minimum learning rate:
    lr = eta_min + w_i/2 (base_lr - eta_min) (1 + cos(pi (t - start_i) / period_i)) inside cycle i."""

    def __init__(self, optimizer, periods, restart_weights=(1,), eta_min=0, last_epoch=-1):
        if len(periods) != len(restart_weights):
            raise AssertionError("periods and restart_weights should have the same length.")
        self.periods, self.restart_weights, self.eta_min = list(periods), list(restart_weights), eta_min
        self.ends = [sum(self.periods[:i + 1]) for i in range(len(self.periods))]
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        i = bisect.bisect_left(self.ends, self.last_epoch)          # first cycle whose end is >= t
        start = 0 if i == 0 else self.ends[i - 1]
        w, lo = self.restart_weights[i], self.eta_min
        c = 1 + math.cos(math.pi * ((self.last_epoch - start) / self.periods[i]))
        return [lo + w * 0.5 * (b - lo) * c for b in self.base_lrs]


class LinearLR(_LRScheduler):
    """lr = (1 - t / total_iter) initial_lr."""

    def __init__(self, optimizer, total_iter, last_epoch=-1):
        self.total_iter = total_iter
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        w = 1 - self.last_epoch / self.total_iter
        return [w * g["initial_lr"] for g in self.optimizer.param_groups]


class VibrateLR(_LRScheduler):
    """A triangle wave of period T = total_iter // 80 (rising over Th = T // 2 iterations, falling over the rest) under an envelope f:
    1 - 8/3 process below process = t / total_iter = 3/8, 0.2 below 5/8, 0.1 after; during the first rise the weight is at least 0.1."""

    def __init__(self, optimizer, total_iter, last_epoch=-1):
        self.total_iter = total_iter
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        process = self.last_epoch / self.total_iter
        f = 1 - process * 8 / 3 if process < 3 / 8 else 0.2 if process < 5 / 8 else 0.1
        T = self.total_iter // 80
        Th = T // 2
        t = self.last_epoch % T
        f2 = t / Th
        if t >= Th:
            f2 = 2 - f2
        w = f * f2
        if self.last_epoch < Th:
            w = max(0.1, w)
        return [w * g["initial_lr"] for g in self.optimizer.param_groups]
