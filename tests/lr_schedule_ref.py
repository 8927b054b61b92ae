"""The learning-rate schedule restated in pure Python float64 with `math`: what recnet_lr_at, and with
it the Adam launches on the device, are held to (tests/test_lr_schedule.py, tests/test_gpu_lr_schedule.py).  Nothing in this
module touches the library or a GPU.

  n: the 1-based optimiser step;  W = warmup_steps;  m = max(0, n - W);  M = total_steps - W
  warm(n)  = n / W for n < W, else 1
  decay(n) = constant 1 | linear 1 - (1 - fmin) min(m, M) / M | cosine fmin + (1 - fmin) (1 + cos(pi min(m, M) / M)) / 2
           | invsqrt max(fmin, sqrt(max(W, 1) / max(n, max(W, 1)))) | step max(fmin, gamma ^ floor(m / period))
  lr(n)    = base_lr * scale * warm(n) * decay(n);  no schedule (None): base_lr * scale"""
import math

KINDS = ("constant", "linear", "cosine", "invsqrt", "step")


def factor(sched, n):
    """warm(n) * decay(n) of the schedule given as a dict (api.LRSchedule.to_dict's fields, missing ones at their defaults);
    None: 1.0."""
    if sched is None:
        return 1.0
    kind = sched["kind"]
    W, total, period = int(sched.get("warmup_steps", 0)), int(sched.get("total_steps", 0)), int(sched.get("period", 0))
    fmin, gamma = float(sched.get("min_factor", 0.0)), float(sched.get("gamma", 1.0))
    n = int(n)
    m, M = max(0, n - W), total - W
    warm = n / W if n < W else 1.0
    if kind == "constant":
        decay = 1.0
    elif kind == "linear":
        decay = 1.0 - (1.0 - fmin) * min(m, M) / M
    elif kind == "cosine":
        decay = fmin + (1.0 - fmin) * 0.5 * (1.0 + math.cos(math.pi * min(m, M) / M))
    elif kind == "invsqrt":
        W1 = max(W, 1)
        decay = max(fmin, math.sqrt(W1 / max(n, W1)))
    elif kind == "step":
        decay = max(fmin, gamma ** (m // period))
    else:
        raise ValueError("unknown kind %r" % (kind,))
    return warm * decay


def lr_at(sched, base_lr, n, scale=1.0):
    return float(base_lr) * float(scale) * factor(sched, n)
