"""The dynamic loss scaler's rule restated in numpy (float32 arithmetic, like the device state), for the tests of the device-side
implementation (csrc/optim.hip: scaler_advance_kernel).  It is Apex's `LossScaler.update_scale` plus a floor and a ceiling:

    overflow:   scale = max(min_scale, scale * backoff_factor); unskipped = 0; skipped_total += 1; skipped_in_a_row += 1
    otherwise:  unskipped += 1; skipped_in_a_row = 0
                if unskipped == growth_interval: scale = min(max_scale, scale * growth_factor); unskipped = 0

State layout (include/vlbert_hip.h, VLB_SCALER_*): [scale, growth_factor, backoff_factor, growth_interval, unskipped, skipped_total,
skipped_in_a_row, min_scale, max_scale].
"""
import numpy as np

FIELDS = ("scale", "growth_factor", "backoff_factor", "growth_interval", "unskipped", "skipped_total", "skipped_in_a_row", "min_scale",
          "max_scale")


def initial(init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0, max_scale=2.0 ** 24):
    return np.array([init_scale, growth_factor, backoff_factor, growth_interval, 0, 0, 0, min_scale, max_scale], dtype=np.float32)


def update(state, overflow):
    """One optimizer step: -> the new state (a copy).  overflow: the step's squared gradient norm was not finite."""
    s = np.array(state, dtype=np.float32, copy=True)
    f32 = np.float32
    if overflow:
        s[0] = max(s[7], f32(s[0] * s[2]))
        s[4] = 0
        s[5] += 1
        s[6] += 1
    else:
        s[4] += 1
        s[6] = 0
        if s[4] == s[3]:
            s[0] = min(s[8], f32(s[0] * s[1]))
            s[4] = 0
    return s


def overflowed(sumsq):
    return not np.isfinite(np.float32(sumsq))


def run(state, overflows):
    """The states after each step of a sequence of overflow flags."""
    out = []
    for o in overflows:
        state = update(state, bool(o))
        out.append(state)
    return out


def as_dict(state):
    return {k: (int(v) if k in ("growth_interval", "unskipped", "skipped_total", "skipped_in_a_row") else float(v))
            for k, v in zip(FIELDS, state)}


def lr_lambda(kind, k, warmup_steps, t_total):
    """The schedule factor at scheduler step k (common/nlp/bert/optimization.py:27-62): kind 0 constant | 1 warmup-constant | 2
    warmup-linear; with a loss scaler k = steps taken + steps skipped + 1."""
    f32 = np.float32
    k, w, t = f32(k), f32(warmup_steps), f32(t_total)
    if kind == 0:
        return f32(1.0)
    if k < w:
        return f32(k / max(f32(1.0), w))
    if kind == 2:
        return f32(max(f32(0.0), f32(f32(t - k) / max(f32(1.0), f32(t - w)))))
    return f32(1.0)
