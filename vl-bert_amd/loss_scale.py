"""Dynamic loss scaling of the fp16 build: Apex `FP16_Optimizer(dynamic_loss_scale=True)` -- what the reference's
`TRAIN.FP16_LOSS_SCALE: 'dynamic'` asks for (pretrain/function/train.py:345-352) -- with the state ON THE DEVICE.

The training step is a replayed hipGraph without a host synchronisation, so the skip decision, the scale, the unscale and the counter the
LR schedule runs on cannot live in Python.  `LossScaler.state` is a 9-float device array (layout: include/vlbert_hip.h, VLB_SCALER_*):
the loss kernels multiply d(logits) by `state[0]`, the optimizer kernels divide it out again, skip the update when the step's squared
gradient norm is not finite, and one single-thread kernel then applies the rule (csrc/optim.hip: scaler_advance_kernel;
tests/loss_scale_ref.py restates it in numpy):

    overflow:   scale = max(min_scale, scale * backoff_factor); unskipped = 0; skipped_total += 1; skipped_in_a_row += 1
    otherwise:  unskipped += 1; skipped_in_a_row = 0;
                if unskipped == growth_interval: scale = min(max_scale, scale * growth_factor); unskipped = 0

Defaults are Apex's (2^16, x2 / x0.5, 2000 clean steps, at most 2^24).  Deviations: `min_scale` defaults to 1.0 (Apex has no floor), and
the rule runs once per OPTIMIZER step on the accumulated gradient (Apex checks every micro-batch under gradient accumulation).
"""
FIELDS = ("scale", "growth_factor", "backoff_factor", "growth_interval", "unskipped", "skipped_total", "skipped_in_a_row", "min_scale",
          "max_scale")
COUNTERS = ("unskipped", "skipped_total", "skipped_in_a_row")
CHECKPOINT_KEY = "loss_scaler"      # top-level key of a checkpoint file (the reference's loader reads 'state_dict' / 'optimizer' only)
# The periodic host check gives up when this many steps in a row were skipped AND the scale sits on its floor: with the defaults (x0.5,
# at most 2^24) thirty-two halvings reach the floor from any scale, and gradients that are still not finite then are so for a reason no
# scale can fix.  A gentler backoff factor or a larger ceiling needs more halvings: such a run is still recovering until the floor is hit.
MAX_SKIPPED_IN_A_ROW = 32


def stuck(values):
    """The 9 state values describe a run that no loss scale can help (see MAX_SKIPPED_IN_A_ROW)."""
    return values[6] >= MAX_SKIPPED_IN_A_ROW and values[0] <= values[7]


class DynamicLossScale:
    """The configuration (a value object): `PretrainEngine(loss_scale=DynamicLossScale(init_scale=2.0 ** 12, growth_interval=500))`;
    `loss_scale="dynamic"` is `DynamicLossScale()`."""

    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, min_scale=1.0,
                 max_scale=2.0 ** 24):
        if not (growth_factor > 1.0 and 0.0 < backoff_factor < 1.0):
            raise ValueError("DynamicLossScale: growth_factor must be > 1 and backoff_factor in (0, 1)")
        if not (0.0 < min_scale <= init_scale <= max_scale) or max_scale == float("inf"):
            raise ValueError("DynamicLossScale: need 0 < min_scale <= init_scale <= max_scale < inf")
        if int(growth_interval) != growth_interval or not (1 <= growth_interval < 2 ** 24):
            raise ValueError("DynamicLossScale: growth_interval must be an integer in [1, 2^24)")
        self.init_scale, self.growth_factor, self.backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        self.growth_interval, self.min_scale, self.max_scale = int(growth_interval), float(min_scale), float(max_scale)

    def initial_values(self):
        return [self.init_scale, self.growth_factor, self.backoff_factor, float(self.growth_interval), 0.0, 0.0, 0.0, self.min_scale,
                self.max_scale]

    def __eq__(self, other):
        return isinstance(other, DynamicLossScale) and self.initial_values() == other.initial_values()

    def __hash__(self):
        return hash(tuple(self.initial_values()))

    def __repr__(self):
        return ("DynamicLossScale(init_scale=%g, growth_factor=%g, backoff_factor=%g, growth_interval=%d, min_scale=%g, max_scale=%g)"
                % (self.init_scale, self.growth_factor, self.backoff_factor, self.growth_interval, self.min_scale, self.max_scale))

    def describe(self):
        return "init %g, x%g after %d clean steps, x%g on overflow" % (self.init_scale, self.growth_factor, self.growth_interval,
                                                                       self.backoff_factor)


def resolve(loss_scale):
    """"dynamic" / a DynamicLossScale -> DynamicLossScale; anything else (None, a number) -> None."""
    if isinstance(loss_scale, str):
        if loss_scale.lower() != "dynamic":
            raise ValueError("loss_scale must be a number, None, 'dynamic' or a DynamicLossScale (got %r)" % loss_scale)
        return DynamicLossScale()
    if isinstance(loss_scale, LossScaler):
        raise ValueError("pass 'dynamic' or a DynamicLossScale: the device state (LossScaler) is built by its owner")
    return loss_scale if isinstance(loss_scale, DynamicLossScale) else None


def values_to_dict(values):
    """9 floats -> {field: value}, the counters and the interval as ints (what a checkpoint stores and scaler_state() returns)."""
    out = {}
    for k, v in zip(FIELDS, values):
        out[k] = int(round(float(v))) if (k in COUNTERS or k == "growth_interval") else float(v)
    return out


def dict_to_values(d):
    missing = [k for k in FIELDS if k not in d]
    if missing:
        raise ValueError("loss scaler state lacks %s" % missing)
    return [float(d[k]) for k in FIELDS]


def put_in_checkpoint(ck, values):
    """Store the scaler state (9 floats, or None: nothing to store) under its own top-level key of the checkpoint dict."""
    if values is not None:
        ck[CHECKPOINT_KEY] = values_to_dict(values)
    return ck


def values_from_checkpoint(ck, spec):
    """The 9 values to continue with: the checkpoint's when it carries them (a run that was dynamic), else `spec`'s initial state."""
    d = ck.get(CHECKPOINT_KEY) if ck is not None else None
    return dict_to_values(d) if d is not None else spec.initial_values()


class LossScaler:
    """The device-resident state.  One object may be shared by an engine-free training loop's optimizer and its loss calls
    (`FusedAdamW(..., loss_scaler=s)`, `ops.ce_fwd_bwd(..., dscale=s.scale)`)."""

    def __init__(self, spec=None, device="cuda:0"):
        import torch
        self.spec = spec if spec is not None else DynamicLossScale()
        self.state = torch.tensor(self.spec.initial_values(), dtype=torch.float32, device=device)
        self.scale = self.state[0:1]      # the device scalar the loss kernels read

    def read(self):
        """{field: value} with one readback (a host synchronisation: not for the timed loop)."""
        return values_to_dict(self.state.detach().cpu().tolist())

    def values(self):
        return self.state.detach().cpu().tolist()

    def load_values(self, values):
        import torch
        if len(values) != len(FIELDS):
            raise ValueError("loss scaler state: expected %d values" % len(FIELDS))
        self.state.copy_(torch.tensor([float(v) for v in values], dtype=torch.float32))

    def reset(self):
        self.load_values(self.spec.initial_values())
