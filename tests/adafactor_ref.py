"""Float64 restatement of one Adafactor step, the metrics that resolve a single update, and the cases the Adafactor tests share
(tests/test_adafactor_cpu.py measures the floors and the power of the metric; tests/test_adafactor_gpu.py and the tightened tests
of test_train_gpu.py / test_grad_accum_gpu.py hold csrc/adafactor.hip to it).  A plain helper module: no fixtures, no pytest hooks.

The step is transformers.optimization.Adafactor as ref: music2midi/model.py:27-30 builds it, i.e. oracle/train.py AdafactorOracle:
eps = (1e-30, 1e-3), clip_threshold 1.0, decay_rate -0.8, scale_parameter, relative_step, warmup_init; dim >= 2 is factored."""
import copy
import math

import torch

from music2midi_amd import synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config

EPS_FP32 = float(torch.finfo(torch.float32).eps)        # 2^-23: one ulp of a stored parameter, relative

MUTANTS = ("update_x0.9", "no_clip", "row_not_normalised", "col_mean_over_cols", "beta2_of_t_minus_1", "rho_without_cap",
           "no_rms_floor", "col_factor_from_previous_step")


def fresh_state(shape):
    """the float64 second moments before the first step: {"row", "col"} for a matrix, {"v"} for a vector"""
    if len(shape) >= 2:
        return {"row": torch.zeros(shape[:-1], dtype=torch.float64), "col": torch.zeros(shape[:-2] + shape[-1:], dtype=torch.float64)}
    return {"v": torch.zeros(shape, dtype=torch.float64)}


def ref_step(p, g, state, t, mutant=None):
    """One step at step number t (1-based) in float64.  p: the fp32 parameter as stored, g: the gradient, state: float64 second
    moments (fresh_state or a previous return; not modified).  Returns (delta, new_state): the new parameter is p + delta.
    mutant: one of MUTANTS, a deliberately wrong step (tests/test_adafactor_cpu.py shows the metric sees each of them)."""
    assert mutant is None or mutant in MUTANTS, mutant
    eps1, eps2, clip, decay = 1e-30, 1e-3, 1.0, -0.8
    p, g = p.detach().double(), g.detach().double()
    rho = 1e-6 * t if mutant == "rho_without_cap" else min(1e-6 * t, 1.0 / math.sqrt(t))
    rms_p = float(p.norm(2)) / math.sqrt(p.numel())
    lr = (rms_p if mutant == "no_rms_floor" else max(eps2, rms_p)) * rho
    tb = max(t - 1, 1) if mutant == "beta2_of_t_minus_1" else t
    beta2t = 1.0 - math.pow(tb, decay)
    upd = g * g + eps1
    if g.dim() >= 2:
        col_n = g.shape[-1] if mutant == "col_mean_over_cols" else g.shape[-2]
        row = state["row"] * beta2t + upd.mean(dim=-1) * (1.0 - beta2t)
        col = state["col"] * beta2t + (upd.sum(dim=-2) / col_n) * (1.0 - beta2t)
        new = {"row": row, "col": col}
        r = row if mutant == "row_not_normalised" else row / row.mean(dim=-1, keepdim=True)
        c = state["col"] if mutant == "col_factor_from_previous_step" and float(state["col"].min()) > 0.0 else col
        upd = r.rsqrt().unsqueeze(-1) * c.rsqrt().unsqueeze(-2) * g
    else:
        v = state["v"] * beta2t + upd * (1.0 - beta2t)
        new = {"v": v}
        upd = v.rsqrt() * g
    if mutant != "no_clip":
        upd = upd / max(1.0, float(upd.norm(2)) / math.sqrt(upd.numel()) / clip)
    delta = -(upd * lr)
    if mutant == "update_x0.9":
        delta = delta * 0.9
    return delta, new


def update_error(p_new, p_old, delta):
    """max_elem(|p_new - (p_old + delta)| - eps_fp32 |p_old|) / max|delta|: one ulp of the stored parameter is free (an fp32
    `p -= small` cannot avoid it), the rest is charged against the size of the update.  None when the update is exactly zero
    (the caller then asks for bit-identity)."""
    dmax = float(delta.abs().max())
    if dmax == 0.0:
        return None
    p_old = p_old.detach().double()
    excess = (p_new.detach().double() - (p_old + delta)).abs() - EPS_FP32 * p_old.abs()
    return max(0.0, float(excess.max())) / dmax


def state_flat(state):
    """a tensor's float64 state in the order of the native buffer: R | C, or V"""
    return torch.cat([state["row"].reshape(-1), state["col"].reshape(-1)]) if "row" in state else state["v"].reshape(-1)


def state_error(got, state):
    """worst per-element relative error of exported second moments (flat, R | C or V) against the float64 state"""
    want = state_flat(state)
    return float(((got.detach().double().reshape(-1) - want).abs() / want.abs()).max())


# ---------------------------------------------------------------------------------------------------------------- the cases
# Geometries: (a) the default widths with one encoder and one decoder layer: (400,384) (384,512) (512,384) (384,1152) (1152,384)
# (3,384) (6,384) (32,8) (384,) -> 1.5, 2 and 4.5 trips of the kernels' 256-column loops, 72 row blocks; (b) the tiny widths with
# 4113 vocabulary rows: 258 row blocks of 16, the last holding one row (second trip of the 256-block strides, a tail of 2 after the
# 8-way unrolled column-partial loop); (c) 409 rows: 26 blocks, the last holding 9 rows.
GEOMETRIES = ("full_1layer", "tiny_v4113", "tiny_v409")
SMALL_TENSOR = "transformer.encoder.block.0.layer.1.DenseReluDense.wo.weight"      # parameters scaled by 1e-4: rms under the 1e-3 floor
ZERO_TENSOR = "transformer.decoder.block.0.layer.1.EncDecAttention.q.weight"       # gradient exactly zero at every step
SMALL_SCALE = 1e-4
# regimes: (first step, number of steps, all-zero gradients).  Warm-up starts fresh; the others start from primed_state() loaded
# at step first - 1.  9 998 - 10 001 crosses rho = min(1e-6 t, 1/sqrt(t)) at t = 10 000.
REGIMES = {"warmup": (1, 4, False), "late_10k": (9998, 4, False), "late_40k": (40000, 2, False), "all_zero": (5, 1, True)}


def case_config(geometry):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    if geometry == "full_1layer":
        cfg["model"]["t5"].update(num_layers=1, num_decoder_layers=1)
    else:
        cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2,
                                  vocab_size={"tiny_v4113": 4113, "tiny_v409": 409}[geometry])
    return cfg


def case_params(geometry):
    """{name: fp32 tensor} of the case's initial parameters (synth, seed 0), SMALL_TENSOR scaled down"""
    from oracle.train import leaf_params
    geom = T5Geometry(load_config(case_config(geometry)).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    params = {k: v.detach().clone() for k, v in leaf_params(sd).items()}
    params[SMALL_TENSOR] *= SMALL_SCALE
    return params


def case_grads(shapes, t, all_zero=False):
    """{name: gradient} of step t for {name: shape}: N(0, scale^2) with scale cycling 1e-2 .. 10 over steps and tensors (the update
    clipping goes both ways), rows 5-18 of every matrix of more than 20 rows exactly zero (embedding rows of tokens a batch does not
    contain), ZERO_TENSOR zero throughout."""
    grads, order = {}, {k: i for i, k in enumerate(sorted(shapes))}      # (the scale must not depend on the order the caller lists tensors in)
    for k, shape in shapes.items():
        i = order[k]
        if all_zero or k == ZERO_TENSOR:
            grads[k] = torch.zeros(tuple(shape))
            continue
        g = torch.from_numpy(synth.normal(t, k, tuple(shape), 10.0 ** ((t + i) % 4 - 2)))
        if len(shape) == 2 and shape[0] > 20:
            g[5:19] = 0.0
        grads[k] = g
    return grads


def primed_state(params):
    """{name: float64 state} after ONE float64 step (the gradients of step 0) from fresh, rounded to fp32: the second moments the
    late regimes load on both sides"""
    shapes = {k: tuple(v.shape) for k, v in params.items()}
    grads = case_grads(shapes, 0)
    return {k: {n: s.float().double() for n, s in ref_step(params[k], grads[k], fresh_state(shapes[k]), 1)[1].items()} for k in params}


class Worst:
    """collects (value, tensor, step) and reports the largest"""

    def __init__(self, what, bar):
        self.what, self.bar, self.items = what, bar, []

    def add(self, value, name, step):
        self.items.append((value, name, step))

    def top(self, n=5):
        return sorted(self.items, key=lambda e: -e[0] if e[0] == e[0] else -math.inf)[:n]

    def worst(self):
        return self.top(1)[0][0] if self.items else 0.0

    def report(self, where):
        if not self.items:
            return f"{where}: no {self.what} measured"
        v, name, step = self.top(1)[0]
        return f"{where}: worst {self.what} {v:.3e} ({name}, step {step}); bar {self.bar:.3e}"

    def check(self, where):
        bad = [e for e in self.items if not e[0] <= self.bar]
        assert not bad, f"{where}: {len(bad)} {self.what} over {self.bar:.3e}; five worst (tensor, step, value): " \
                        f"{[(n, s, float(f'{v:.3e}')) for v, n, s in sorted(bad, key=lambda e: -e[0] if e[0] == e[0] else -math.inf)[:5]]}"


def run_steps(step_fn, get_params, get_state, shapes, regime, state64, update_bar, state_bar, where, probe=None):
    """The loop both the CPU and the GPU tests run.  Per step of the regime: read the implementation's own parameters (so errors do not
    compound and a failure names a tensor and a step), step it with case_grads, and hold every tensor's new parameters to
    p_old + delta64 and its second moments to the float64 state.
      step_fn(grads, t): one step of the implementation under test;  get_params() -> {name: fp32 cpu tensor} (copies);
      get_state() -> {name: flat fp32 cpu tensor, R | C or V};  state64: {name: float64 state} the reference starts from.
    A tensor whose float64 update is exactly zero is held to bit-identity instead.  Returns (update Worst, state Worst, number of
    (tensor, step) pairs that were held to bit-identity, final float64 state).  probe(t, name, p_old, g, state_before, delta), when
    given, is called for every tensor and step with the reference's view of it."""
    first, n, all_zero = REGIMES[regime]
    upd, st, skipped = Worst("update error", update_bar), Worst("state error", state_bar), 0
    for t in range(first, first + n):
        grads = case_grads(shapes, t, all_zero)
        p_old = get_params()
        step_fn(grads, t)
        p_new, s_new = get_params(), get_state()
        for k in shapes:
            before = state64[k]
            delta, state64[k] = ref_step(p_old[k], grads[k], before, t)
            if probe is not None:
                probe(t, k, p_old[k], grads[k], before, delta)
            e = update_error(p_new[k], p_old[k], delta)
            if e is None:
                skipped += 1
                assert torch.equal(p_new[k], p_old[k]), f"{where}: {k} moved at step {t} under an exactly-zero update"
            else:
                upd.add(e, k, t)
            st.add(state_error(s_new[k], state64[k]), k, t)
    return upd, st, skipped, state64


# --------------------------------------------------------------------------------------------------------- recorded floors
# What the fp32 AdafactorOracle (oracle/train.py, pinned to HuggingFace by the `train` golden) needs against ref_step, measured by
# tests/test_adafactor_cpu.py on the CPU on 2026-10-19 (the same figures with 1, 4 and 16 torch threads): per regime the worst over
# GEOMETRIES, with SMALL_TENSOR, ZERO_TENSOR and the zero rows as in case_grads, rounded up to two digits.  Measured, as
# full_1layer / tiny_v4113 / tiny_v409:
#   update   warmup 2.135e-6 / 1.173e-6 / 2.318e-7   late_10k 3.883e-6 / 3.175e-6 / 4.037e-7   late_40k 3.171e-6 / 1.248e-6 / 3.589e-7
#   state    warmup 3.855e-7 / 3.385e-7 / 3.385e-7   late_10k 3.966e-7 / 4.379e-7 / 4.379e-7   late_40k 2.237e-7 / 1.965e-7 / 1.965e-7
#            all_zero 9.938e-8 / 9.964e-8 / 9.964e-8   (the all-zero step has no update to measure: every tensor is held to bit-identity)
# One floor per regime, not per geometry: the rounding is a property of the arithmetic, and the worst of more tensors is the better
# estimate of it.  tests/test_adafactor_cpu.py asserts the oracle stays at or under them (and that they are not looser than measured).
UPDATE_FLOOR = {"warmup": 2.2e-6, "late_10k": 3.9e-6, "late_40k": 3.2e-6, "all_zero": 0.0}
STATE_FLOOR = {"warmup": 3.9e-7, "late_10k": 4.4e-7, "late_40k": 2.3e-7, "all_zero": 1.0e-7}
# The device bar: 8x the floor of the same metric.  The kernels sum up to 1152 columns and 4113 rows in another fixed order than
# torch, use the hardware rsqrt and may contract to FMA; each shifts the update by a few 1e-7 relative.  Derived from the oracle,
# never from the device's output; the weakest mutant (update x 0.9) sits at 0.1.
DEVICE_MARGIN = 8.0


def update_bar(regime):
    return DEVICE_MARGIN * UPDATE_FLOOR[regime]


def state_bar(regime):
    return DEVICE_MARGIN * STATE_FLOOR[regime]
