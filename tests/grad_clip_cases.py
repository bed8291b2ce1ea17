"""Cases, the float64 reference and the recorded floors of the gradient-clipping tests (tests/test_grad_clip_cpu.py measures the floors
and the power of the metric; tests/test_grad_clip_gpu.py holds csrc/grad_clip.hip and the CLIP forms of csrc/adafactor.hip to them).
A plain helper module: no fixtures, no pytest hooks.  Everything about one Adafactor step — the float64 step, the two error metrics,
the synthetic gradients, the primed state — is tests/adafactor_ref.py's, imported and used as it is.

The reference of a clipped step: clip the gradients in float64 (clip64: the rules of music2midi_amd/clipping.py), then
adafactor_ref.ref_step on the clipped gradient.  The steps are 9 998 - 10 001 (adafactor_ref's late_10k regime) from the primed state:
at t = 1 beta2 is 0 and Adafactor's update does not change when the gradient is scaled, so a warm-up step cannot see the coefficient.
"""
import contextlib
import copy
import math

import numpy as np
import torch

import adafactor_ref as ar
from music2midi_amd import synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config

# adafactor_ref's three (every trip count of the 256-column and 16-row loops) and one with 12 + 12 layers of the tiny widths: 284
# tensors, the second trip of the finish kernel's 256-tensor loop
MANY = "tiny_many_layers"
GEOMETRIES = ar.GEOMETRIES + (MANY,)
REGIME = "late_10k"
FIRST, N_STEPS, _ = ar.REGIMES[REGIME]
VALUE_V = 0.05
# norm cases: max_norm = the fraction below of the float64 total norm of the FIRST step's gradient (rounded to fp32, so that every side
# clips against the same number) -> coef near 0.3 / near 1e-2 at every step of the regime (the totals of the four steps are within a
# factor of 2.2 of each other: every step has a quarter of the tensors at each of the four scales);  norm_1: 4x the largest total, coef 1
CASES = ("norm_0.3", "norm_1e-2", "norm_1", "value", "all_zero")
_FRACTION = {"norm_0.3": 0.3, "norm_1e-2": 1e-2}


@contextlib.contextmanager
def one_thread():
    """the CPU measurements run on one torch thread: the tensors are small (a thread pool costs more than it saves, many times more on a
    busy machine), and torch's fp32 sums then always split the same way, so the recorded floors are the same figures everywhere"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def case_config(geometry):
    if geometry != MANY:
        return ar.case_config(geometry)
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=12, num_decoder_layers=12, num_heads=2, vocab_size=409)
    return cfg


def case_state_dict(geometry):
    geom = T5Geometry(load_config(case_config(geometry)).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    return sd


def case_params(geometry):
    """as adafactor_ref.case_params, for the four geometries"""
    if geometry != MANY:
        return ar.case_params(geometry)
    from oracle.train import leaf_params
    params = {k: v.detach().clone() for k, v in leaf_params(case_state_dict(geometry)).items()}
    params[ar.SMALL_TENSOR] *= ar.SMALL_SCALE
    return params


def step_grads(shapes, case, t):
    return ar.case_grads(shapes, t, all_zero=(case == "all_zero"))


def total64(grads):
    """the norm of the per-tensor norms, in float64 (there it equals the flat norm)"""
    return math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads.values()))


def case_setting(shapes, case):
    """(mode, value) of a case for tensors of these shapes; the value is an fp32 number"""
    if case == "value":
        return "value", float(np.float32(VALUE_V))
    if case == "all_zero":
        return "norm", 1.0
    if case == "norm_1":
        top = max(total64(ar.case_grads(shapes, t)) for t in range(FIRST, FIRST + N_STEPS))
        return "norm", float(np.float32(4.0 * top))
    return "norm", float(np.float32(_FRACTION[case] * total64(ar.case_grads(shapes, FIRST))))


def clip64(grads, mode, value, mutant=None):
    """({name: float64 clipped gradient}, total norm, coef) — total and coef None in value mode.  mutant "coef_unclamped": the
    coefficient without its min(1, .)."""
    if mode == "value":
        return {k: g.double().clamp(-value, value) for k, g in grads.items()}, None, None
    assert mode == "norm", mode
    total = total64(grads)
    coef = value / (total + 1e-6)
    if mutant != "coef_unclamped":
        coef = min(1.0, coef)
    return {k: g.double() * coef for k, g in grads.items()}, total, coef


def rel(got, want):
    """relative error of one of the two norm words; a word that should be exactly 0 (the all-zero step's norm) or exactly 1 (an
    inactive coefficient) has to be exact"""
    if want == 0.0 or want == 1.0:
        return 0.0 if got == want else math.inf
    return abs(got - want) / abs(want)


def run_clipped(step_fn, get_params, get_state, get_words, shapes, case, state64, bars, where):
    """adafactor_ref.run_steps with the clipped float64 reference.  Per step of the regime: the implementation's own parameters,
    one step of it on the UNCLIPPED gradients (step_fn(grads, t) clips by the case's setting itself), and every tensor's new
    parameters against p_old + delta64(clipped gradient), its second moments against the float64 state of the clipped gradient;
    get_words() -> (total norm, coef) of the step as Python floats, against float64 (norm cases; None: not measured).
    bars: {"update", "state", "norm", "coef"}.  Returns the four ar.Worst and the number of pairs held to bit-identity."""
    mode, value = case_setting(shapes, case)
    upd, st = ar.Worst("update error", bars["update"]), ar.Worst("state error", bars["state"])
    wn, wc = ar.Worst("norm word error", bars["norm"]), ar.Worst("coef word error", bars["coef"])
    skipped = 0
    for t in range(FIRST, FIRST + (1 if case == "all_zero" else N_STEPS)):
        grads = step_grads(shapes, case, t)
        g64, total, coef = clip64(grads, mode, value)
        p_old = get_params()
        step_fn(grads, t)
        p_new, s_new = get_params(), get_state()
        if mode == "norm" and get_words is not None:
            got_total, got_coef = get_words()
            wn.add(rel(got_total, total), "total_norm", t)
            wc.add(rel(got_coef, coef), "coef", t)
        for k in shapes:
            delta, state64[k] = ar.ref_step(p_old[k], g64[k], state64[k], t)
            e = ar.update_error(p_new[k], p_old[k], delta)
            if e is None:
                skipped += 1
                assert torch.equal(p_new[k], p_old[k]), f"{where}: {k} moved at step {t} under an exactly-zero update"
            else:
                upd.add(e, k, t)
            st.add(ar.state_error(s_new[k], state64[k]), k, t)
    return upd, st, wn, wc, skipped


# --------------------------------------------------------------------------------------------------------- recorded floors
# What the fp32 oracle — clipping.clip_reference (torch's clip_grad_norm_ / clip_grad_value_ in fp32) followed by oracle/train.py's
# AdafactorOracle — needs against the reference above, measured by tests/test_grad_clip_cpu.py on the CPU on 2026-10-21: per case the
# worst over GEOMETRIES and the steps, rounded up to two digits.  Measured, as full_1layer / tiny_v4113 / tiny_v409 / tiny_many_layers:
#   update   norm_0.3 3.125e-6 / 6.637e-6 / 6.338e-7 / 5.770e-7   norm_1e-2 2.207e-6 / 4.122e-6 / 4.377e-7 / 4.263e-7
#            norm_1   3.883e-6 / 3.175e-6 / 4.037e-7 / 5.806e-7   value     4.001e-6 / 4.668e-6 / 8.530e-7 / 6.869e-7
#   state    norm_0.3 6.464e-6 / 8.087e-6 / 5.514e-7 / 4.119e-7   norm_1e-2 6.406e-6 / 7.998e-6 / 3.746e-7 / 3.551e-7
#            norm_1   3.966e-7 / 4.379e-7 / 4.379e-7 / 4.379e-7   value     3.315e-7 / 3.187e-7 / 3.187e-7 / 3.500e-7   all_zero 9.404e-8 (all four)
#   norm     3.160e-6 / 3.922e-6 / 1.951e-7 / 1.437e-7 (the gradients are the same in the three norm cases)
#   coef     norm_0.3 3.187e-6 / 3.957e-6 / 1.479e-7 / 9.578e-8   norm_1e-2 3.149e-6 / 3.958e-6 / 1.369e-7 / 1.295e-7
# torch's fp32 norm of a 400 x 384 or 4113 x 128 tensor is itself 3e-6 to 4e-6 off: that error is the coefficient's, and twice it the
# second moments' (they see coef^2), which is why the clipped cases' state floors are 20x those of the unclipped step.
# The device bar is adafactor_ref.DEVICE_MARGIN (8) x the floor of the same metric, as for the unclipped step.  A floor of 0 is exact:
# norm_1's coefficient is exactly 1 on every side, the all-zero step's norm exactly 0, and value mode has no words.
UPDATE_FLOOR = {"norm_0.3": 6.7e-6, "norm_1e-2": 4.2e-6, "norm_1": 3.9e-6, "value": 4.7e-6, "all_zero": 0.0}
STATE_FLOOR = {"norm_0.3": 8.1e-6, "norm_1e-2": 8.0e-6, "norm_1": 4.4e-7, "value": 3.6e-7, "all_zero": 9.5e-8}
NORM_FLOOR = {"norm_0.3": 4.0e-6, "norm_1e-2": 4.0e-6, "norm_1": 4.0e-6, "value": 0.0, "all_zero": 0.0}
COEF_FLOOR = {"norm_0.3": 4.0e-6, "norm_1e-2": 4.0e-6, "norm_1": 0.0, "value": 0.0, "all_zero": 0.0}


def floors(case):
    return {"update": UPDATE_FLOOR[case], "state": STATE_FLOOR[case], "norm": NORM_FLOOR[case], "coef": COEF_FLOOR[case]}


def bars(case):
    return {k: ar.DEVICE_MARGIN * v for k, v in floors(case).items()}
