"""CPU: gradient clipping (music2midi_amd/clipping.py) — the validation rules value by value, the floors of the clipped-step metric
(tests/grad_clip_cases.py) and its power, the new exports against the header, and the bookkeeping of fit_batches' override.

Floor: what the fp32 oracle (clipping.clip_reference, then oracle/train.py's AdafactorOracle) needs against the float64 reference on
the cases the GPU test runs.  Power: the wrong steps a folded clip invites, each of which must exceed the device bar."""
import functools
import math
import re
from pathlib import Path

import pytest
import torch

import adafactor_ref as ar
import grad_clip_cases as gc
from music2midi_amd import clipping, native
from music2midi_amd.clipping import check_gradient_clip, clip_reference
from music2midi_amd.config import DEFAULT_CONFIG, ConfigNode
from music2midi_amd.model import Music2MIDI
from oracle.train import AdafactorOracle

ROOT = Path(__file__).resolve().parents[1]


# ---- check_gradient_clip ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("val, algorithm, want", [
    (None, None, ("off", 0.0)), (None, "value", ("off", 0.0)), (0, None, ("off", 0.0)), (0.0, "norm", ("off", 0.0)),
    (-1.0, "value", ("off", 0.0)), (1.0, None, ("norm", 1.0)), (1, None, ("norm", 1.0)), (0.5, "norm", ("norm", 0.5)),
    (0.5, "NORM", ("norm", 0.5)), (0.05, "value", ("value", 0.05)), (2, "Value", ("value", 2.0))])
def test_check_gradient_clip_accepts(val, algorithm, want):
    got = check_gradient_clip(val, algorithm)
    assert got == want and isinstance(got[1], float)


@pytest.mark.parametrize("val", [True, False, "1.0", [1.0]])
def test_a_clip_value_that_is_no_number_is_a_type_error(val):
    with pytest.raises(TypeError):
        check_gradient_clip(val, None)
    with pytest.raises(TypeError):
        check_gradient_clip(val, "value")


@pytest.mark.parametrize("algorithm", ["l2", "", "norm ", 1, True])
def test_an_unknown_algorithm_is_a_value_error(algorithm):
    with pytest.raises(ValueError):
        check_gradient_clip(1.0, algorithm)
    with pytest.raises(ValueError):
        check_gradient_clip(None, algorithm)              # refused even while clipping is off, as the Trainer does


def test_clip_reference_is_torch():
    g = [torch.tensor([3.0, 0.0]), torch.tensor([[0.0, 4.0]])]
    total = clip_reference(g, "norm", 1.0)
    assert float(total) == 5.0                                              # the norm of (3, 4)
    coef = torch.tensor(1.0) / (torch.tensor(5.0) + 1e-6)
    assert torch.equal(g[0], torch.tensor([3.0, 0.0]) * coef) and torch.equal(g[1], torch.tensor([[0.0, 4.0]]) * coef)
    g = [torch.tensor([3.0, -0.01, float("nan"), -7.0])]
    assert clip_reference(g, "value", 0.05) is None
    assert torch.equal(g[0][[0, 1, 3]], torch.tensor([0.05, -0.01, -0.05])) and math.isnan(float(g[0][2]))
    g = [torch.tensor([1.0, float("inf")])]
    assert float(clip_reference(g, "norm", 1.0)) == math.inf and float(g[0][0]) == 0.0 and math.isnan(float(g[0][1]))
    g = [torch.tensor([1.0])]
    assert clip_reference(g, "off", 0.0) is None and float(g[0]) == 1.0
    assert clipping.MODE_CODES == {"off": 0, "norm": 1, "value": 2}


# ---- the floors -------------------------------------------------------------------------------------------------------------
class _Oracle:
    """clip_reference + AdafactorOracle, in fp32, behind the callables of grad_clip_cases.run_clipped"""

    def __init__(self, params, state64, step, setting):
        self.params = {k: v.clone() for k, v in params.items()}
        self.opt = AdafactorOracle(self.params)
        for k, s in state64.items():
            self.opt.state[k] = dict({"step": step}, **{n: v.float() for n, v in s.items()})
        self.mode, self.value = setting
        self.words = None

    def step(self, grads, t):
        g = {k: v.clone() for k, v in grads.items()}
        total = clip_reference(list(g.values()), self.mode, self.value)
        if total is not None:
            q = self.value / (total + 1e-6)                                 # clip_grad_norm_'s own coefficient, in fp32 as it takes it
            self.words = (float(total), float(torch.clamp(q, max=1.0)))
        self.opt.step(g)
        assert all(s["step"] == t for s in self.opt.state.values())

    def get_params(self):
        return {k: v.clone() for k, v in self.params.items()}

    def get_state(self):
        return {k: (torch.cat([s["row"].reshape(-1), s["col"].reshape(-1)]) if "row" in s else s["v"].reshape(-1).clone())
                for k, s in self.opt.state.items()}


@functools.lru_cache(maxsize=None)
def _params(geometry):
    return gc.case_params(geometry)


@functools.lru_cache(maxsize=None)
def _primed(geometry):
    return ar.primed_state(_params(geometry))


@functools.lru_cache(maxsize=None)
def _measure(geometry, case):
    with gc.one_thread():
        return _measure_now(geometry, case)


def _measure_now(geometry, case):
    params = _params(geometry)
    shapes = {k: tuple(v.shape) for k, v in params.items()}
    side = _Oracle(params, _primed(geometry), gc.FIRST - 1, gc.case_setting(shapes, case))
    where = f"fp32 oracle {geometry} {case}"
    out = gc.run_clipped(side.step, side.get_params, side.get_state, lambda: side.words, shapes, case, dict(_primed(geometry)),
                         gc.floors(case), where)
    for w in out[:4]:
        print(w.report(where))
    return out + (len(shapes),)


def test_the_many_layer_geometry_has_more_than_256_tensors():
    assert len(_params(gc.MANY)) > 256


@pytest.mark.parametrize("case", gc.CASES)
@pytest.mark.parametrize("geometry", gc.GEOMETRIES)
def test_fp32_oracle_stays_within_the_recorded_floors(geometry, case):
    upd, st, wn, wc, skipped, n_tensors = _measure(geometry, case)
    where = f"fp32 oracle {geometry} {case}"
    n = 1 if case == "all_zero" else gc.N_STEPS
    assert skipped == (n_tensors if case == "all_zero" else 1) * n       # only ZERO_TENSOR, or every tensor of the all-zero step
    assert len(upd.items) + skipped == n_tensors * n and len(st.items) == n_tensors * n
    assert len(wn.items) == len(wc.items) == (0 if case == "value" else n)
    for w in (upd, st, wn, wc):
        w.check(where)


def test_recorded_floors_are_the_measured_ones():
    """the constants are the worst over the geometries, rounded up to two digits (not a looser number)"""
    for case in gc.CASES:
        for i, (name, table) in enumerate([("update", gc.UPDATE_FLOOR), ("state", gc.STATE_FLOOR), ("norm", gc.NORM_FLOOR),
                                           ("coef", gc.COEF_FLOOR)]):
            m = max(_measure(g, case)[i].worst() for g in gc.GEOMETRIES)
            print(f"{case}: measured {name} floor {m:.3e} (recorded {table[case]:.3e})")
            assert m <= table[case] <= 1.05 * m, (case, name, m)


def test_the_cases_clip_as_intended():
    """coef near 0.3 / near 1e-2 / exactly 1 at every step; the value case clamps a large share of the elements"""
    for geometry in gc.GEOMETRIES:
        shapes = {k: tuple(v.shape) for k, v in _params(geometry).items()}
        for case, lo, hi in [("norm_0.3", 0.2, 0.7), ("norm_1e-2", 6e-3, 2.5e-2), ("norm_1", 1.0, 1.0)]:
            mode, value = gc.case_setting(shapes, case)
            for t in range(gc.FIRST, gc.FIRST + gc.N_STEPS):
                coef = gc.clip64(ar.case_grads(shapes, t), mode, value)[2]
                assert lo <= coef <= hi, (geometry, case, t, coef)
        grads = ar.case_grads(shapes, gc.FIRST)
        clamped = sum(int((g.abs() > gc.VALUE_V).sum()) for g in grads.values()) / sum(g.numel() for g in grads.values())
        assert 0.2 < clamped < 0.9, (geometry, clamped)


# ---- the power of the metric ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wrong_steps(geometry, case):
    with gc.one_thread():
        return _wrong_steps_now(geometry, case)


def _wrong_steps_now(geometry, case):
    """{mutant: worst update error over the tensors} at the regime's first step, from the primed state, against the case's clipped
    float64 step.  Every mutant is a float64 step too, stored to fp32 like a parameter, so only its arithmetic differs."""
    params, state = _params(geometry), _primed(geometry)
    shapes = {k: tuple(v.shape) for k, v in params.items()}
    mode, value = gc.case_setting(shapes, case)
    t = gc.FIRST
    grads = ar.case_grads(shapes, t)
    good, _, coef = gc.clip64(grads, mode, value)
    wrong = {"no_clipping": {k: g.double() for k, g in grads.items()}}
    if mode == "norm":
        wrong["value_in_place_of_norm"] = gc.clip64(grads, "value", value)[0]
        wrong["coef_unclamped"] = gc.clip64(grads, mode, value, mutant="coef_unclamped")[0]
    else:
        wrong["norm_in_place_of_value"] = gc.clip64(grads, "norm", value)[0]
    worst = {m: 0.0 for m in wrong}
    if mode == "norm":
        worst["moments_from_the_unclipped_gradient"] = 0.0
    for k, p in params.items():
        delta, _ = ar.ref_step(p, good[k], state[k], t)
        if float(delta.abs().max()) == 0.0:
            continue
        for m, g in wrong.items():
            d_m, _ = ar.ref_step(p, g[k], state[k], t)
            worst[m] = max(worst[m], ar.update_error((p.double() + d_m).float(), p, delta))
        if mode == "norm":
            # the folded form's own mutant: passes B and C read g * coef, pass A the unclipped g.  ref_step's "no_clip" is Adafactor's
            # update clipping left out: -delta / lr is then r c g with the factors of the UNCLIPPED gradient's second moments
            rho = min(1e-6 * t, 1.0 / math.sqrt(t))
            lr = max(1e-3, float(p.double().norm(2)) / math.sqrt(p.numel())) * rho
            raw = -ar.ref_step(p, grads[k], state[k], t, mutant="no_clip")[0] / lr
            u = raw * coef
            u = u / max(1.0, float(u.norm(2)) / math.sqrt(u.numel()))
            worst["moments_from_the_unclipped_gradient"] = max(worst["moments_from_the_unclipped_gradient"],
                                                               ar.update_error((p.double() - u * lr).float(), p, delta))
    return worst


@pytest.mark.parametrize("case, mutant", [
    ("norm_0.3", "no_clipping"), ("norm_1e-2", "no_clipping"), ("value", "no_clipping"),
    ("norm_0.3", "moments_from_the_unclipped_gradient"), ("norm_1e-2", "moments_from_the_unclipped_gradient"),
    ("norm_1", "coef_unclamped"), ("norm_0.3", "value_in_place_of_norm"), ("value", "norm_in_place_of_value")])
def test_the_metric_sees_a_wrong_clip(case, mutant):
    """each wrong step exceeds the device bar of its case, on every geometry.  (One flat norm over everything in place of the norm of
    the per-tensor norms is not here: in float64 the two are the same number, and in fp32 they differ by rounding only — 1e-7 of the
    coefficient, far under any bar — so no step can tell them apart; the finish kernel's form is held by the norm word's bar.)"""
    for geometry in gc.GEOMETRIES:
        e = _wrong_steps(geometry, case)[mutant]
        print(f"{mutant} at {case}, {geometry}: {e:.3e} = {e / gc.bars(case)['update']:.3g} x the device bar")
        assert e > gc.bars(case)["update"], (geometry, e)


# ---- header against the ctypes table ----------------------------------------------------------------------------------------
def test_header_declares_what_the_binding_binds():
    import ctypes as C
    header = (ROOT / "include" / "music2midi_amd.h").read_text()
    for name, proto in [
            ("m2m_trainer_set_grad_clip", "int m2m_trainer_set_grad_clip(m2m_trainer* t, int algorithm /* 0 off, 1 norm, 2 value */, float value);"),
            ("m2m_trainer_grad_norm", "int m2m_trainer_grad_norm(m2m_trainer* t, const float* grads_dev, float* out_dev /* [2] */, void* stream);")]:
        assert proto in header, name
        assert name in native.EXPORTED_SYMBOLS and hasattr(native.load(), name)
    assert native._SIGNATURES["m2m_trainer_set_grad_clip"] == (C.c_int, [C.c_void_p, C.c_int, C.c_float])
    assert native._SIGNATURES["m2m_trainer_grad_norm"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
    lib = native.load()
    assert lib.m2m_trainer_set_grad_clip(None, 1, 1.0) == -1 and lib.m2m_trainer_grad_norm(None, None, None, None) == -1     # M2M_ERR_INVALID


# ---- fit_batches with a stand-in trainer (as tests/test_grad_accum_cpu.py's) -------------------------------------------------
class _FakeTrainer:
    def __init__(self):
        self.grads = torch.zeros(6)
        self.sync_stream = None
        self.early_ranges = []
        self.step_count = 0
        self.grad_clip = ("off", 0.0)
        self.set_calls = []
        self.seen = []                         # the clipping in force at each optimizer step

    def set_grad_clip(self, mode, value=0.0):
        self.set_calls.append((mode, value))
        self.grad_clip = (mode, value)

    def grad_stats(self):
        return torch.tensor([7.0, 0.5])


class _StubModel(Music2MIDI):
    def __init__(self, trainer_cfg):
        torch.nn.Module.__init__(self)
        cfg = dict(DEFAULT_CONFIG)
        cfg["trainer"] = dict(trainer_cfg)
        self.config = ConfigNode(cfg)
        self._trainer = _FakeTrainer()
        self.passes = 0

    def training_step(self, inputs, batch_idx):
        self.passes += 1
        self.logged = {"train/loss": torch.tensor(float(inputs))}
        return torch.tensor(float(inputs))

    def logged_metrics(self):                  # the real one, without the device of a transformer that is not there
        from music2midi_amd import distributed as D
        return D.reduce_logged(dict(self.logged))


class _Opt:
    def __init__(self, model):
        self.model = model

    def step(self):
        tr = self.model._trainer
        tr.step_count += 1
        tr.seen.append(tr.grad_clip)


_BASE = {"max_epochs": 1, "log_every_n_steps": 2}


def test_fit_batches_applies_the_config_and_the_override_for_that_call_only():
    m = _StubModel(dict(_BASE, gradient_clip_val=0.5))
    m.fit_batches(list(range(4)), optimizer=_Opt(m))
    assert m._trainer.seen == [("norm", 0.5)] * 4 and m._trainer.set_calls == [("norm", 0.5)]      # set once, not per step
    assert [h["step"] for h in m.log_history] == [2, 4] and all(h["train/grad_norm"] == 7.0 for h in m.log_history)
    m.fit_batches(list(range(2)), optimizer=_Opt(m), gradient_clip_val=0.1, gradient_clip_algorithm="value")
    assert m._trainer.seen[4:] == [("value", 0.1)] * 2
    assert "train/grad_norm" not in m.log_history[-1]                    # value mode computes no norm
    assert m._clip_override is None and m._clip_fit is None and m._gradient_clip() == ("norm", 0.5)
    m.fit_batches(list(range(1)), optimizer=_Opt(m), gradient_clip_algorithm="value")      # one keyword: the other from the config
    assert m._trainer.seen[6:] == [("value", 0.5)]
    m.fit_batches(list(range(1)), optimizer=_Opt(m), gradient_clip_val=0)                  # <= 0: off for this call
    assert m._trainer.seen[7:] == [("off", 0.0)]
    m.fit_batches(list(range(1)), optimizer=_Opt(m))
    assert m._trainer.seen[8:] == [("norm", 0.5)]


def test_absent_keys_mean_off_and_touch_nothing():
    m = _StubModel(_BASE)
    m.fit_batches(list(range(3)), optimizer=_Opt(m))
    assert m._trainer.set_calls == [] and m._trainer.seen == [("off", 0.0)] * 3
    assert all("train/grad_norm" not in h for h in m.log_history)
    assert "gradient_clip_val" not in DEFAULT_CONFIG["trainer"] and "gradient_clip_algorithm" not in DEFAULT_CONFIG["trainer"]


@pytest.mark.parametrize("val, algorithm, error", [(True, None, TypeError), ("1", None, TypeError), (1.0, "l2", ValueError)])
def test_fit_batches_refuses_a_bad_setting_before_the_first_step(val, algorithm, error):
    m = _StubModel(dict(_BASE, gradient_clip_val=0.5))
    with pytest.raises(error):
        m.fit_batches(list(range(3)), optimizer=_Opt(m), gradient_clip_val=val, gradient_clip_algorithm=algorithm)
    assert m.passes == 0 and m.global_step == 0 and m._trainer.set_calls == []
    assert m._clip_override is None and m._clip_fit is None and m._gradient_clip() == ("norm", 0.5)      # restored
    bad = {"gradient_clip_val": val}
    if algorithm is not None:
        bad["gradient_clip_algorithm"] = algorithm
    m = _StubModel(dict(_BASE, **bad))
    with pytest.raises(error):
        m.fit_batches(list(range(3)), optimizer=_Opt(m))
    assert m.passes == 0 and m._trainer.set_calls == []


def test_clip_gradients_arms_one_step_of_a_hand_written_loop():
    from music2midi_amd.training import Adafactor
    m = _StubModel(dict(_BASE, gradient_clip_val=0.5))
    tr = m._trainer
    tr.optimizer_step = lambda: tr.seen.append(tr.grad_clip)
    m._native_trainer = lambda *a, **k: tr
    opt = Adafactor(m)
    opt.step()                                             # a hand-written loop clips only what it asks for
    m.clip_gradients(opt)                                  # no arguments: the config's
    opt.step()
    opt.step()                                             # armed for ONE step
    m.clip_gradients(opt, gradient_clip_val=2.0, gradient_clip_algorithm="value")
    opt.step()
    assert tr.seen == [("off", 0.0), ("norm", 0.5), ("off", 0.0), ("value", 2.0)]
    with pytest.raises(TypeError):
        m.clip_gradients(opt, gradient_clip_val="2")
