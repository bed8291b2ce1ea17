"""CPU: the floor and the power of the Adafactor update metric (tests/adafactor_ref.py).

Floor: what the fp32 AdafactorOracle (oracle/train.py, pinned to HuggingFace by the `train` golden) needs against the float64
restatement, per regime, on the cases the GPU test runs; the recorded floors (UPDATE_FLOOR / STATE_FLOOR) are what the device bar is
derived from.  Power: eight deliberately wrong steps, each of which must show at more than 100x the device bar."""
import functools

import pytest
import torch

import adafactor_ref as ar
from oracle.train import AdafactorOracle


class _Oracle:
    """AdafactorOracle behind the three callables of adafactor_ref.run_steps"""

    def __init__(self, params, state64=None, step=0):
        self.params = {k: v.clone() for k, v in params.items()}
        self.opt = AdafactorOracle(self.params)
        if state64 is not None:
            for k, s in state64.items():
                self.opt.state[k] = dict({"step": step}, **{n: v.float() for n, v in s.items()})

    def step(self, grads, t):
        self.opt.step(grads)
        assert all(s["step"] == t for s in self.opt.state.values())

    def get_params(self):
        return {k: v.clone() for k, v in self.params.items()}

    def get_state(self):
        return {k: (torch.cat([s["row"].reshape(-1), s["col"].reshape(-1)]) if "row" in s else s["v"].reshape(-1).clone())
                for k, s in self.opt.state.items()}


@functools.lru_cache(maxsize=None)
def _params(geometry):
    return ar.case_params(geometry)


@functools.lru_cache(maxsize=None)
def _primed(geometry):
    return ar.primed_state(_params(geometry))


@functools.lru_cache(maxsize=None)
def _measure(geometry, regime):
    """(oracle's worst update error, worst state error, skipped pairs, {mutant: (worst error, worst error on SMALL_TENSOR)}); the
    mutants are applied at the regime's last step, to the reference's own inputs of that step"""
    params = _params(geometry)
    shapes = {k: tuple(v.shape) for k, v in params.items()}
    first, n, _ = ar.REGIMES[regime]
    if regime == "warmup":
        side, state64 = _Oracle(params), {k: ar.fresh_state(s) for k, s in shapes.items()}
    else:
        side, state64 = _Oracle(params, _primed(geometry), first - 1), dict(_primed(geometry))
    mutants = {m: [0.0, 0.0] for m in ar.MUTANTS}

    def probe(t, k, p_old, g, before, delta):
        if t != first + n - 1 or float(delta.abs().max()) == 0.0:
            return
        for m in ar.MUTANTS:
            d_m, _ = ar.ref_step(p_old, g, before, t, mutant=m)
            e = ar.update_error((p_old.double() + d_m).float(), p_old, delta)
            mutants[m][0] = max(mutants[m][0], e)
            if k == ar.SMALL_TENSOR:
                mutants[m][1] = max(mutants[m][1], e)

    where = f"oracle {geometry} {regime}"
    upd, st, skipped, _ = ar.run_steps(side.step, side.get_params, side.get_state, shapes, regime, state64,
                                       ar.UPDATE_FLOOR[regime], ar.STATE_FLOOR[regime], where, probe=probe)
    print(upd.report(where))
    print(st.report(where))
    return upd, st, skipped, {m: tuple(v) for m, v in mutants.items()}, len(shapes)


@pytest.mark.parametrize("regime", list(ar.REGIMES))
@pytest.mark.parametrize("geometry", ar.GEOMETRIES)
def test_fp32_oracle_stays_within_the_recorded_floors(geometry, regime):
    upd, st, skipped, _, n_tensors = _measure(geometry, regime)
    where = f"oracle {geometry} {regime}"
    first, n, all_zero = ar.REGIMES[regime]
    assert skipped == (n_tensors if all_zero else 1) * n            # only ZERO_TENSOR, or every tensor of the all-zero step
    assert len(upd.items) + skipped == n_tensors * n and len(st.items) == n_tensors * n
    upd.check(where)
    st.check(where)


def test_recorded_floors_are_the_measured_ones():
    """the constants are the worst over the geometries, rounded up to two digits (not a looser number)"""
    for regime in ar.REGIMES:
        u = max(_measure(g, regime)[0].worst() for g in ar.GEOMETRIES)
        s = max(_measure(g, regime)[1].worst() for g in ar.GEOMETRIES)
        print(f"{regime}: measured update floor {u:.3e} (recorded {ar.UPDATE_FLOOR[regime]:.3e}), state floor {s:.3e} "
              f"(recorded {ar.STATE_FLOOR[regime]:.3e})")
        assert u <= ar.UPDATE_FLOOR[regime] <= 1.05 * u, regime
        assert s <= ar.STATE_FLOOR[regime] <= 1.05 * s, regime


@pytest.mark.parametrize("mutant", ar.MUTANTS)
def test_the_metric_sees_a_wrong_update(mutant):
    """each wrong step exceeds 100x the device bar of its regime on at least one case; the missing 1/sqrt(t) cap in a late regime,
    the missing 1e-3 floor on the small-parameter tensor"""
    regimes = [r for r in ar.REGIMES if r != "all_zero"]
    if mutant == "rho_without_cap":
        regimes = ["late_10k", "late_40k"]
    seen = {}
    for regime in regimes:
        for g in ar.GEOMETRIES:
            e_all, e_small = _measure(g, regime)[3][mutant]
            seen[(g, regime)] = (e_small if mutant == "no_rms_floor" else e_all) / (100.0 * ar.update_bar(regime))
    best = max(seen, key=seen.get)
    print(f"{mutant}: {seen[best]:.3g} x (100 x device bar) on {best}")
    assert seen[best] > 1.0, seen
