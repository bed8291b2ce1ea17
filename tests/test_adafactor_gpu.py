"""GPU: the Adafactor kernels (csrc/adafactor.hip, behind NativeTrainer.optimizer_step) held step by step to the float64
restatement of tests/adafactor_ref.py, at every column width of the real model and every row-block count the kernels loop over:

  full_1layer  default widths, one encoder + one decoder layer: 384 / 512 / 1152 columns (1.5, 2 and 4.5 trips of the 256-column
               loops of passes A, A2, B and C), 72 row blocks
  tiny_v4113   4113 vocabulary rows: 258 row blocks, the last holding ONE row (the second trip of the 256-block strides of passes A2
               and B2; the 8-way unrolled column-partial loop ends on a tail of 2)
  tiny_v409    409 rows: 26 blocks, the last holding 9 rows

and in every step regime: warm-up from a fresh state, steps 9 998 - 10 001 (rho = min(1e-6 t, 1/sqrt(t)) changes branch at 10 000) and
40 000 - 40 001 from a host-built state through load_optimizer_state, and one step of all-zero gradients.  Gradients are synthetic
(adafactor_ref.case_grads: scales 1e-2 .. 10, rows 5-18 of the larger matrices exactly zero, one tensor's gradient zero throughout, one
tensor's parameters scaled under the max(1e-3, rms(p)) floor); no forward or backward pass is built.  The bars are 8x what the fp32
oracle needs against the same reference (adafactor_ref.UPDATE_FLOOR / STATE_FLOOR, measured by tests/test_adafactor_cpu.py)."""
import numpy as np
import pytest
import torch

import adafactor_ref as ar
from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

pytestmark = pytest.mark.gpu


class _Device:
    """one trainer of the smallest sizes it accepts (one clip, two frames after the conditioning rows, two labels) and the case's
    initial parameters; the three callables of adafactor_ref.run_steps"""

    def __init__(self, geometry):
        from music2midi_amd.training import NativeTrainer
        cfg = ar.case_config(geometry)
        geom = T5Geometry(load_config(cfg).model.t5)
        sd = synth.t5_state_dict(geom, seed=0)
        synth.perturb_layer_norms(sd, 0)
        model = T5Transformer(cfg, precision="fp32")
        load_t5_state(model, sd, strict=False)
        self.tr = NativeTrainer(model.cuda(), 1, 4, 2, precision="fp32")
        self.p0 = ar.case_params(geometry)
        self.shapes = {k: tuple(shape) for k, (_, shape) in self.tr.layout.items()}
        assert self.shapes == {k: tuple(self.p0[k].shape) for k in self.shapes} and len(self.shapes) == len(self.p0)
        self.primed = ar.primed_state(self.p0)
        self._slices = {s[0]: s for s in self.tr._state_slices()}

    def reset(self, state64, step):
        """the initial parameters, and the second moments of state64 (None: a fresh state) loaded at `step`; returns the float64 state the
        reference starts from: exactly the fp32 state the device imported"""
        tr = self.tr
        for k, (off, shape) in tr.layout.items():
            tr.params[off:off + self.p0[k].numel()].copy_(self.p0[k].reshape(-1))
        tr.grads.zero_()
        n = sum(sum(s) for s in self.shapes.values())
        flat = torch.zeros(n, dtype=torch.float32)
        if state64 is not None:
            for name, shape, o_r, o_c in tr._state_slices():
                f = ar.state_flat(state64[name]).float()
                flat[o_r:o_r + f.numel()] = f
        if state64 is not None or tr.step_count != 0:
            tr.load_optimizer_state({"step": step, "second_moments": flat})
        back = tr.optimizer_state()
        assert back["step"] == step == tr.step_count and torch.equal(back["second_moments"], flat)      # bit-equal to what was loaded
        return {k: self._cut64(back["second_moments"], k) for k in self.shapes}

    def _cut64(self, flat, name):
        _, shape, o_r, o_c = self._slices[name]
        if o_c is None:
            return {"v": flat[o_r:o_r + shape[0]].double()}
        return {"row": flat[o_r:o_r + shape[0]].double(), "col": flat[o_c:o_c + shape[1]].double()}

    def step(self, grads, t):
        for k, (off, shape) in self.tr.layout.items():
            self.tr.grads[off:off + grads[k].numel()].copy_(grads[k].reshape(-1))
        self.tr.optimizer_step()
        assert self.tr.step_count == t

    def get_params(self):
        flat = self.tr.params.cpu()
        return {k: flat[off:off + int(np.prod(shape))].view(shape).clone() for k, (off, shape) in self.tr.layout.items()}

    def get_state(self):
        flat = self.tr.optimizer_state()["second_moments"]
        return {name: flat[o_r:o_r + sum(shape)].clone() for name, shape, o_r, _ in self.tr._state_slices()}


@pytest.fixture(scope="module")
def devices():
    made = {}

    def get(geometry):
        if geometry not in made:
            made[geometry] = _Device(geometry)
        return made[geometry]
    yield get
    for d in made.values():
        d.tr.close()


@pytest.mark.parametrize("regime", list(ar.REGIMES))
@pytest.mark.parametrize("geometry", ar.GEOMETRIES)
def test_every_step_matches_the_float64_reference(devices, geometry, regime):
    dev = devices(geometry)
    first, n, all_zero = ar.REGIMES[regime]
    state64 = dev.reset(None if regime == "warmup" else dev.primed, first - 1)
    where = f"adafactor {geometry} {regime}"
    before = dev.tr.params.clone()
    upd, st, skipped, _ = ar.run_steps(dev.step, dev.get_params, dev.get_state, dev.shapes, regime, state64,
                                       ar.update_bar(regime), ar.state_bar(regime), where)
    print(upd.report(where) + f" (oracle's floor {ar.UPDATE_FLOOR[regime]:.1e})")
    print(st.report(where) + f" (oracle's floor {ar.STATE_FLOOR[regime]:.1e})")
    # coverage: every (tensor, step) pair is measured; only an exactly-zero float64 update is held to bit-identity instead
    n_tensors = len(dev.shapes)
    assert skipped == (n_tensors if all_zero else 1) * n
    assert len(upd.items) + skipped == n_tensors * n and len(st.items) == n_tensors * n
    assert dev.tr.step_count == first + n - 1
    if all_zero:
        assert torch.equal(dev.tr.params, before)                 # every parameter (and the padding between tensors) bit-identical
    upd.check(where)
    st.check(where)
