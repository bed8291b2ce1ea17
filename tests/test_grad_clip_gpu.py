"""GPU: gradient clipping in the Adafactor step — the norm kernels of csrc/grad_clip.hip and the CLIP forms of passes A, B and C of
csrc/adafactor.hip, behind NativeTrainer.set_grad_clip / optimizer_step / grad_stats / grad_norm — held to the clipped float64
reference of tests/grad_clip_cases.py: clip in float64, then adafactor_ref.ref_step.

Geometries: adafactor_ref's three (1.5, 2 and 4.5 trips of the 256-column loops; 258 row blocks with a last block of one row; 26 with a
last block of nine) and tiny_many_layers, 284 tensors: the second trip of the finish kernel's loops.  Cases: max_norm for a coefficient
near 0.3, near 1e-2 and of exactly 1, the value clamp at 0.05, and all-zero gradients; steps 9 998 - 10 001 from the primed state (a
warm-up step cannot see the coefficient).  As in tests/test_adafactor_gpu.py the smallest trainer is used and the synthetic gradients
are written into the flat buffer: no forward or backward pass is built.  The bars are 8x what the fp32 oracle needs against the same
reference (grad_clip_cases.*_FLOOR, measured by tests/test_grad_clip_cpu.py)."""
import copy
import math

import numpy as np
import pytest
import torch

import adafactor_ref as ar
import grad_clip_cases as gc
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.transformer import T5Transformer

pytestmark = pytest.mark.gpu


class _Device:
    """tests/test_adafactor_gpu.py's: one trainer of the smallest sizes and the case's initial parameters"""

    def __init__(self, geometry):
        from music2midi_amd.training import NativeTrainer
        cfg = gc.case_config(geometry)
        model = T5Transformer(cfg, precision="fp32")
        load_t5_state(model, gc.case_state_dict(geometry), strict=False)
        self.tr = NativeTrainer(model.cuda(), 1, 4, 2, precision="fp32")
        self.p0 = gc.case_params(geometry)
        self.shapes = {k: tuple(shape) for k, (_, shape) in self.tr.layout.items()}
        assert self.shapes == {k: tuple(self.p0[k].shape) for k in self.shapes} and len(self.shapes) == len(self.p0)
        with gc.one_thread():
            self.primed = ar.primed_state(self.p0)
        self._slices = {s[0]: s for s in self.tr._state_slices()}

    def reset(self):
        """the initial parameters and the primed second moments at step FIRST - 1; returns the float64 state the reference starts
        from: exactly the fp32 state the device imported"""
        tr = self.tr
        for k, (off, shape) in tr.layout.items():
            tr.params[off:off + self.p0[k].numel()].copy_(self.p0[k].reshape(-1))
        tr.grads.zero_()
        flat = torch.zeros(sum(sum(s) for s in self.shapes.values()), dtype=torch.float32)
        for name, shape, o_r, o_c in tr._state_slices():
            f = ar.state_flat(self.primed[name]).float()
            flat[o_r:o_r + f.numel()] = f
        tr.load_optimizer_state({"step": gc.FIRST - 1, "second_moments": flat})
        back = tr.optimizer_state()
        assert back["step"] == gc.FIRST - 1 == tr.step_count and torch.equal(back["second_moments"], flat)
        return {k: self._cut64(back["second_moments"], k) for k in self.shapes}

    def _cut64(self, flat, name):
        _, shape, o_r, o_c = self._slices[name]
        if o_c is None:
            return {"v": flat[o_r:o_r + shape[0]].double()}
        return {"row": flat[o_r:o_r + shape[0]].double(), "col": flat[o_c:o_c + shape[1]].double()}

    def write_grads(self, grads):
        for k, (off, shape) in self.tr.layout.items():
            self.tr.grads[off:off + grads[k].numel()].copy_(grads[k].reshape(-1))

    def step(self, grads, t):
        self.write_grads(grads)
        before = self.tr.grads.clone()
        self.tr.optimizer_step()
        assert self.tr.step_count == t
        assert torch.equal(self.tr.grads, before)                      # no pass writes the gradient buffer: .grad stays unclipped

    def get_params(self):
        flat = self.tr.params.cpu()
        return {k: flat[off:off + int(np.prod(shape))].view(shape).clone() for k, (off, shape) in self.tr.layout.items()}

    def get_state(self):
        flat = self.tr.optimizer_state()["second_moments"]
        return {name: flat[o_r:o_r + sum(shape)].clone() for name, shape, o_r, _ in self.tr._state_slices()}

    def get_words(self):
        return tuple(self.tr.grad_stats().tolist())


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


@pytest.mark.parametrize("case", gc.CASES)
@pytest.mark.parametrize("geometry", gc.GEOMETRIES)
def test_every_clipped_step_matches_the_float64_reference(devices, geometry, case):
    dev = devices(geometry)
    state64 = dev.reset()
    mode, value = gc.case_setting(dev.shapes, case)
    dev.tr.set_grad_clip(mode, value)
    where = f"clipped adafactor {geometry} {case}"
    before = dev.tr.params.clone()
    try:
        with gc.one_thread():
            upd, st, wn, wc, skipped = gc.run_clipped(dev.step, dev.get_params, dev.get_state, dev.get_words, dev.shapes, case, state64,
                                                      gc.bars(case), where)
    finally:
        dev.tr.set_grad_clip("off")
    for w in (upd, st, wn, wc):
        print(w.report(where))
    n_tensors, n = len(dev.shapes), (1 if case == "all_zero" else gc.N_STEPS)
    assert skipped == (n_tensors if case == "all_zero" else 1) * n
    assert len(upd.items) + skipped == n_tensors * n and len(st.items) == n_tensors * n
    assert len(wn.items) == len(wc.items) == (0 if mode == "value" else n)
    if case == "all_zero":
        assert torch.equal(dev.tr.params, before)                      # norm 0, coef 1 (the words' bars are 0), nothing moved
    for w in (upd, st, wn, wc):
        w.check(where)


@pytest.mark.parametrize("geometry", gc.GEOMETRIES)
def test_norm_words_are_deterministic_and_the_same_from_both_entry_points(devices, geometry):
    dev = devices(geometry)
    dev.reset()
    grads = ar.case_grads(dev.shapes, gc.FIRST)
    mode, value = gc.case_setting(dev.shapes, "norm_0.3")
    _, total, coef = gc.clip64(grads, mode, value)
    dev.write_grads(grads)
    off = dev.tr.grad_norm()                                           # clipping off: the coefficient is taken against +inf
    dev.tr.set_grad_clip(mode, value)
    try:
        first, second = dev.tr.grad_norm(), dev.tr.grad_norm(dev.tr.grads.clone())
        dev.tr.optimizer_step()
        own = dev.tr.grad_stats()
    finally:
        dev.tr.set_grad_clip("off")
    off, first, second, own = (w.cpu() for w in (off, first, second, own))
    print(f"{geometry}: norm {float(first[0]):.9g} (float64 {total:.9g}), coef {float(first[1]):.9g} (float64 {coef:.9g})")
    assert torch.equal(first, second) and torch.equal(first, own)      # bit for bit: two calls, another buffer, the step's own words
    assert float(off[0]) == float(first[0]) and float(off[1]) == 1.0
    assert gc.rel(float(first[0]), total) <= gc.bars("norm_0.3")["norm"]
    assert gc.rel(float(first[1]), coef) <= gc.bars("norm_0.3")["coef"]


def _two_steps(dev):
    dev.reset()
    for t in (gc.FIRST, gc.FIRST + 1):
        dev.step(ar.case_grads(dev.shapes, t), t)
    return dev.tr.params.clone(), dev.tr.optimizer_state()["second_moments"]


@pytest.mark.parametrize("geometry", ["full_1layer", "tiny_v4113"])
def test_a_coefficient_of_one_and_clipping_switched_off_again_are_the_unclipped_step(devices, geometry):
    """bit for bit: against a trainer that never set clipping"""
    never = _Device(geometry)
    try:
        want = _two_steps(never)
    finally:
        never.tr.close()
    dev = devices(geometry)
    dev.tr.set_grad_clip(*gc.case_setting(dev.shapes, "norm_1"))
    try:
        got = _two_steps(dev)
        assert dev.get_words()[1] == 1.0
    finally:
        dev.tr.set_grad_clip("off")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "coef = 1 changed the step"
    dev.tr.set_grad_clip("value", 0.05)
    dev.tr.set_grad_clip("off")
    got = _two_steps(dev)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "clipping switched off again changed the step"


def test_set_grad_clip_refuses_what_the_header_says(devices):
    from music2midi_amd import native
    tr = devices("tiny_v409").tr
    for mode, value in [("norm", 0.0), ("norm", -1.0), ("value", float("nan")), ("value", 0.0)]:
        with pytest.raises(native.NativeError):
            tr.set_grad_clip(mode, value)
    assert native.load().m2m_trainer_set_grad_clip(tr.handle, 3, 1.0) == -1
    with pytest.raises(ValueError):
        tr.set_grad_clip("l2", 1.0)
    assert tr.grad_clip == ("off", 0.0)
    tr.set_grad_clip("off", float("nan"))                              # off: the value is ignored


def test_an_infinite_gradient_element_is_not_special_cased(devices):
    dev = devices("tiny_v409")
    dev.reset()
    dev.write_grads(ar.case_grads(dev.shapes, gc.FIRST))
    g = dev.tr.grads.clone()
    off, shape = dev.tr.layout[ar.SMALL_TENSOR]
    g[off + 77] = float("inf")
    dev.tr.set_grad_clip("norm", 1.0)
    try:
        words = dev.tr.grad_norm(g).tolist()
    finally:
        dev.tr.set_grad_clip("off")
    assert words[0] == math.inf and words[1] == 0.0


# ---- end to end: trainer.gradient_clip_val through fit_batches ----------------------------------------------------------------
def _fit(batches, clip_in_config, **keywords):
    from music2midi_amd.model import Music2MIDI
    from test_t5_gpu import tiny_config
    cfg = tiny_config()
    cfg["dataloader"]["batch_size"] = 3
    cfg["trainer"]["log_every_n_steps"] = 3
    if clip_in_config is not None:
        cfg["trainer"]["gradient_clip_val"] = clip_in_config
    torch.manual_seed(5)
    m = Music2MIDI(copy.deepcopy(cfg)).cuda()
    m.train_precision = "fp32"
    m.fit_batches(batches, **keywords)
    assert m.global_step == 3
    return m


def test_fit_batches_honours_gradient_clip_val():
    from test_train_gpu import _notes_batches
    batches = _notes_batches(3)
    plain, by_config, by_keyword = _fit(batches, None), _fit(batches, 0.05), _fit(batches, None, gradient_clip_val=0.05)
    assert plain._trainer.grad_clip == ("off", 0.0) and by_config._trainer.grad_clip == ("norm", 0.05)
    names = [n for n, _ in plain.named_parameters()]
    differ = [n for (n, a), (_, b) in zip(plain.named_parameters(), by_config.named_parameters()) if not torch.equal(a, b)]
    print(f"{len(differ)} of {len(names)} tensors differ between the clipped and the unclipped run")
    assert len(differ) > len(names) // 2
    for (n, a), (_, b) in zip(by_config.named_parameters(), by_keyword.named_parameters()):
        assert torch.equal(a, b), n
    assert all("train/grad_norm" not in h for h in plain.log_history)
    for m in (by_config, by_keyword):
        assert [h["step"] for h in m.log_history] == [3]
        norm = m.log_history[0]["train/grad_norm"]
        print(f"train/grad_norm at step 3: {norm:.6g}")
        assert math.isfinite(norm) and norm > 0.05                     # (the pre-clip norm: the clip was active)
    assert by_config.log_history[0]["train/grad_norm"] == by_keyword.log_history[0]["train/grad_norm"]
