"""CPU: gradient accumulation bookkeeping (music2midi_amd.accumulation) — where the 1/N scale, the accumulate flag, the optimizer
steps and the gradient all-reduces fall for pytorch-lightning 2.1.0's ``accumulate_grad_batches`` — and ``fit_batches`` driving it,
single-process and with gloo at world size 2 (one all-reduce per window)."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from music2midi_amd import distributed as D
from music2midi_amd.accumulation import MicroStep, check_accumulate_grad_batches, micro_step, windows
from music2midi_amd.config import ConfigNode, DEFAULT_CONFIG
from music2midi_amd.model import Music2MIDI


def _lightning_plan(n, length):
    """What Lightning 2.1.0's automatic optimisation does over `length` batches: (scale, accumulate, step) per batch."""
    out = []
    for i in range(length):
        pos = i % n
        last = i == length - 1
        out.append((1.0 / n, pos > 0, pos == n - 1 or last))
    return out


@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("length", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12])
def test_windows_follow_lightning(n, length):
    plan = list(windows(range(length), n))
    assert [b for b, _ in plan] == list(range(length))
    got = [(ms.grad_scale, ms.accumulate, ms.step) for _, ms in plan]
    assert got == _lightning_plan(n, length)
    assert all(ms.sync == ms.step for _, ms in plan)                      # the all-reduce goes with the optimizer step
    assert sum(ms.step for _, ms in plan) == -(-length // n)              # ceil: an incomplete last window still steps
    assert [ms.position for _, ms in plan] == [i % n for i in range(length)]
    if n == 1:                                                            # N = 1: the plain pass, every batch
        assert all(ms == MicroStep(0, 1.0, False, True) for _, ms in plan)


def test_windows_over_a_generator_and_an_empty_iterable():
    gen = (i for i in range(5))
    assert [ms.step for _, ms in windows(gen, 2)] == [False, True, False, True, True]
    assert list(windows([], 3)) == []


def test_micro_step():
    assert micro_step(3, 0) == MicroStep(0, 1 / 3, False, False)
    assert micro_step(3, 2) == MicroStep(2, 1 / 3, True, True)
    assert micro_step(3, 1, last=True).step
    with pytest.raises(ValueError):
        micro_step(3, 3)


@pytest.mark.parametrize("bad", [0, -1, 2.5, "4", True, None, 4.0])
def test_accumulate_grad_batches_must_be_a_positive_int(bad):
    with pytest.raises(ValueError):
        check_accumulate_grad_batches(bad)
    with pytest.raises(ValueError):
        list(windows(range(3), bad))
    assert check_accumulate_grad_batches(1) == 1 and check_accumulate_grad_batches(8) == 8


# ---- fit_batches with a stand-in trainer: the window logic of the real method, no GPU --------------------------------------
class _FakeTrainer:
    """What fit_batches touches of NativeTrainer: the flat gradient buffer, the sync stream, the step counter."""

    def __init__(self, n_floats=6):
        self.grads = torch.zeros(n_floats)
        self.sync_stream = None
        self.early_ranges = []
        self.step_count = 0
        self.passes = []                       # (grad_scale, accumulate) per training_step


class _StubModel(Music2MIDI):
    """Music2MIDI without the transformer: training_step adds a known gradient (scaled, accumulated) to the fake buffer."""

    def __init__(self, trainer_cfg, rank=0):
        torch.nn.Module.__init__(self)
        cfg = dict(DEFAULT_CONFIG)
        cfg["trainer"] = dict(trainer_cfg)
        self.config = ConfigNode(cfg)
        self._trainer = _FakeTrainer()
        self.rank = rank
        self.applied = []                      # the buffer the optimizer saw at each step

    def training_step(self, inputs, batch_idx):
        n = self._accumulation()
        ms = self._micro if self._micro is not None else micro_step(n, batch_idx % n)
        tr = self._trainer
        g = torch.full_like(tr.grads, float(inputs) + 100.0 * self.rank) * ms.grad_scale
        if ms.accumulate:
            tr.grads += g
        else:
            tr.grads.copy_(g)
        tr.passes.append((ms.grad_scale, ms.accumulate, self.global_step))
        return torch.tensor(float(inputs))


class _Opt:
    def __init__(self, model):
        self.model = model

    def step(self):
        self.model._trainer.step_count += 1
        self.model.applied.append(self.model._trainer.grads.clone())


def test_fit_batches_steps_once_per_window():
    m = _StubModel({"max_epochs": 1, "accumulate_grad_batches": 4, "log_every_n_steps": 1000})
    losses = m.fit_batches(list(range(10)), optimizer=_Opt(m))
    assert m.global_step == 3 and m._trainer.step_count == 3
    assert losses == [float(i) for i in range(10)]                        # unscaled, one per micro-batch
    assert [p[1] for p in m._trainer.passes] == [False, True, True, True] * 2 + [False, True]
    assert all(p[0] == 0.25 for p in m._trainer.passes)                   # 1/N, also in the incomplete last window
    assert [p[2] for p in m._trainer.passes] == [0] * 4 + [1] * 4 + [2] * 2      # global_step constant inside a window
    for applied, window in zip(m.applied, [range(0, 4), range(4, 8), range(8, 10)]):
        assert torch.allclose(applied, torch.full((6,), sum(window) / 4.0))


def test_fit_batches_override_and_config_default():
    m = _StubModel({"max_epochs": 1, "log_every_n_steps": 1000})          # key absent: N = 1
    m.fit_batches(list(range(5)), optimizer=_Opt(m))
    assert m.global_step == 5 and all(p[:2] == (1.0, False) for p in m._trainer.passes)
    m = _StubModel({"max_epochs": 1, "accumulate_grad_batches": 1, "log_every_n_steps": 1000})
    m.fit_batches(list(range(7)), optimizer=_Opt(m), accumulate_grad_batches=3)
    assert m.global_step == 3


@pytest.mark.parametrize("bad", [0, -1, 2.5, "4"])
def test_fit_batches_rejects_a_bad_accumulate_grad_batches_before_the_first_step(bad):
    m = _StubModel({"max_epochs": 1, "accumulate_grad_batches": bad, "log_every_n_steps": 1000})
    with pytest.raises(ValueError):
        m.fit_batches(list(range(3)), optimizer=_Opt(m))
    assert m._trainer.passes == [] and m.global_step == 0
    m = _StubModel({"max_epochs": 1, "log_every_n_steps": 1000})
    with pytest.raises(ValueError):
        m.fit_batches(list(range(3)), optimizer=_Opt(m), accumulate_grad_batches=bad)
    assert m._trainer.passes == []


def test_log_and_save_count_optimizer_steps(monkeypatch):
    m = _StubModel({"max_epochs": 1, "accumulate_grad_batches": 3, "log_every_n_steps": 2})
    monkeypatch.setattr(_StubModel, "logged_metrics", lambda self: {"train/loss": 0.0})
    saved = []
    monkeypatch.setattr(_StubModel, "save_checkpoint", lambda self, path, collective=True: saved.append(self.global_step))
    m.fit_batches(list(range(13)), optimizer=_Opt(m), save_path="unused", save_every_n_steps=2)
    assert m.global_step == 5
    assert [h["step"] for h in m.log_history] == [2, 4]
    assert saved == [2, 4, 5]                                             # every 2 optimizer steps (windows of 3) and at the end


# ---- gloo, world size 2: one gradient all-reduce per window -----------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    D.init_process_group("gloo")
    calls = []
    real = D.all_reduce_gradients

    def counting(flat):
        calls.append(1)
        return real(flat)

    D.all_reduce_gradients = counting
    m = _StubModel({"max_epochs": 1, "accumulate_grad_batches": 3, "log_every_n_steps": 1000}, rank=rank)
    m.fit_batches(list(range(7)), optimizer=_Opt(m))
    # windows [0, 1, 2], [3, 4, 5], [6]: the rank's gradient is (sum of batch values + 100 rank * len) / 3, averaged over ranks
    want = []
    for w in ([0, 1, 2], [3, 4, 5], [6]):
        want.append(sum((sum(w) + 100.0 * r * len(w)) / 3.0 for r in range(world)) / world)
    ok = len(calls) == 3 and m.global_step == 3 and all(torch.allclose(a, torch.full((6,), v)) for a, v in zip(m.applied, want))
    D.barrier()
    torch.distributed.destroy_process_group()
    q.put((rank, ok, len(calls), [float(a[0]) for a in m.applied], want))


def test_gloo_world2_one_gradient_all_reduce_per_window():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, ok, n_calls, got, want in results:
        assert ok, (rank, n_calls, got, want)


def test_the_fit_batches_override_holds_for_that_call_only():
    m = _StubModel({"max_epochs": 1, "accumulate_grad_batches": 2, "log_every_n_steps": 1000})
    m.fit_batches(list(range(6)), optimizer=_Opt(m), accumulate_grad_batches=3)
    assert m.global_step == 2 and m._accumulation() == 2 and m._accumulate_override is None
    with pytest.raises(ValueError):
        m.fit_batches(list(range(6)), optimizer=_Opt(m), accumulate_grad_batches=0)
    assert m._accumulation() == 2
