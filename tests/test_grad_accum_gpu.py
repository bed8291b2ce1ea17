"""GPU: gradient accumulation (m2m_train_forward_backward_acc / NativeTrainer.forward_backward(grad_scale=, accumulate=) /
fit_batches with accumulate_grad_batches) against autograd over the oracle (oracle/train.py), as tests/test_train_gpu.py does for
the single pass.  Every gradient writer must ADD in accumulate mode: before each accumulating pass the buffer gets a known non-zero
pattern on top of what it holds, subtracted afterwards — a writer that still overwrites shows up as a tensor off by the pattern."""
import copy
import types

import numpy as np
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.config import DEFAULT_CONFIG

import adafactor_ref as ar
from test_t5_gpu import tiny_config
from test_train_gpu import FP8_FLOORS, _notes_batches, _rel, _setup, fp8_agreement

pytestmark = pytest.mark.gpu

N = 3
# (B, F, Ld) of the three micro-batches: different clip counts and label lengths in one window
SHAPES = [(3, 21, 14), (2, 30, 9), (3, 21, 17)]
MAX = (3, 32, 17)


def _micro(geom, B, F, Ld, seed):
    feats = torch.from_numpy(synth.normal(300 + seed, "acc_feats", (B, F, geom.d_model), 2.0))
    cond = torch.from_numpy(synth.cond_index_batch(310 + seed, B))
    labels = torch.from_numpy((synth.uniform01(320 + seed, "acc_labels", B * Ld) * 330).astype(np.int64).reshape(B, Ld)) + 3
    labels[B - 1, Ld - 3:] = -100
    x = torch.zeros((B, F + 2, geom.d_model))
    x[:, 2:] = feats
    return x, feats, cond, labels


def _pattern(n, seed):
    return torch.from_numpy(synth.normal(900 + seed, "acc_pattern", (n,), 1.0)).cuda()


def _window(tr, micros, pattern_scale=1.0):
    """N micro-batches through the trainer, the buffer NaN before the first and pattern-shifted before the others; returns the
    accumulated buffer and the unscaled losses."""
    losses = []
    tr.grads.fill_(float("nan"))
    for i, (x, _, cond, labels) in enumerate(micros):
        pat = None
        if i:
            pat = _pattern(tr.n_floats, i) * pattern_scale
            tr.grads.add_(pat)
        loss, _ = tr.forward_backward(x.cuda(), cond.cuda(), labels.cuda(), grad_scale=1.0 / len(micros), accumulate=i > 0)
        losses.append(loss.item())
        if pat is not None:
            tr.grads.sub_(pat)
    return tr.grads.clone(), losses


def _oracle_sum(orc, micros, masks=None):
    total, losses = None, []
    for i, (_, feats, cond, labels) in enumerate(micros):
        loss_o, _, g = orc.loss_and_grads(feats, cond, labels, masks(i)) if masks else orc.loss_and_grads(feats, cond, labels)
        losses.append(loss_o.item())
        total = {k: v.clone() for k, v in g.items()} if total is None else {k: total[k] + g[k] for k in total}
    return {k: v / len(micros) for k, v in total.items()}, losses


@pytest.mark.parametrize("dropout", [0.0, 0.1])
def test_fp32_accumulated_gradients_and_step_match_the_oracle(dropout):
    from oracle.train import AdafactorOracle, DropoutMasks
    model, tr, orc, params, geom, *_ = _setup(tiny_config(), "fp32", *SHAPES[0], max_sizes=(MAX[0], MAX[1] + 2, MAX[2]))
    micros = [_micro(geom, B, F, Ld, i) for i, (B, F, Ld) in enumerate(SHAPES)]
    if dropout:
        tr.set_dropout(dropout, seed=4321)
    acc, losses = _window(tr, micros)
    ref, losses_o = _oracle_sum(orc, micros, (lambda i: DropoutMasks(dropout, 4321, i)) if dropout else None)
    for l, lo in zip(losses, losses_o):                                  # the returned loss is the unscaled one
        assert abs(l - lo) < 1e-4 * max(1.0, abs(lo)), (losses, losses_o)
    worst = {}
    for name, (off, shape) in tr.layout.items():
        worst[name] = _rel(acc[off:off + int(np.prod(shape))].view(shape).cpu(), ref[name])
    bad = {k: v for k, v in worst.items() if not v <= 1e-4}
    print(f"fp32 N={N} dropout {dropout}: worst accumulated gradient rel err {max(worst.values()):.2e} over {len(worst)} tensors")
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
    # one Adafactor step from the accumulated buffer gives the oracle's parameters
    tr.grads.copy_(acc)
    p_ref = {k: v.detach().clone() for k, v in params.items()}
    AdafactorOracle(p_ref).step(ref)
    p_old = tr.params.cpu()
    tr.optimizer_step()
    worst_p = max(_rel(tr.params[off:off + int(np.prod(shape))].view(shape).cpu(), p_ref[k]) for k, (off, shape) in tr.layout.items())
    print(f"  after one Adafactor step: worst parameter rel err {worst_p:.2e}")
    assert worst_p < 2e-5
    # the line above is the size of the step itself (lr = rms(p) 1e-6 at t = 1): also resolve the update, per tensor, against the
    # float64 step from the device's own parameters and accumulated gradient (tests/adafactor_ref.py; the bar of test_adafactor_gpu.py)
    p_new, g_dev = tr.params.cpu(), acc.cpu()
    upd = ar.Worst("update error", ar.update_bar("warmup"))
    for k, (off, shape) in tr.layout.items():
        old, new, g = (b[off:off + int(np.prod(shape))].view(shape) for b in (p_old, p_new, g_dev))
        delta, _ = ar.ref_step(old, g, ar.fresh_state(tuple(shape)), 1)
        e = ar.update_error(new, old, delta)
        if e is None:                                                    # an all-zero gradient: nothing may move
            assert torch.equal(new, old), k
        else:
            upd.add(e, k, 1)
    print("  " + upd.report("that step against the float64 update"))
    assert len(upd.items) == len(tr.layout)                             # (every tensor has a gradient in a real pass)
    upd.check("accumulated step")


def test_bf16_accumulated_gradients_track_the_fp32_oracle():
    model, tr, orc, params, geom, *_ = _setup(tiny_config(), "bf16", *SHAPES[0], max_sizes=(MAX[0], MAX[1] + 2, MAX[2]))
    micros = [_micro(geom, B, F, Ld, i) for i, (B, F, Ld) in enumerate(SHAPES)]
    acc, losses = _window(tr, micros)
    ref, losses_o = _oracle_sum(orc, micros)
    for l, lo in zip(losses, losses_o):
        assert abs(l - lo) < 2e-2 * abs(lo)
    cos_min, worst = 1.0, 0.0
    for name, (off, shape) in tr.layout.items():
        g = acc[off:off + int(np.prod(shape))].cpu().double()
        r = ref[name].reshape(-1).double()
        if r.norm() < 1e-12:
            continue
        cos_min = min(cos_min, float(torch.dot(g, r) / (g.norm() * r.norm() + 1e-30)))
        worst = max(worst, float((g - r).norm() / r.norm()))
    print(f"bf16 N={N}: min cosine {cos_min:.5f}, worst rel l2 {worst:.3e}")
    assert cos_min > 0.995 and worst < 0.1


def test_fp8_accumulated_gradients_track_the_mx_emulating_oracle():
    model, tr, orc, params, geom, *_ = _setup(tiny_config(), "fp8", *SHAPES[0], max_sizes=(MAX[0], MAX[1] + 2, MAX[2]))
    micros = [_micro(geom, B, F, Ld, i) for i, (B, F, Ld) in enumerate(SHAPES)]
    acc, losses = _window(tr, micros)
    x0, _, c0, l0 = micros[0]
    plain, _ = tr.forward_backward(x0.cuda(), c0.cuda(), l0.cuda())
    assert plain.item() == losses[0]                                     # the forward pass is the plain pass's, bit for bit
    ref_plain, losses_plain = _oracle_sum(orc, micros)
    orc.mx8, orc.mx8_dw, orc.bf16 = True, False, True
    ref_emul, losses_emul = _oracle_sum(orc, micros)
    view = types.SimpleNamespace(layout=tr.layout, grads=acc)
    cmin, cmed, worst = fp8_agreement(view, ref_emul)
    pmin, pmed, _ = fp8_agreement(view, ref_plain)
    print(f"fp8 N={N}: cosine vs the emulating oracle min {cmin:.4f} / median {cmed:.4f}; vs fp32 min {pmin:.4f} / median {pmed:.4f}")
    # (the loss is the forward pass alone, unchanged by accumulation — checked bit for bit above; on these inputs one micro-batch
    # measured 1.2 % from the emulation, past the 1 % the single-batch fp8 test holds at its own inputs, so both bars are 3 %)
    for l, le, lp in zip(losses, losses_emul, losses_plain):
        assert abs(l - le) < 3e-2 * abs(le) and abs(l - lp) < 3e-2 * abs(lp), (losses, losses_emul, losses_plain)
    floor = FP8_FLOORS["tiny"]
    assert cmin > floor[0] and cmed > floor[1], (cmin, cmed, floor)
    assert pmin > floor[2] and pmed > floor[3], (pmin, pmed, floor)


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp8"])
def test_accumulate_graph_replay_equals_direct_issue_and_split_releases_final_values(precision, monkeypatch):
    """Per micro-batch, over three windows (the second call of each (shape, mode) captures, later ones replay): the captured graph
    equals direct issue bit for bit in both modes; the split backward gives the same bits and its early ranges are final — the
    ACCUMULATED values — when the sync stream is released."""
    from music2midi_amd import distributed as D
    from music2midi_amd.training import NativeTrainer
    model, tr_graph, orc, params, geom, *_ = _setup(tiny_config(), precision, *SHAPES[0], max_sizes=(MAX[0], MAX[1] + 2, MAX[2]))
    monkeypatch.setenv("M2M_TRAIN_GRAPH", "0")
    tr_direct = NativeTrainer(model, MAX[0], MAX[1] + 2, MAX[2], precision=precision)
    monkeypatch.delenv("M2M_TRAIN_GRAPH")
    tr_split = NativeTrainer(model, MAX[0], MAX[1] + 2, MAX[2], precision=precision)
    sync = torch.cuda.Stream()
    tr_split.set_sync_stream(sync)
    early, _ = D.split_ranges(tr_split.n_floats, tr_split.early_ranges)
    trs = (tr_graph, tr_direct, tr_split)
    for tr in trs:
        tr.set_dropout(0.1, seed=99)
        tr.grads.fill_(float("nan"))
    for window in range(3):
        micros = [_micro(geom, B, F, Ld, 10 * window + i) for i, (B, F, Ld) in enumerate(SHAPES[:2])]
        for i, (x, _, cond, labels) in enumerate(micros):
            outs = []
            for tr in trs:
                loss, _ = tr.forward_backward(x.cuda(), cond.cuda(), labels.cuda(), grad_scale=0.5, accumulate=i > 0)
                if tr is tr_split:
                    with torch.cuda.stream(sync):                          # what an all-reduce on the sync stream would read
                        snap = [tr.grads[o:o + c].clone() for o, c in early]
                outs.append(loss.item())
            torch.cuda.synchronize()
            assert outs[0] == outs[1] == outs[2], (window, i, outs)
            assert torch.equal(tr_graph.grads, tr_direct.grads), f"window {window} micro {i}: graph replay differs from direct issue"
            assert torch.equal(tr_split.grads, tr_direct.grads), f"window {window} micro {i}: split pass differs"
            assert not torch.isnan(tr_graph.grads).any()
            for (o, c), sn in zip(early, snap):
                assert torch.equal(sn, tr_split.grads[o:o + c]), f"window {window} micro {i}: range ({o}, {c}) not final at the release"
    assert tr_graph.graph_nodes() > 0
    for tr in trs:
        tr.close()


def _music2midi(cfg, precision="fp32"):
    from music2midi_amd.model import Music2MIDI
    torch.manual_seed(5)
    m = Music2MIDI(copy.deepcopy(cfg)).cuda()
    m.train_precision = precision
    return m


def _fit_cfg(n):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["dataloader"]["batch_size"] = 3
    cfg["trainer"]["log_every_n_steps"] = 1000                  # no greedy decode inside the steps
    if n is None:
        del cfg["trainer"]["accumulate_grad_batches"]
    else:
        cfg["trainer"]["accumulate_grad_batches"] = n
    return cfg


def test_fit_batches_accumulates_four_batches_per_step_and_resumes_bit_for_bit(tmp_path):
    """accumulate_grad_batches = 4 over 10 batches: 3 optimizer steps (windows 4, 4, 2 — the last one incomplete, still 1/4), the
    parameters of the same windows composed by hand from plain passes, the unscaled per-batch losses, and a run resumed from the
    checkpoint at the second window boundary equal to the uninterrupted one bit for bit (dropout on)."""
    batches = _notes_batches(10)
    m = _music2midi(_fit_cfg(4))
    losses = m.fit_batches(batches)
    assert m.global_step == 3 and m._trainer.step_count == 3 and len(losses) == 10

    # the same windows by hand: overwrite passes, gradients summed / 4 in torch, one optimizer step per window
    h = _music2midi(_fit_cfg(1))
    losses_h = []
    for w in (batches[0:4], batches[4:8], batches[8:10]):
        total = None
        for b in w:
            losses_h.append(h.training_step(b, 0).item())
            g = h._trainer.grads.clone()
            total = g if total is None else total + g
        h._trainer.grads.copy_(total / 4)
        h._trainer.optimizer_step()
        h.global_step += 1
    assert losses[:4] == losses_h[:4]                            # same parameters, same passes: the unscaled losses bit for bit
    assert all(abs(a - b) < 1e-4 * abs(b) for a, b in zip(losses, losses_h)), (losses, losses_h)
    worst = max(_rel(p1.detach().cpu(), p2.detach().cpu()) for p1, p2 in zip(m.parameters(), h.parameters()))
    print(f"fit_batches N=4 vs windows composed by hand: worst parameter rel err {worst:.2e}")
    assert worst < 1e-4

    # resume at a window boundary
    ck = tmp_path / "w2.ckpt"
    first = _music2midi(_fit_cfg(4))
    losses_a = first.fit_batches(batches[:8], save_path=ck)
    assert first.global_step == 2
    second = _music2midi(_fit_cfg(4))
    losses_b = second.fit_batches(batches[8:], ckpt_path=ck)
    assert second.global_step == 3 and second._trainer.step_count == 3
    assert losses_a + losses_b == losses
    for (n1, p1), (n2, p2) in zip(m.named_parameters(), second.named_parameters()):
        assert n1 == n2 and torch.equal(p1, p2), n1


def test_accumulate_grad_batches_one_is_the_plain_run():
    """N = 1 (explicit) is the run with the key absent: losses, parameters and the ids generated afterwards, bit for bit."""
    batches = _notes_batches(3)
    runs = []
    for n in (None, 1):
        m = _music2midi(_fit_cfg(n), precision="bf16")
        losses = m.fit_batches(batches)
        single = m.training_step(batches[0], 7).item()
        m.eval()
        ids = m.model.generate(batches[0], max_length=10).cpu()
        runs.append((losses, single, [p.detach().clone() for p in m.parameters()], ids, m.global_step))
    (la, sa, pa, ia, ga), (lb, sb, pb, ib, gb) = runs
    assert la == lb and sa == sb and ga == gb == 3
    assert all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert torch.equal(ia, ib)


def _long_notes_batch(seed, B=3, n_notes=40):
    """A batch whose labels run past the trainer's 64-position floor (a decoder length the first batches never reach)."""
    notes = []
    for b in range(B):
        u = synth.uniform01(500 + seed, f"long{b}", n_notes * 3).reshape(n_notes, 3)
        on = np.sort(u[:, 0] * 2.5)
        notes.append(np.stack([on, on + 0.05 + u[:, 1] * 0.4, np.floor(40 + u[:, 2] * 40), np.full(n_notes, 80.0)], axis=1))
    from music2midi_amd.input import ModelInputs
    wav = torch.from_numpy(synth.waveform_batch(600 + seed, B, 48000, "music")).cuda()
    idx = torch.from_numpy(synth.cond_index_batch(610 + seed, B)).cuda()
    return ModelInputs(input_waveform=wav, notes_batch=tuple(notes), cond_index=idx)


def test_a_trainer_rebuilt_inside_a_window_keeps_the_window_gradients_and_masks():
    """The second micro-batch of a window has longer labels than any before: the trainer is rebuilt for it in the middle of the
    window.  The gradients of the first micro-batch must survive the rebuild and the dropout masks must continue (dropout on):
    the step equals the same window through a trainer built large enough from the start, composed by hand from plain passes."""
    small = _notes_batches(1)[0]
    big = _long_notes_batch(0)
    m = _music2midi(_fit_cfg(2))
    assert m._labels(big.notes_batch).shape[1] > 64 >= m._labels(small.notes_batch).shape[1]
    losses = m.fit_batches([small, big])
    assert m._trainer.limits[2] > 64 and m.global_step == 1 and m._train_passes == 2      # rebuilt once, one step
    h = _music2midi(_fit_cfg(1))
    x = h.model.encoder_inputs(big)
    h._native_trainer(x.shape[0], x.shape[1], h._labels(big.notes_batch).shape[1])          # large from the start: no rebuild
    limits = h._trainer.limits
    total, losses_h = None, []
    for b in (small, big):
        losses_h.append(h.training_step(b, 0).item())
        g = h._trainer.grads.clone()
        total = g if total is None else total + g
    assert h._trainer.limits == limits
    h._trainer.grads.copy_(total / 2)
    h._trainer.optimizer_step()
    assert losses == losses_h, (losses, losses_h)                                        # same weights, same masks: same bits
    worst = max(_rel(p1.detach().cpu(), p2.detach().cpu()) for p1, p2 in zip(m.parameters(), h.parameters()))
    print(f"rebuild inside a window: worst parameter rel err {worst:.2e} against the unrebuilt window")
    assert worst < 1e-5


def test_fit_batches_with_accumulation_matches_the_oracle_and_logs_unscaled_losses():
    """accumulate_grad_batches = 4 over 10 batches in fp32 (dropout off): per window, autograd over the oracle on the same encoder
    inputs and labels, Σ gradients / 4 (also for the incomplete last window) and AdafactorOracle — the parameters after the three
    steps are the oracle's.  log_every_n_steps = 1: every step logs the unscaled loss of the window's last micro-batch."""
    from oracle.train import AdafactorOracle, T5TrainOracle, leaf_params
    from music2midi_amd.config import T5Geometry, load_config
    cfg = _fit_cfg(4)
    cfg["model"]["t5"]["dropout_rate"] = 0.0
    cfg["trainer"]["log_every_n_steps"] = 1
    batches = _notes_batches(10)
    m = _music2midi(cfg)
    geom = T5Geometry(load_config(copy.deepcopy(cfg)).model.t5)
    params = leaf_params({k: v.detach().cpu().numpy() for k, v in m.model.named_parameters()})
    p_ref = {k: v.detach().clone() for k, v in params.items()}
    orc, opt = T5TrainOracle(geom, params), AdafactorOracle(p_ref)
    n_cond = len(m.model.conditioning.embeds)
    inputs = [(m.model.encoder_inputs(b)[:, n_cond:].cpu(), b.cond_index.cpu(), m._labels(b.notes_batch)) for b in batches]
    losses = m.fit_batches(batches)
    assert m.global_step == 3 and m._trainer.step_count == 3
    losses_o = []
    for w in (inputs[0:4], inputs[4:8], inputs[8:10]):
        total = None
        for feats, cond, labels in w:
            loss_o, _, g = orc.loss_and_grads(feats, cond, labels)
            losses_o.append(loss_o.item())
            total = {k: v.clone() for k, v in g.items()} if total is None else {k: total[k] + g[k] for k in total}
        opt.step({k: v / 4 for k, v in total.items()})
        with torch.no_grad():
            for k in params:
                params[k].copy_(p_ref[k])
    assert all(abs(a - b) < 1e-4 * max(1.0, abs(b)) for a, b in zip(losses, losses_o)), (losses, losses_o)
    own = dict(m.model.named_parameters())
    worst = max(_rel(own[k].detach().cpu(), p_ref[k]) for k in p_ref)
    print(f"fit_batches N=4 x 10 batches vs the oracle: worst parameter rel err {worst:.2e}")
    assert worst < 1e-4
    assert [h["step"] for h in m.log_history] == [1, 2, 3]
    for h, last in zip(m.log_history, (3, 7, 9)):
        assert h["train/loss"] == pytest.approx(losses[last], rel=1e-6), (h, losses)


def _large_window_check(precision):
    """16 clips x S = 261 x 256 labels, full model, N = 2 under the NaN + pattern check: the accumulated buffer equals the two plain
    passes' gradients summed / 2 (a power of two: the scaled backward is the plain one times 1/2)."""
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.config import T5Geometry, load_config
    from music2midi_amd.training import NativeTrainer
    from music2midi_amd.transformer import T5Transformer
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    geom = T5Geometry(load_config(copy.deepcopy(cfg)).model.t5)
    model = T5Transformer(cfg, precision="fp32")
    load_t5_state(model, synth.t5_state_dict(geom, seed=0), strict=False)
    model = model.cuda()
    B, S, Ld = 16, 261, 256
    tr = NativeTrainer(model, B, S, Ld, precision=precision)
    micros = []
    for i in range(2):
        x = torch.from_numpy(synth.normal(700 + i, "x", (B, S, geom.d_model), 2.0))
        cond = torch.from_numpy(synth.cond_index_batch(710 + i, B))
        labels = torch.from_numpy((synth.uniform01(720 + i, "l", B * Ld) * 330).astype(np.int64).reshape(B, Ld)) + 3
        labels[3, 200:] = -100
        micros.append((x, None, cond, labels))
    plain = []
    for x, _, cond, labels in micros:
        tr.forward_backward(x.cuda(), cond.cuda(), labels.cuda())
        plain.append(tr.grads.clone())
    want = (plain[0] + plain[1]) / 2
    for _ in range(2):                                       # direct issue, then capture (the graph test covers replay)
        acc, _ = _window(tr, micros, pattern_scale=1e-3)        # (small against the gradients: its rounding stays out of the bar)
        assert not torch.isnan(acc).any()
        worst = {name: _rel(acc[off:off + int(np.prod(shape))].cpu(), want[off:off + int(np.prod(shape))].cpu())
                 for name, (off, shape) in tr.layout.items()}
        bad = {k: v for k, v in worst.items() if not v <= 1e-4}
        assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
    tr.close()
    return max(worst.values())


# The writers a 16-clip step reaches besides the default grouped launch (full 128 x 128 tiles of dw_tile_tr): the per-product
# split-K weight gradients and per-norm / per-layer reductions (M2M_TRAIN_DW_GROUP=0), the MXFP8 split-K weight gradients
# (M2M_FP8_PARTS=fwd,dx,dw), and the split-K bgemm fallback (M2M_TRAIN_DW_OLD, latched when a trainer is created; set for a child).
@pytest.mark.parametrize("precision,env", [("bf16", {}), ("fp32", {}), ("bf16", {"M2M_TRAIN_DW_GROUP": "0"}),
                                           ("fp8", {"M2M_FP8_PARTS": "fwd,dx,dw"}), ("fp8", {})])
def test_large_window_every_gradient_writer_adds(precision, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    worst = _large_window_check(precision)
    print(f"{precision} {env or 'default'} 16 x 261 x 256: accumulated vs summed plain passes, worst rel err {worst:.2e}")


def test_large_window_bgemm_fallback_adds():
    import os
    import subprocess
    import sys
    from pathlib import Path
    here = Path(__file__).resolve().parent
    env = dict(os.environ, M2M_TRAIN_DW_OLD="1", M2M_TRAIN_DW_GROUP="0", OMP_NUM_THREADS="4")
    code = f"import sys; sys.path[:0] = [{str(here)!r}, {str(here.parent)!r}]; import test_grad_accum_gpu as t; print(t._large_window_check('bf16'))"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
