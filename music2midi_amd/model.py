"""Music2MIDI — the task wrapper callers use (ref: music2midi/model.py:20-140),
without pytorch-lightning: same constructor, ``load_from_checkpoint``,
``generate(audio_path|audio_y, sr, cond_index)``, ``sample_tokens`` and
``evaluate_batch``; segmentation, zero padding, chunking by
``inference.batch_size``, conditioning broadcast, ``max_length=1024`` and the
sequential token decode follow the reference line by line in behaviour.
``training_step`` / ``configure_optimizers`` run the native forward+backward and Adafactor
(csrc/train.hip) instead of autograd + Lightning.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn

from . import distributed as D
from .accumulation import check_accumulate_grad_batches, micro_step, windows
from .audio import load_audio as _load_audio
from .checkpoint import load_t5_state, read_checkpoint
from .clipping import NORM, OFF, check_gradient_clip
from .confidence import confidence_velocities, decode_with_confidence, min_logprob
from .config import inference_beams, inference_consensus, load_config
from .evaluation import (evaluate_batch, evaluate_tokens, frame_scores_host, frame_scores_tokens, note_scores_host,
                         note_scores_tokens)
from .input import ModelInputs
from .transformer import T5Transformer
from .utils import numpy_to_midi


def _decode_entry(model, config, grammar_kwargs: dict, consensus: Optional[int] = None):
    """(decode function, its keywords): ``model.generate`` with the grammar keyword, or - with ``config.inference.num_beams`` > 1 -
    ``model.beam_search_processed`` with the config's beam settings, one returned sequence per clip and the same grammar switch, or
    - with ``config.inference.consensus_samples`` > 1, or a call's ``consensus`` - ``model.generate_consensus`` with the config's
    sampling settings.  Consensus together with beams raises ``ValueError``."""
    chosen = inference_consensus(config, consensus)
    if chosen:
        return model.generate_consensus, dict(chosen, **grammar_kwargs)
    beams = inference_beams(config)
    if not beams:
        return model.generate, grammar_kwargs
    return model.beam_search_processed, dict(beams, num_return_sequences=1, **grammar_kwargs)


def _rows_per_clip(decode_kwargs: dict) -> int:
    """The rows one clip takes in a decode call: its beams, or its consensus candidates."""
    return int(decode_kwargs.get("num_beams", decode_kwargs.get("num_samples", 1)))


def _no_consensus(config, consensus: Optional[int], what: str) -> None:
    """``ValueError`` when consensus decoding is on and the call also asks for per-note confidence: a sampled row's log-probabilities
    are those of the warped distribution and a greedy row's are raw, so they are not mixed."""
    if inference_consensus(config, consensus):
        raise ValueError(f"consensus decoding does not combine with {what}: the log-probabilities of sampled rows (warped) and of "
                         "the greedy row (raw) are not comparable")


def _labelled_token_ids(model, config, grammar_kwargs: dict, inputs) -> torch.Tensor:
    """The decode of one labelled batch that ``evaluate_batch`` and ``score_batch`` share: four tokens per label note of the busiest
    clip; with beams, chunks of batch_size // num_beams clips, as sample_tokens, so a call's rows stay within inference.batch_size;
    with consensus decoding, chunks of batch_size // consensus_samples clips by the same rule."""
    budget = 4 * max(len(n) for n in inputs.notes_batch)
    decode, decode_kwargs = _decode_entry(model, config, grammar_kwargs)
    nb = _rows_per_clip(decode_kwargs)
    if nb == 1:
        return decode(inputs, max_length=budget, **decode_kwargs)
    per_call = max(1, int(config.inference.get("batch_size", 128)) // nb)
    n_clips, parts = len(inputs.notes_batch), []
    for lo in range(0, n_clips, per_call):
        hi = min(lo + per_call, n_clips)
        part = type(inputs)(input_waveform=inputs.input_waveform[lo:hi], notes_batch=inputs.notes_batch[lo:hi],
                            cond_index=inputs.cond_index[lo:hi] if inputs.cond_index is not None else None)
        parts.append(decode(part, max_length=budget, **decode_kwargs))
    width = max(p.shape[1] for p in parts)
    pad = model.geometry.pad_token_id
    return torch.cat([torch.nn.functional.pad(p, (0, width - p.shape[1]), value=pad) for p in parts], dim=0)


def _score_on_host(tokenizer, token_ids, notes_batch):
    """(chroma accuracy, decoded MIDI per clip, label MIDI per clip): detokenise, build the MIDI objects and score, on the host."""
    predicted = [numpy_to_midi(n) for n in tokenizer.decode(token_ids, mode="batched")]
    wanted = [numpy_to_midi(n) for n in notes_batch]
    return evaluate_batch(wanted, predicted), predicted, wanted


def _scored_decode(model, config, grammar_kwargs: dict, inputs, max_length: int):
    """(ids [B, n], log-probabilities [B, n]) of one greedy decode with ``output_logprobs=True``: ``generate`` returns the
    log-probability of ids[:, i + 1] in column i, so one leading 0.0 column (the start token's) aligns column i with ids[:, i]."""
    if inference_beams(config):
        raise ValueError("per-note confidence needs the log-probability of every token; with inference.num_beams > 1 the beam search "
                         "returns sequences_scores only")
    _no_consensus(config, None, "per-note confidence (min_note_confidence, a positive threshold)")
    out = model.generate(inputs, max_length=max_length, return_dict_in_generate=True, output_logprobs=True, **grammar_kwargs)
    return out.sequences, torch.nn.functional.pad(out.logprobs, (1, 0), value=0.0)


def _min_note_confidence(config, min_confidence: Optional[float]) -> float:
    """The threshold of a call: the argument, else ``config.inference.min_note_confidence`` (absent: 0.0, every note is kept);
    ``ValueError`` for a value above 1 or NaN."""
    if min_confidence is None:
        min_confidence = config.inference.get("min_note_confidence", 0.0)
    min_logprob(min_confidence)
    return float(min_confidence)


def _any_positive(thresholds) -> bool:
    """True when a sweep needs the tokens' log-probabilities: some threshold keeps less than every note.  ``ValueError`` for a
    threshold above 1 or NaN, an empty sweep or one longer than the device takes."""
    from .scoring import threshold_logprobs
    return bool((threshold_logprobs(thresholds, True, "note_scores") != -np.inf).any())


def _single_process(what: str, instead: str) -> None:
    if D.dist.is_available() and D.dist.is_initialized() and D.dist.get_world_size() > 1:
        raise NotImplementedError(f"{what} runs on one GPU: with a process group, {instead}")


def _on_device_scorable(token_ids, label_arrays) -> bool:
    """The device path takes ids that are on a GPU and labels ``scoring.labels_eligible`` accepts; everything else is the host's."""
    if not (isinstance(token_ids, torch.Tensor) and token_ids.is_cuda):
        return False
    from .scoring import labels_eligible
    return labels_eligible(label_arrays)


class Music2MIDI(nn.Module):
    def __init__(self, config_path: str, precision: Optional[str] = None):
        super().__init__()
        self.config = load_config(config_path)
        self.model = T5Transformer(config_path, precision=precision)
        self.hparams = {"config_path": config_path}

    # -- checkpoint ----------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, config_path: Optional[str] = None, map_location=None,
                             strict: bool = True, **kwargs) -> "Music2MIDI":
        """Lightning-format ``.ckpt`` -> model (ref: evaluate.py:27, webui.py:90)."""
        ckpt = read_checkpoint(checkpoint_path)
        if config_path is None:
            config_path = (ckpt.get("hyper_parameters") or {}).get("config_path", "config.yaml")
        obj = cls(config_path, **kwargs)
        state = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
        prefix = "model."
        inner = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
        load_t5_state(obj.model, inner if inner else state, strict=strict)
        return obj

    @property
    def device(self) -> torch.device:
        return self.model.transformer.device

    # -- training surface (ref model.py:27-43) -----------------
    _trainer = None
    global_step = 0

    def _native_trainer(self, B: int = 0, S: int = 0, L: int = 0, keep_grads: bool = False):
        """The native trainer, (re)built when a batch exceeds the sizes it was created for.  ``keep_grads``: the next pass adds to
        the gradients (a micro-batch inside an accumulation window), so a rebuild carries the flat gradient buffer over."""
        from .training import NativeTrainer
        tr = self._trainer
        if tr is None or not tr.fits(B, S, L):
            old = tr.limits if tr is not None else (0, 0, 0)
            state = tr.optimizer_state() if tr is not None and tr.step_count > 0 else None
            grads = tr.grads if tr is not None and keep_grads else None      # (a torch allocation: it outlives close())
            if tr is not None:
                tr.close()
            limits = (max(B, old[0], int(self.config.dataloader.batch_size)), max(S, old[1]), max(L, old[2], 64))
            self._trainer = NativeTrainer(self.model, *limits, precision=getattr(self, "train_precision", None))
            if state is None and self._resume_optimizer_state is not None:      # a checkpoint read before the first batch
                state, self._resume_optimizer_state = self._resume_optimizer_state, None
            if state is not None:
                self._trainer.load_optimizer_state(state)
            if grads is not None:
                if grads.numel() != self._trainer.grads.numel():
                    raise RuntimeError(f"trainer rebuild inside an accumulation window: gradient layout changed ({grads.numel()} -> "
                                       f"{self._trainer.grads.numel()} floats)")
                self._trainer.grads.copy_(grads)
            if D.dist.is_available() and D.dist.is_initialized() and D.dist.get_world_size() > 1 and self._trainer.device.type == "cuda":
                # every pass of this trainer releases the decoder-side gradients half-way (distributed.all_reduce_gradients_overlapped)
                self._trainer.set_sync_stream(torch.cuda.Stream(device=self._trainer.device))
        # dropout as the reference trains: model.train() (ref train.py:33) activates T5Config.dropout_rate (0.1 unless the
        # config says otherwise); .eval() switches it off
        # The mask sequence is indexed by passes: a trainer (re)built or resumed after P passes restarts it at seed + P, where the
        # uninterrupted trainer is.  With N = 1 the passes are the optimizer steps (global_step); with gradient accumulation they are
        # counted (_train_passes, kept in the checkpoint), so a rebuild inside a window continues the masks too.
        want = float(self.config.model.t5.get("dropout_rate", 0.1)) if self.training else 0.0
        if self._trainer.dropout != want:
            done = self.global_step if self._accumulation() == 1 else self._train_passes
            self._trainer.set_dropout(want, seed=int(getattr(self, "seed", 0)) + done)
        return self._trainer

    _resume_optimizer_state = None

    def configure_optimizers(self):
        """ref model.py:27-30: Adafactor(self.parameters(), warmup_init=True) + AdafactorSchedule."""
        from .training import Adafactor, AdafactorSchedule
        optimizer = Adafactor(self)
        return [optimizer], [AdafactorSchedule(optimizer)]

    # Labels are padded to the longest sequence of the batch (ref: music2midi/tokenizer.py:86-96), so the decoder length changes
    # from batch to batch.  Rounded up to a multiple of LABEL_BUCKET with ignored (-100) positions the loss and every gradient are
    # unchanged — an ignored position contributes nothing and, being causal, is seen by no scored one — while the trainer meets a
    # handful of shapes instead of one per batch and replays their captured graphs (csrc/train.hip GraphSlot).
    LABEL_BUCKET = 16

    def _labels(self, notes_batch) -> torch.Tensor:
        """The labels of one batch: ``tokenizer(notes_batch)`` with PAD -> -100, padded to the bucket.  With
        ``config.trainer.device_labels: true`` (absent: off), the model on a GPU and notes ``tokenize.notes_eligible`` accepts, the
        same tensor is written on the device by one kernel (``T5Transformer.device_labels``) and stays there."""
        t5 = self.model
        if bool(self.config.get("trainer", {}).get("device_labels", False)):
            labels = t5.device_labels(notes_batch, bucket=self.LABEL_BUCKET, enabled=True)
            if labels is not None:
                return labels
        labels = t5.tokenizer(notes_batch)
        labels[labels == t5.geometry.pad_token_id] = -100
        pad = -labels.shape[1] % self.LABEL_BUCKET
        if pad:
            labels = torch.nn.functional.pad(labels, (0, pad), value=-100)
        return labels

    _accumulate_override = None
    _train_passes = 0                  # forward + backward passes of training_step (the dropout mask index; see _native_trainer)
    _micro = None                      # the MicroStep fit_batches hands the next training_step

    def _accumulation(self) -> int:
        """N of gradient accumulation: ``fit_batches(accumulate_grad_batches=)`` if given, else ``config.trainer.accumulate_grad_batches``
        (ref config.yaml; 1 when the key is absent)."""
        if self._accumulate_override is not None:
            return check_accumulate_grad_batches(self._accumulate_override)
        return check_accumulate_grad_batches(self.config.trainer.get("accumulate_grad_batches", 1))

    # Gradient clipping (music2midi_amd.clipping): Lightning's automatic optimisation clips where the optimizer steps, with the
    # Trainer's gradient_clip_val / gradient_clip_algorithm — here fit_batches, from config.trainer or its own keywords.  A
    # hand-written loop clips only what clip_gradients() armed, as a LightningModule under manual optimisation does.
    _clip_override = None              # (val, algorithm) of fit_batches' keywords, for the duration of that call
    _clip_fit = None                   # (mode, value) every step of the running fit_batches applies
    _clip_armed = None                 # (mode, value) clip_gradients() set for the next optimizer.step()

    def _gradient_clip(self):
        """(mode, value) of ``trainer.gradient_clip_val`` / ``trainer.gradient_clip_algorithm`` (absent keys: off, "norm"), each
        replaced by ``fit_batches``' keyword when that is given; TypeError / ValueError as ``check_gradient_clip`` raises them."""
        val = self.config.trainer.get("gradient_clip_val", None)
        algorithm = self.config.trainer.get("gradient_clip_algorithm", None)
        if self._clip_override is not None:
            o_val, o_alg = self._clip_override
            val = o_val if o_val is not None else val
            algorithm = o_alg if o_alg is not None else algorithm
        return check_gradient_clip(val, algorithm)

    def clip_gradients(self, optimizer=None, gradient_clip_val=None, gradient_clip_algorithm=None):
        """``LightningModule.clip_gradients`` for hand-written loops: call it between the backward pass and ``optimizer.step()``.
        Arguments left ``None`` take ``config.trainer``'s values.  Unlike Lightning's it does not touch ``.grad``: it ARMS the next
        ``optimizer.step()``, whose kernels read the clipped gradient on the fly (second moments and update see exactly what
        ``clip_grad_norm_`` / ``clip_grad_value_`` would have left), and ``.grad`` keeps the unclipped gradient afterwards."""
        val = gradient_clip_val if gradient_clip_val is not None else self.config.trainer.get("gradient_clip_val", None)
        algorithm = gradient_clip_algorithm if gradient_clip_algorithm is not None else self.config.trainer.get("gradient_clip_algorithm", None)
        self._clip_armed = check_gradient_clip(val, algorithm)

    def _sync_grad_clip(self, tr):
        """Set the clipping the next optimizer step applies on the trainer (a rebuilt trainer starts with clipping off): what
        clip_gradients() armed, else the running fit_batches' setting, else off.  Returns it."""
        want = self._clip_armed or self._clip_fit or (OFF, 0.0)
        if getattr(tr, "grad_clip", (OFF, 0.0)) != want:
            tr.set_grad_clip(*want)
        return want

    def training_step(self, inputs: ModelInputs, batch_idx):
        """ref model.py:32-43.  Lightning calls backward() on the returned loss; here forward AND backward have
        already been ENQUEUED when this returns: every parameter's ``.grad`` will hold d loss / d parameter (views of one flat
        buffer), ready for ``distributed.all_reduce_gradients`` and ``optimizer.step()``.  Nothing here waits for the device: the
        returned loss and ``self.logged["train/loss"]`` are 0-dim tensors on the GPU (``logged_metrics()`` reads them), so the
        gradient all-reduce the caller enqueues next overlaps the backward pass that is still running.
        With ``accumulate_grad_batches = N`` > 1 this is one micro-batch of a window (position ``batch_idx % N`` unless ``fit_batches``
        says otherwise): the gradient of loss / N is written (first of the window) or added (the others); the returned and logged
        loss is the unscaled one."""
        t5 = self.model
        labels = self._labels(inputs.notes_batch)
        x = t5.encoder_inputs(inputs)
        n = self._accumulation()
        ms = self._micro if self._micro is not None else micro_step(n, int(batch_idx) % n)
        tr = self._native_trainer(x.shape[0], x.shape[1], labels.shape[1], keep_grads=n > 1 and ms.accumulate)
        if n == 1:
            loss, _ = tr.forward_backward(x, inputs.cond_index, labels)
        else:
            loss, _ = tr.forward_backward(x, inputs.cond_index, labels, grad_scale=ms.grad_scale, accumulate=ms.accumulate)
        self._train_passes += 1
        loss = loss[0].clone()                                # the trainer's loss word is rewritten by the next pass
        self.logged = {"train/loss": loss, "batch_size": int(x.shape[0])}
        if (self.global_step + 1) % int(self.config.trainer.log_every_n_steps) == 0:
            self.logged["train/score"] = float(self.score_batch(inputs))
        return loss

    def logged_metrics(self) -> dict:
        """The values of the last step as Lightning would log them: ``self.log(..., sync_dist=True)`` in the reference
        (ref model.py:37,42,49,52) means the MEAN over the data-parallel ranks — one packed all-reduce
        (``distributed.reduce_logged``); this is also where device-resident values are read."""
        return D.reduce_logged(dict(getattr(self, "logged", {}) or {}), device=self.device)

    # -- checkpoints of a training run (ref train.py:41: trainer.fit(..., ckpt_path=args.ckpt)) ------------------------------
    def save_checkpoint(self, path, collective: bool = True) -> None:
        """A Lightning-layout ``.ckpt`` of the run: ``state_dict`` (``model.*`` keys incl. the torchaudio buffers), the optimizer
        state as ``transformers.optimization.Adafactor.state_dict()`` lays it out (``optimizer_states[0]``), ``global_step``,
        ``hyper_parameters`` — what ``load_from_checkpoint`` and ``fit_batches(ckpt_path=)`` (and the reference's own
        ``trainer.fit(ckpt_path=)``) read.  Under data parallelism only global rank 0 writes (as Lightning does), into a temporary
        file that is renamed over ``path`` once complete — a reader never sees a torn file — and every rank leaves through a
        broadcast of rank 0's outcome: a ``resume_from_checkpoint`` that follows on any rank reads the finished file, and when
        rank 0 FAILED (disk full, permissions) every rank raises instead of walking into the next gradient all-reduce without it.
        Like ``Trainer.save_checkpoint`` this is therefore a collective call: every rank must make it.  A caller that guards it
        itself (``if rank == 0: model.save_checkpoint(p, collective=False)``) gets the plain single-process behaviour."""
        failure = None
        if D.is_rank_zero() or not collective:
            try:
                tr = self._trainer
                opt = tr.optimizer_state_hf() if tr is not None else {"state": {}, "param_groups": []}     # reads the device: rank 0 only
                torch.cuda.synchronize(self.device) if self.device.type == "cuda" else None
                path = Path(path)
                tmp = path.with_name(f".{path.name}.tmp{os.getpid()}")
                try:
                    extra = {"train_passes": int(self._train_passes)} if self._accumulation() > 1 else {}     # (see _native_trainer)
                    torch.save({
                        **extra,
                        "epoch": int(getattr(self, "current_epoch", 0)), "global_step": int(self.global_step), "pytorch-lightning_version": "2.1.0",
                        "state_dict": {k: v.detach().cpu().clone() for k, v in self.state_dict().items()},
                        "callbacks": {}, "optimizer_states": [opt],
                        "lr_schedulers": [{"base_lrs": [0.0], "last_epoch": int(self.global_step), "_step_count": int(self.global_step) + 1}],
                        "hparams_name": "kwargs", "hyper_parameters": dict(self.hparams),
                    }, tmp)
                    os.replace(tmp, path)
                finally:
                    if tmp.exists():
                        tmp.unlink()
            except Exception as e:           # the other ranks are on their way to the barrier: meet them there before raising
                failure = e
        if collective:
            failed = D.broadcast_flag(1 if failure is not None else 0, self.device)
            if failed and failure is None:
                raise RuntimeError(f"save_checkpoint: global rank 0 failed to write {path} (see its error); nothing was saved")
        if failure is not None:
            raise failure

    def resume_from_checkpoint(self, path) -> None:
        """Weights, Adafactor state and step counter of a ``.ckpt`` written by ``save_checkpoint`` or by Lightning."""
        ckpt = read_checkpoint(path)
        state = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
        inner = {k[len("model."):]: v for k, v in state.items() if k.startswith("model.")}
        tr = self._trainer
        if tr is not None:                                   # the parameters are views of the trainer's flat buffer: copy in place
            own = dict(self.model.named_parameters())
            with torch.no_grad():
                for k, v in (inner or state).items():
                    if k in own:
                        own[k].copy_(torch.as_tensor(v).to(own[k].device, own[k].dtype))
            self.model._weights_epoch = getattr(self.model, "_weights_epoch", 0) + 1
        else:
            load_t5_state(self.model, inner if inner else state, strict=False)
        self.global_step = int(ckpt.get("global_step", 0))
        # passes so far (written by save_checkpoint under gradient accumulation; without it, every earlier window was complete)
        self._train_passes = int(ckpt.get("train_passes", self.global_step * self._accumulation()))
        opts = ckpt.get("optimizer_states") or []
        opt = opts[0] if opts else None
        if opt is not None and opt.get("state"):
            if tr is not None:
                tr.load_optimizer_state(opt)
            else:
                self._resume_optimizer_state = opt
        if tr is not None:
            tr.dropout = -1.0                                # the mask sequence restarts from the restored step (see _native_trainer)

    def fit_batches(self, batches, optimizer=None, world_size: int = 1, ckpt_path=None, save_path=None, save_every_n_steps: int = 0,
                    accumulate_grad_batches=None, augment=None, gradient_clip_val=None, gradient_clip_algorithm=None):
        """Minimal stand-in for ``pl.Trainer.fit`` (ref train.py:40-41): step over an iterable of ModelInputs.  ``ckpt_path``
        resumes a run (weights + Adafactor state + step counter) as ``trainer.fit(..., ckpt_path=)`` does; ``save_path`` is
        (re)written every ``save_every_n_steps`` steps and at the end.  The host never waits for a step: losses stay on the device
        until the loop is over, metrics are reduced over the ranks and read every ``trainer.log_every_n_steps`` steps
        (``self.log_history``).
        Gradient accumulation (``accumulate_grad_batches``, default ``config.trainer.accumulate_grad_batches``; see
        ``music2midi_amd.accumulation``): the optimizer steps — and the gradients are all-reduced — once per window of N batches
        and after the last batch; ``global_step``, ``save_every_n_steps`` and ``log_every_n_steps`` count optimizer steps, so
        checkpoints fall on window boundaries.  The returned losses are per batch, unscaled.  The override holds for this call only.
        Gradient clipping (``gradient_clip_val`` / ``gradient_clip_algorithm``, default ``config.trainer``'s, absent: off / "norm";
        see ``music2midi_amd.clipping``): every optimizer step clips — once per window, on the summed gradient, after the
        all-reduce.  A bad value is refused before the first step; the override holds for this call only.  ``.grad`` keeps the
        unclipped gradient (the step clips on the fly).  In norm mode every ``log_history`` entry carries ``train/grad_norm``, the
        total norm before clipping of that step, read at the log step only.
        ``augment`` (a ``np.random.Generator``, or ``True`` for ``default_rng(0)``): every batch goes through
        ``music2midi_amd.augment.augment`` first — the reference dataset's normalise / transpose draws (ref dataset.py:130-133), the
        audio shifted on the device; ``None`` leaves the batches as they are."""
        if augment is not None and augment is not False:
            from .augment import augment as augment_batch
            rng = np.random.default_rng(0) if augment is True else augment
            batches = (augment_batch(batch, rng) for batch in batches)
        if accumulate_grad_batches is not None:
            check_accumulate_grad_batches(accumulate_grad_batches)
        if gradient_clip_val is not None or gradient_clip_algorithm is not None:
            check_gradient_clip(gradient_clip_val, gradient_clip_algorithm)
        previous = self._accumulate_override, self._clip_override, self._clip_fit
        self._accumulate_override = accumulate_grad_batches
        self._clip_override = (gradient_clip_val, gradient_clip_algorithm)
        try:
            n = self._accumulation()                     # ValueError before the first step
            self._clip_fit = self._gradient_clip()       # TypeError / ValueError before the first step
            return self._fit_windows(batches, n, optimizer, ckpt_path, save_path, save_every_n_steps)
        finally:
            self._accumulate_override, self._clip_override, self._clip_fit = previous

    def _fit_windows(self, batches, n, optimizer, ckpt_path, save_path, save_every_n_steps):
        if ckpt_path is not None:
            self.resume_from_checkpoint(ckpt_path)
        if optimizer is None:
            optimizer = self.configure_optimizers()[0][0]
        log_every = max(1, int(self.config.trainer.log_every_n_steps))
        self.log_history = getattr(self, "log_history", [])
        losses, pending = [], []          # host floats so far / device scalars of the steps since the last read
        for i, (batch, ms) in enumerate(windows(batches, n)):
            self._micro = ms
            try:
                loss = self.training_step(batch, i)
            finally:
                self._micro = None
            pending.append(loss)
            if not ms.step:                      # inside a window: no all-reduce, no optimizer step (Lightning's no_sync)
                continue
            tr = self._trainer
            if tr.sync_stream is not None:       # data-parallel (set when the trainer was built): decoder-side pieces overlap the encoder backward
                D.all_reduce_gradients_overlapped(tr.grads, tr.early_ranges, tr.sync_stream)
            else:
                D.all_reduce_gradients(tr.grads)
            clip_mode, _ = self._sync_grad_clip(tr)      # clipping runs where the optimizer steps: after the all-reduce, on the window's sum
            optimizer.step()
            self.global_step += 1
            if self.global_step % log_every == 0:
                if clip_mode == NORM:                    # the step's own norm word, still on the device: read with the other metrics
                    self.logged["train/grad_norm"] = self._trainer.grad_stats()[0]
                self.log_history.append(dict(self.logged_metrics(), step=self.global_step))
                # logged_metrics() has just waited for this step: move the window's losses to the host here, so that a long run
                # (119 200 steps in the reference's) holds at most log_every device scalars, not one per step
                losses.extend(float(v) for v in torch.stack(pending).cpu())
                pending = []
            if save_path is not None and save_every_n_steps and self.global_step % save_every_n_steps == 0:
                self.save_checkpoint(save_path)
        if save_path is not None:
            self.save_checkpoint(save_path)
        if pending:
            losses.extend(float(v) for v in torch.stack(pending).cpu())
        return losses

    def validation_step(self, inputs: ModelInputs, batch_idx):
        """ref model.py:45-54: teacher-forced loss + chroma score of a greedy decode; returns the LOSS (as the
        reference does).  Lightning's ``self.log`` does not exist here: the two values are kept in
        ``self.logged`` under the reference's metric names, already reduced over the ranks (``sync_dist=True``)."""
        loss = self.model(inputs).loss
        score = self.score_batch(inputs)
        self.logged = D.reduce_logged({"val/loss": loss, "val/score": float(score), "batch_size": int(inputs.input_waveform.shape[0])},
                                      device=self.device)
        self.logged["batch_size"] = int(self.logged["batch_size"])
        return loss

    # -- inference -----------------------------------------------------------
    def _grammar_kwargs(self) -> dict:
        """``midi_grammar=True`` for generate when ``config.inference.midi_grammar`` says so (absent: unconstrained, no keyword)."""
        return {"midi_grammar": True} if bool(self.config.inference.get("midi_grammar", False)) else {}

    @torch.no_grad()
    def evaluate_batch(self, inputs: ModelInputs):
        """(chroma accuracy, decoded MIDI per clip, label MIDI per clip) for one labelled batch — ref
        model.py:55-65.  The decode budget is four tokens per label note of the busiest clip."""
        token_ids = _labelled_token_ids(self.model, self.config, self._grammar_kwargs(), inputs)
        return _score_on_host(self.model.tokenizer, token_ids, inputs.notes_batch)

    @torch.no_grad()
    def score_batch(self, inputs: ModelInputs) -> float:
        """``evaluate_batch(inputs)[0]`` without the host: the same decode, then detokenising, melody and counts on the device
        (``evaluation.evaluate_tokens``) - the same float.  Labels the device path does not take, or ids that are not on a GPU,
        are scored on the host from the same ids.  With ``config.inference.min_note_confidence`` > 0 the decode also returns the
        tokens' log-probabilities and only the notes of at least that confidence are scored (``music2midi_amd.confidence``)."""
        floor = _min_note_confidence(self.config, None)
        if floor > 0:
            budget = 4 * max(len(n) for n in inputs.notes_batch)
            token_ids, lps = _scored_decode(self.model, self.config, self._grammar_kwargs(), inputs, budget)
            if _on_device_scorable(token_ids, inputs.notes_batch):
                return evaluate_tokens(self.model.tokenizer, token_ids, inputs.notes_batch, token_logprobs=lps, min_confidence=floor)
            decoded, _ = decode_with_confidence(self.model.tokenizer, token_ids, lps, mode="batched", min_confidence=floor)
            return float(evaluate_batch([numpy_to_midi(n) for n in inputs.notes_batch], [numpy_to_midi(n) for n in decoded]))
        token_ids = _labelled_token_ids(self.model, self.config, self._grammar_kwargs(), inputs)
        if _on_device_scorable(token_ids, inputs.notes_batch):
            return evaluate_tokens(self.model.tokenizer, token_ids, inputs.notes_batch)
        return float(_score_on_host(self.model.tokenizer, token_ids, inputs.notes_batch)[0])

    def generate(self, audio_path: Optional[Union[str, Path]] = None, audio_y: Optional[np.ndarray] = None,
                 sr: Optional[int] = None, cond_index: Optional[list] = None, confidence_velocity: bool = False,
                 consensus: Optional[int] = None, beat_grid: Optional[bool] = None, quantize: Optional[int] = None):
        """Specify either audio_path or audio_y as input; returns a MIDI object.  ``confidence_velocity=True`` writes every note's
        confidence into its velocity: ``max(1, min(127, int(round(127 * confidence))))``.  ``consensus=K`` as in
        :meth:`generate_notes`.

        ``beat_grid=True`` (``None``: ``config.inference.beat_grid``, absent off) tracks the recording's beats
        (:meth:`generate_beats`) and returns the stand-in ``SimpleMIDI`` - always, also with pretty_midi installed - with its
        ``beat_times`` set, so that ``write`` lays a tempo map along the beats and an editor shows bars and beats that follow the
        music; note times in seconds are unchanged.  ``quantize=n`` (with the beat grid only) snaps onsets and offsets to ``n`` grid
        points per beat first (``music2midi_amd.beats.quantize``).  Without the keyword and the config key a call is what it was."""
        if beat_grid is None:
            beat_grid = bool(self.config.inference.get("beat_grid", False))
        if quantize is not None and not beat_grid:
            raise ValueError("generate: quantize needs beat_grid=True")
        if not confidence_velocity:
            override = {} if consensus is None else {"consensus": consensus}
            notes = self.generate_notes(audio_path, audio_y, sr, cond_index, **override)
        else:
            _no_consensus(self.config, consensus, "confidence_velocity=True")
            notes, confidence = self.generate_notes(audio_path, audio_y, sr, cond_index, return_confidence=True)
            notes[:, 3] = confidence_velocities(confidence)
        if not beat_grid:
            return numpy_to_midi(notes)
        from . import beats as beats_mod
        from .utils import simple_midi
        result = self.generate_beats(audio_path, audio_y, sr)
        if quantize is not None and len(result.beat_times) >= 2:
            notes = beats_mod.quantize(notes, result.beat_times, quantize)
        midi = simple_midi(notes)
        midi.beat_times = result.beat_times if len(result.beat_times) >= 2 else None
        return midi

    def generate_beats(self, audio_path=None, audio_y=None, sr=None):
        """``music2midi_amd.beats.BeatResult`` of a recording: its beat times in seconds, their frames, the period and the tempo.
        The audio is read as :meth:`generate` reads it (at the model's sample rate) and tracked on the model's device
        (``beats.track``), by the definition in numpy when the model is on the CPU."""
        from . import beats as beats_mod
        samples = self._resolve_audio(audio_path, audio_y, sr)
        rate = self.config.model.sample_rate
        if self.device.type != "cuda":
            return beats_mod.track_host(samples, sr=rate)
        return beats_mod.track(samples, sr=rate, device=self.device)

    # The three steps below are what ref model.py:67-140 does inline: validate/load, cut the song into
    # whole segments (zero-padded tail), decode the segments in chunks and stitch the notes together.
    def _resolve_audio(self, audio_path, audio_y, sr) -> np.ndarray:
        model_sr = self.config.model.sample_rate
        if audio_path is None and audio_y is None:
            raise ValueError("Either audio_path or audio_y should be specified")
        if sr is not None:
            assert sr == model_sr
        if audio_y is None:
            audio_y = _load_audio(audio_path, model_sr)
        return np.asarray(audio_y, dtype=np.float32)

    def _segment_length(self) -> int:
        return int(self.config.model.sample_rate * self.config.dataset.segment_duration)

    def generate_notes(self, audio_path=None, audio_y=None, sr=None, cond_index=None, return_confidence: bool = False,
                       min_confidence: Optional[float] = None, consensus: Optional[int] = None):
        """Note array [n, 4] (onset_s, offset_s, pitch, velocity) for a whole recording.  ``return_confidence=True`` returns
        ``(notes, confidence [n] float64)``: the probability the model gave the six tokens that made each note
        (``music2midi_amd.confidence``).  ``min_confidence`` (``None``: ``config.inference.min_note_confidence``, absent 0.0) drops
        the notes below it.  Either one decodes with ``output_logprobs=True`` and detokenises on the device; greedy, one GPU.

        ``consensus=K`` (``None``: ``config.inference.consensus_samples``, off when absent, 0 or 1) decodes every segment K times -
        the greedy row and K - 1 sampled rows (``inference.consensus_temperature`` / ``consensus_top_k`` / ``consensus_top_p``) -
        and keeps the row the others agree with most by note-level F1 (``T5Transformer.generate_consensus``,
        ``music2midi_amd.consensus``); a chunk is then ``batch_size // K`` segments.  The selection is per segment: each row is
        detokenised on its own in batched mode, where a note left open at the row's end is dropped; the chosen rows then go
        through the sequential decode as always.  Consensus with ``inference.num_beams`` > 1, with ``return_confidence=True`` or
        with a positive ``min_confidence`` raises ``ValueError``.  Whether the chosen rows transcribe better than the greedy ones
        on a trained model has not been measured."""
        floor = _min_note_confidence(self.config, min_confidence)
        if return_confidence or floor > 0:
            _no_consensus(self.config, consensus, "return_confidence=True or a positive min_confidence")
        else:
            inference_consensus(self.config, consensus)          # a bad K, or consensus with beams, is refused before the audio is read
        padded, seg = self._padded_segments(audio_path, audio_y, sr)
        if not return_confidence and not floor > 0:
            override = {} if consensus is None else {"consensus": consensus}
            return self.sample_tokens(padded, seg, split_duration=self.config.dataset.segment_duration, cond_index=cond_index, **override)
        token_ids, lps = self.sample_scored_rows(padded, seg, cond_index)
        duration = self.config.dataset.segment_duration
        if token_ids.is_cuda:
            from .scoring import detokenize_scored
            dn = detokenize_scored(self.model.tokenizer, token_ids, lps, "sequential", duration, floor)
            notes, confidence = dn.to_numpy(), dn.confidence_numpy()
        else:
            notes, confidence = decode_with_confidence(self.model.tokenizer, token_ids, lps, "sequential", duration, floor)
        return (notes, confidence) if return_confidence else notes

    def generate_audio(self, audio_path=None, audio_y=None, sr=None, cond_index=None, fs=None, normalize: bool = True):
        """``(notes, audio)``: ``generate_notes``, then the notes rendered on the model's device by ``music2midi_amd.render.render``
        at ``fs`` (``None``: the model's sample rate) - a fp32 tensor of ``last offset + release`` samples, peak-normalised unless
        ``normalize=False``.  The timbre is the renderer's built-in voice."""
        from .render import render
        notes = self.generate_notes(audio_path, audio_y, sr, cond_index)
        fs = self.config.model.sample_rate if fs is None else fs
        return notes, render(notes, fs, normalize=normalize, device=self.device)

    def _device_ingest(self, audio_path, audio_y) -> bool:
        """The device ingest takes the call when ``config.inference.device_ingest`` is set (absent: off), the audio comes as a
        path, the model is on a GPU and ``ingest.eligible`` accepts the file; everything else is the host's ``load_audio``."""
        if audio_path is None or audio_y is not None or not bool(self.config.inference.get("device_ingest", False)):
            return False
        if self.device.type != "cuda":
            return False
        from . import ingest
        return ingest.eligible(audio_path, self.config.model.sample_rate)

    def _padded_segments(self, audio_path, audio_y, sr):
        """(the recording on the device, zero-padded to whole segments; samples per segment).  With
        ``config.inference.device_ingest: true`` an eligible WAVE file given as ``audio_path`` is decoded, downmixed, resampled and
        padded on the device (``ingest.load_audio_device``): the samples ``audio.read_wav`` + scipy's ``resample_poly`` give, bit for
        bit.  The key wins over an installed librosa - the device path restates the scipy definition, not librosa's soxr resampler,
        so with librosa present the two paths differ.  Files the device path does not take (compressed containers, 8 or more
        channels, unknown sample formats) go through the host as without the key."""
        seg = self._segment_length()
        if self._device_ingest(audio_path, audio_y):
            from . import ingest
            if sr is not None:
                assert sr == self.config.model.sample_rate
            return ingest.load_audio_device(audio_path, self.config.model.sample_rate, device=self.device, pad_to=seg), seg
        samples = self._resolve_audio(audio_path, audio_y, sr)
        n_segments = -(-len(samples) // seg)                       # ceil
        padded = np.zeros(n_segments * seg, dtype=np.float32)
        padded[: len(samples)] = samples
        return torch.from_numpy(padded).to(self.device), seg

    def _cond_rows(self, n_rows: int, cond_index: Optional[list]) -> torch.Tensor:
        """[n_rows, n_embeds] int64: the same (genre, difficulty) pair for every segment; zeros when None."""
        n_embeds = len(self.model.conditioning.embeds)
        rows = torch.zeros((n_rows, n_embeds))
        if cond_index is not None:
            rows = rows + torch.Tensor(cond_index)
        rows = rows.long()
        self.model.conditioning.check_indices(rows)      # IndexError on the host, as nn.Embedding raises it (ref input.py:57)
        return rows.to(self.device)

    @torch.no_grad()
    def sample_tokens(self, waveform: torch.Tensor, split_size: int, split_duration: float,
                      cond_index: Optional[list] = None, consensus: Optional[int] = None) -> np.ndarray:
        """Segments -> chunks of inference.batch_size -> generate(max_length=1024) -> notes.  With inference.num_beams > 1 a chunk is
        batch_size // num_beams clips, decoded by beam_search_processed: the rows of a call stay what the config sized the session for.
        With consensus decoding (``consensus``, else inference.consensus_samples) a chunk is batch_size // K clips by the same rule."""
        token_rows = self.sample_token_rows(waveform, split_size, cond_index, **({} if consensus is None else {"consensus": consensus}))
        return self.model.tokenizer.decode(token_rows, mode="sequential", duration_per_batch=split_duration)

    @torch.no_grad()
    def sample_token_rows(self, waveform: torch.Tensor, split_size: int, cond_index: Optional[list] = None,
                          consensus: Optional[int] = None) -> list:
        """The token row of every segment, in segment order, not detokenised (rows of different chunks may differ in width)."""
        decode, decode_kwargs = _decode_entry(self.model, self.config, self._grammar_kwargs(), consensus)
        per_call = max(1, int(self.config.inference.batch_size) // _rows_per_clip(decode_kwargs))
        token_rows = []
        for inputs in self._segment_chunks(waveform, split_size, cond_index, per_call):
            # with a process group (one process per GPU) the chunk's segments are sharded over the ranks and the ids
            # all-gathered back in segment order; a single process decodes the chunk itself
            ids = D.generate_sharded(decode, inputs, max_length=1024, pad_id=self.model.geometry.pad_token_id, **decode_kwargs)
            token_rows.extend(ids.unbind(0))
        return token_rows

    def _segment_chunks(self, waveform: torch.Tensor, split_size: int, cond_index: Optional[list], per_call: int):
        """The segments of a recording as the inputs of one decode call each, ``per_call`` segments at a time."""
        pieces = torch.split(waveform, split_size)
        for first in range(0, len(pieces), per_call):
            group = pieces[first:first + per_call]
            longest = max(p.shape[0] for p in group)
            wav = waveform.new_zeros((len(group), longest)).to(self.device)
            for row, piece in enumerate(group):                      # right-pad a ragged last piece with zeros
                wav[row, : piece.shape[0]] = piece
            yield ModelInputs(input_waveform=wav, cond_index=self._cond_rows(len(group), cond_index))

    @torch.no_grad()
    def sample_scored_rows(self, waveform: torch.Tensor, split_size: int, cond_index: Optional[list] = None):
        """(ids [segments, W] int64, log-probabilities [segments, W] float32) of every segment, in segment order: the chunks of
        ``sample_token_rows`` decoded with ``output_logprobs=True`` and padded to one width - PAD for the ids, 0.0 for the
        log-probabilities; column i of the second belongs to column i of the first.  Greedy decoding on one GPU: beams raise
        ``ValueError``, a process group of more than one rank ``NotImplementedError``."""
        _single_process("per-note confidence", "decode on one rank (the log-probabilities are not gathered across ranks)")
        grammar_kwargs, pad = self._grammar_kwargs(), self.model.geometry.pad_token_id
        parts = [_scored_decode(self.model, self.config, grammar_kwargs, inputs, 1024)
                 for inputs in self._segment_chunks(waveform, split_size, cond_index, max(1, int(self.config.inference.batch_size)))]
        width = max(int(ids.shape[1]) for ids, _ in parts)
        token_ids = torch.cat([torch.nn.functional.pad(ids, (0, width - int(ids.shape[1])), value=pad) for ids, _ in parts])
        lps = torch.cat([torch.nn.functional.pad(lp, (0, width - int(lp.shape[1])), value=0.0) for _, lp in parts])
        return token_ids, lps

    def score_recording(self, label_notes: np.ndarray, audio_path=None, audio_y=None, sr=None, cond_index=None,
                        min_confidence: Optional[float] = None) -> float:
        """Chroma accuracy of a whole recording against its label notes: ``generate_notes``' segmentation and chunked decode, then
        the sequential detokenising and the scoring on the device.  Equals
        ``evaluate_batch([numpy_to_midi(label_notes)], [self.generate(...)])``; labels the device path does not take, or ids that
        are not on a GPU, are scored on the host from the same ids.  One GPU only.  ``min_confidence`` (``None``:
        ``config.inference.min_note_confidence``) scores only the notes of at least that confidence, as ``generate_notes`` drops
        them; the filter runs on the device, so a sweep over thresholds copies three integers per call to the host."""
        _single_process("score_recording", "score generate()'s notes on the host")
        floor = _min_note_confidence(self.config, min_confidence)
        padded, seg = self._padded_segments(audio_path, audio_y, sr)
        if floor > 0:
            token_ids, lps = self.sample_scored_rows(padded, seg, cond_index)
            duration = self.config.dataset.segment_duration
            if _on_device_scorable(token_ids, [label_notes]):
                return evaluate_tokens(self.model.tokenizer, token_ids, label_notes, mode="sequential", duration_per_batch=duration,
                                       token_logprobs=lps, min_confidence=floor)
            decoded, _ = decode_with_confidence(self.model.tokenizer, token_ids, lps, "sequential", duration, floor)
            return float(evaluate_batch([numpy_to_midi(label_notes)], [numpy_to_midi(decoded)]))
        rows = self.sample_token_rows(padded, seg, cond_index=cond_index)
        duration = self.config.dataset.segment_duration
        width = max(int(r.shape[0]) for r in rows)
        pad = self.model.geometry.pad_token_id
        token_ids = torch.stack([torch.nn.functional.pad(r, (0, width - int(r.shape[0])), value=pad) for r in rows])
        if _on_device_scorable(token_ids, [label_notes]):
            return evaluate_tokens(self.model.tokenizer, token_ids, label_notes, mode="sequential", duration_per_batch=duration)
        decoded = self.model.tokenizer.decode(rows, mode="sequential", duration_per_batch=duration)
        return float(evaluate_batch([numpy_to_midi(label_notes)], [numpy_to_midi(decoded)]))

    # -- note-level precision / recall / F1 over confidence thresholds (music2midi_amd.note_metrics) ------------------------
    @torch.no_grad()
    def note_scores_batch(self, inputs: ModelInputs, thresholds=None, offset_ratio: Optional[float] = 0.2) -> dict:
        """Note-level precision, recall and F1 of one labelled batch for every confidence threshold of ``thresholds`` (``None``:
        ``[0.0]``): ``score_batch``'s decode - with the tokens' log-probabilities when any threshold is positive - then the matching
        on the device, one launch for all thresholds (``evaluation.note_scores_tokens``).  ``{"precision", "recall", "f1"}`` [K]
        float64 micro-averaged over the clips, ``{"tp", "n_est", "n_ref"}`` [K] int64.  ``offset_ratio=None`` matches onsets only.
        Ids that are not on a GPU, or labels the device path does not take, are scored by the definition from the same ids."""
        _single_process("note_scores_batch", "score the decoded notes on the host")
        scored = _any_positive(thresholds)
        tok = self.model.tokenizer
        if scored:
            budget = 4 * max(len(n) for n in inputs.notes_batch)
            token_ids, lps = _scored_decode(self.model, self.config, self._grammar_kwargs(), inputs, budget)
        else:
            token_ids, lps = _labelled_token_ids(self.model, self.config, self._grammar_kwargs(), inputs), None
        score = note_scores_tokens if _on_device_scorable(token_ids, inputs.notes_batch) else note_scores_host
        return score(tok, token_ids, inputs.notes_batch, "batched", None, token_logprobs=lps, thresholds=thresholds,
                     offset_ratio=offset_ratio)

    @torch.no_grad()
    def note_scores_recording(self, label_notes: np.ndarray, audio_path=None, audio_y=None, sr=None, cond_index=None,
                              thresholds=None, offset_ratio: Optional[float] = 0.2) -> dict:
        """``note_scores_batch``'s dict for a whole recording against its label notes: ``score_recording``'s segmentation and
        chunked decode, the sequential detokenising and the matching on the device.  One GPU, greedy when a threshold is positive."""
        _single_process("note_scores_recording", "score generate()'s notes on the host")
        scored = _any_positive(thresholds)
        padded, seg = self._padded_segments(audio_path, audio_y, sr)
        duration = self.config.dataset.segment_duration
        if scored:
            token_ids, lps = self.sample_scored_rows(padded, seg, cond_index)
        else:
            rows = self.sample_token_rows(padded, seg, cond_index=cond_index)
            width = max(int(r.shape[0]) for r in rows)
            pad = self.model.geometry.pad_token_id
            token_ids, lps = torch.stack([torch.nn.functional.pad(r, (0, width - int(r.shape[0])), value=pad) for r in rows]), None
        score = note_scores_tokens if _on_device_scorable(token_ids, [label_notes]) else note_scores_host
        return score(self.model.tokenizer, token_ids, label_notes, "sequential", duration, token_logprobs=lps, thresholds=thresholds,
                     offset_ratio=offset_ratio)

    # -- frame-level precision / recall / F1 and the TP / FN / FP error roll (music2midi_amd.frame_metrics) -----------------
    @torch.no_grad()
    def frame_scores_batch(self, inputs: ModelInputs, thresholds=None) -> dict:
        """Frame-level precision, recall and F1 of one labelled batch for every confidence threshold of ``thresholds`` (``None``:
        ``[0.0]``), on the full piano roll and, with a ``melody_`` prefix, on the 12-row melody roll: ``note_scores_batch``'s decode
        and routing, then the rolls on the device, one launch for all thresholds (``evaluation.frame_scores_tokens``).  Ids that are
        not on a GPU, or labels the device path does not take, are scored by the definition from the same ids."""
        _single_process("frame_scores_batch", "score the decoded notes on the host")
        scored = _any_positive(thresholds)
        if scored:
            budget = 4 * max(len(n) for n in inputs.notes_batch)
            token_ids, lps = _scored_decode(self.model, self.config, self._grammar_kwargs(), inputs, budget)
        else:
            token_ids, lps = _labelled_token_ids(self.model, self.config, self._grammar_kwargs(), inputs), None
        score = frame_scores_tokens if _on_device_scorable(token_ids, inputs.notes_batch) else frame_scores_host
        return score(self.model.tokenizer, token_ids, inputs.notes_batch, "batched", None, token_logprobs=lps, thresholds=thresholds)

    def _recording_token_ids(self, audio_path, audio_y, sr, cond_index, scored: bool):
        """(ids [segments, W], log-probabilities or ``None``) of a whole recording: ``note_scores_recording``'s decode."""
        padded, seg = self._padded_segments(audio_path, audio_y, sr)
        if scored:
            return self.sample_scored_rows(padded, seg, cond_index)
        rows = self.sample_token_rows(padded, seg, cond_index=cond_index)
        width = max(int(r.shape[0]) for r in rows)
        pad = self.model.geometry.pad_token_id
        return torch.stack([torch.nn.functional.pad(r, (0, width - int(r.shape[0])), value=pad) for r in rows]), None

    @torch.no_grad()
    def frame_scores_recording(self, label_notes: np.ndarray, audio_path=None, audio_y=None, sr=None, cond_index=None,
                               thresholds=None) -> dict:
        """``frame_scores_batch``'s dict for a whole recording against its label notes: ``note_scores_recording``'s segmentation and
        chunked decode, the sequential detokenising and the rolls on the device.  One GPU, greedy when a threshold is positive."""
        _single_process("frame_scores_recording", "score generate()'s notes on the host")
        token_ids, lps = self._recording_token_ids(audio_path, audio_y, sr, cond_index, _any_positive(thresholds))
        score = frame_scores_tokens if _on_device_scorable(token_ids, [label_notes]) else frame_scores_host
        return score(self.model.tokenizer, token_ids, label_notes, "sequential", self.config.dataset.segment_duration, token_logprobs=lps,
                     thresholds=thresholds)

    @torch.no_grad()
    def error_midi_recording(self, label_notes: np.ndarray, audio_path=None, audio_y=None, sr=None, cond_index=None,
                             melody_only: bool = False, min_confidence: Optional[float] = None):
        """Where the transcription of a recording is right, misses and adds: the MIDI object with the instruments TP, FN and FP
        (programs 0, 1, 2) of ``frame_metrics.evaluate_midi_result(label_notes, generate_notes(...), melody_only)``, with the rolls
        and the notes extracted on the device (``scoring.error_notes``); it can be ``.write()``n and ``.synthesize()``d.
        ``min_confidence`` as in ``score_recording``.  Ids that are not on a GPU, or labels the device path does not take, go
        through the definition from the same ids.  One GPU only."""
        from .frame_metrics import error_midi, evaluate_midi_result
        _single_process("error_midi_recording", "compare generate()'s notes on the host")
        floor = _min_note_confidence(self.config, min_confidence)
        token_ids, lps = self._recording_token_ids(audio_path, audio_y, sr, cond_index, floor > 0)
        tok, duration = self.model.tokenizer, self.config.dataset.segment_duration
        if _on_device_scorable(token_ids, [label_notes]):
            from .scoring import error_notes
            found = error_notes(tok, token_ids, label_notes, "sequential", duration, melody_only=melody_only, token_logprobs=lps,
                                min_confidence=floor if lps is not None else 0.0)
            return error_midi(*found.to_numpy()[0])
        if lps is None:
            decoded = tok.decode(token_ids, mode="sequential", duration_per_batch=duration)
        else:
            decoded, _ = decode_with_confidence(tok, token_ids, lps, "sequential", duration, floor)
        return evaluate_midi_result(np.asarray(label_notes, dtype=np.float64), decoded, melody_only)
