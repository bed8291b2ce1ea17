"""T5Transformer — MI355X implementation of ref: music2midi/transformer.py:10-45.

Same constructor (``config_path``), same attributes (``transformer``,
``tokenizer``, ``spectrogram``, ``conditioning``, ``t5config``) and the same two
entry points: ``forward(ModelInputs) -> output with .loss/.logits`` and
``generate(ModelInputs, **kwargs) -> LongTensor [B, L]``.  The parameters live in
a module tree whose ``state_dict()`` keys equal HuggingFace T5's, so a reference
checkpoint loads unchanged; the arithmetic runs in the HIP library (encoder,
cross-K/V projection, graph-replayed greedy or sampled decode) — there is no torch
compute path and no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from types import SimpleNamespace
from typing import Optional

import torch
import torch.nn as nn

from . import native
from .config import T5Geometry, load_config
from .generation import GenerateConfig, ProcessConfig, resolve_beam_kwargs, resolve_beam_process_kwargs, resolve_generate_kwargs
from .input import Conditioning, LogMelSpectrogram, ModelInputs
from .tokenizer import EOS, MidiTokenizer

_PRECISIONS = {"fp32": native.PREC_FP32, "bf16": native.PREC_BF16}


# --------------------------------------------------------------------------
# Parameter containers with HuggingFace T5 state-dict names (no compute).
# --------------------------------------------------------------------------
class _Norm(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))


class _Attention(nn.Module):
    def __init__(self, g: T5Geometry, has_bias: bool):
        super().__init__()
        self.q = nn.Linear(g.d_model, g.inner_dim, bias=False)
        self.k = nn.Linear(g.d_model, g.inner_dim, bias=False)
        self.v = nn.Linear(g.d_model, g.inner_dim, bias=False)
        self.o = nn.Linear(g.inner_dim, g.d_model, bias=False)
        if has_bias:
            self.relative_attention_bias = nn.Embedding(g.num_buckets, g.num_heads)


class _GatedFF(nn.Module):
    def __init__(self, g: T5Geometry):
        super().__init__()
        self.wi_0 = nn.Linear(g.d_model, g.d_ff, bias=False)
        self.wi_1 = nn.Linear(g.d_model, g.d_ff, bias=False)
        self.wo = nn.Linear(g.d_ff, g.d_model, bias=False)


class _SubLayer(nn.Module):
    def __init__(self, name: str, inner: nn.Module, d: int):
        super().__init__()
        setattr(self, name, inner)
        self.layer_norm = _Norm(d)


class _Block(nn.Module):
    def __init__(self, g: T5Geometry, is_decoder: bool, first: bool):
        super().__init__()
        layers = [_SubLayer("SelfAttention", _Attention(g, first), g.d_model)]
        if is_decoder:
            layers.append(_SubLayer("EncDecAttention", _Attention(g, False), g.d_model))
        layers.append(_SubLayer("DenseReluDense", _GatedFF(g), g.d_model))
        self.layer = nn.ModuleList(layers)


class _Stack(nn.Module):
    def __init__(self, g: T5Geometry, embed: nn.Embedding, is_decoder: bool):
        super().__init__()
        self.embed_tokens = embed   # same module as `shared`: state_dict carries the HF alias keys
        n = g.num_decoder_layers if is_decoder else g.num_layers
        self.block = nn.ModuleList([_Block(g, is_decoder, i == 0) for i in range(n)])
        self.final_layer_norm = _Norm(g.d_model)


class T5Parameters(nn.Module):
    """Holds the T5 weights under HF names; initialised like HF's ``_init_weights``
    (hf: models/t5/modeling_t5.py:563-616) with an UNTIED ``lm_head`` — the
    transformers-4.34 meaning of ``tie_word_embeddings: false`` (ref: config.yaml:23)."""

    def __init__(self, g: T5Geometry):
        super().__init__()
        self.geometry = g
        self.shared = nn.Embedding(g.vocab_size, g.d_model)
        self.encoder = _Stack(g, self.shared, False)
        self.decoder = _Stack(g, self.shared, True)
        self.lm_head = nn.Linear(g.d_model, g.vocab_size, bias=False)
        self.config = SimpleNamespace(**g.as_dict(), is_encoder_decoder=True, tie_word_embeddings=False)
        self._init_weights()

    @torch.no_grad()
    def _init_weights(self):
        g = self.geometry
        d, dk, H, dff = g.d_model, g.d_kv, g.num_heads, g.d_ff
        self.shared.weight.normal_(0.0, 1.0)
        self.lm_head.weight.normal_(0.0, 1.0)
        for m in self.modules():
            if isinstance(m, _Attention):
                m.q.weight.normal_(0.0, (d * dk) ** -0.5)
                m.k.weight.normal_(0.0, d ** -0.5)
                m.v.weight.normal_(0.0, d ** -0.5)
                m.o.weight.normal_(0.0, (H * dk) ** -0.5)
                if hasattr(m, "relative_attention_bias"):
                    m.relative_attention_bias.weight.normal_(0.0, d ** -0.5)
            elif isinstance(m, _GatedFF):
                m.wi_0.weight.normal_(0.0, d ** -0.5)
                m.wi_1.weight.normal_(0.0, d ** -0.5)
                m.wo.weight.normal_(0.0, dff ** -0.5)

    @property
    def device(self) -> torch.device:
        return self.shared.weight.device

    def forward(self, *a, **k):
        raise RuntimeError("T5Parameters only stores weights; use T5Transformer.forward/generate")


class Seq2SeqOutput(dict):
    """Minimal stand-in for HF's Seq2SeqLMOutput: attribute and key access to loss/logits."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError as e:
            raise AttributeError(name) from e


class GenerateOutput(Seq2SeqOutput):
    """``generate(return_dict_in_generate=True)``: ``sequences`` [B * n, L]; ``scores``: a tuple of L - 1 tensors [B * n, V] (the
    unbound views of one buffer), or ``None``; ``logprobs`` [B * n, L - 1] float32, or ``None``."""


class ConsensusOutput(Seq2SeqOutput):
    """``generate_consensus(return_candidates=True)``: ``sequences`` [B, W] the chosen rows; ``candidates`` [B, K, W] with the greedy
    row first; ``chosen`` [B] int32; ``utility`` [B, K] float64; ``tp`` [B, K, K] and ``n`` [B, K] int32 - all on the device."""


def _consensus_arguments(num_samples, keywords: dict) -> int:
    """K of a consensus decode; ``ValueError`` for a K outside 2..16 or beams, ``NotImplementedError`` with a process group of more
    than one rank (the candidates of a clip are not gathered across ranks)."""
    from .consensus import check_candidates
    K = check_candidates(num_samples, "generate_consensus: num_samples")
    if "num_beams" in keywords:
        raise ValueError("generate_consensus: num_beams is not supported - the candidates are one greedy and num_samples - 1 sampled rows")
    for name in ("do_sample", "num_return_sequences", "return_dict_in_generate", "output_scores", "output_logprobs"):
        if name in keywords:
            raise ValueError(f"generate_consensus: {name} is set by the consensus decode itself")
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError("generate_consensus runs on one GPU: with a process group, decode on one rank")
    return K


# --------------------------------------------------------------------------
class T5Transformer(nn.Module):
    def __init__(self, config_path, precision: Optional[str] = None):
        super().__init__()
        self.config = load_config(config_path)
        self.geometry = T5Geometry(self.config.model.t5)
        self.t5config = SimpleNamespace(**self.geometry.as_dict())

        self.transformer = T5Parameters(self.geometry)
        self.tokenizer = MidiTokenizer(self.config)
        self.spectrogram = LogMelSpectrogram(
            sample_rate=self.config.model.sample_rate,
            n_mels=self.config.model.t5.d_model,
            **self.config.spectrogram,
        )
        self.conditioning = Conditioning(
            self.config.model.t5.d_model,
            [len(v) for v in self.config.conditioning.values()],
        )
        # The reference runs inference in fp32 (SURVEY.md §5 "precision flags"); fp32 is the
        # default so token ids match it.  "bf16" is the throughput mode (BASELINE config 3).
        self.precision = precision or os.environ.get("M2M_PRECISION", "fp32")
        if self.precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {self.precision!r}")
        self._lock = threading.RLock()   # a session is not re-entrant (threaded Flask dev server)
        self._model_handle = None
        self._model_key = None
        self._session = None
        self._session_key = None
        self._workspace = None
        self._keepalive = None

    # -- native objects ------------------------------------------------------
    def set_precision(self, precision: str) -> "T5Transformer":
        if precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
        if precision != self.precision:
            self.precision = precision
            self._drop_native()
        return self

    def _drop_native(self):
        lib = native.load()
        if self._session is not None:
            lib.m2m_session_destroy(self._session)
            self._session = None
            self._session_key = None
            self._workspace = None
        if self._model_handle is not None:
            lib.m2m_model_destroy(self._model_handle)
            self._model_handle = None
            self._model_key = None

    def __del__(self):
        try:
            self._drop_native()
        except Exception:
            pass

    def _param_key(self):
        ps = list(self.transformer.parameters())
        # _weights_epoch: bumped by the native trainer, whose in-place kernel updates torch's version counters cannot see
        return (self.precision, str(ps[0].device), getattr(self, "_weights_epoch", 0)) + tuple((p.data_ptr(), p._version) for p in ps)

    def _get_model(self):
        """Repack the current parameters into the library (once per weight version)."""
        native.require_gpu()
        dev = self.transformer.device
        if dev.type != "cuda":
            raise native.NativeError("T5Transformer weights are on the CPU: call .cuda() first "
                                     "(the MI355X path has no CPU fallback)")
        key = self._param_key()
        if self._model_handle is not None and key == self._model_key:
            return self._model_handle
        self._drop_native()
        lib = native.load()
        g, t = self.geometry, self.transformer
        keep = []

        def p(param):
            x = param.detach().to(dtype=torch.float32).contiguous()
            keep.append(x)
            return x.data_ptr()

        def attn(a):
            return p(a.q.weight), p(a.k.weight), p(a.v.weight), p(a.o.weight)

        enc = (native.EncLayerWeights * g.num_layers)()
        for i, blk in enumerate(t.encoder.block):
            sa, ff = blk.layer[0], blk.layer[1]
            q, k, v, o = attn(sa.SelfAttention)
            enc[i] = native.EncLayerWeights(p(sa.layer_norm.weight), q, k, v, o, p(ff.layer_norm.weight),
                                            p(ff.DenseReluDense.wi_0.weight), p(ff.DenseReluDense.wi_1.weight),
                                            p(ff.DenseReluDense.wo.weight))
        dec = (native.DecLayerWeights * g.num_decoder_layers)()
        for i, blk in enumerate(t.decoder.block):
            sa, ca, ff = blk.layer[0], blk.layer[1], blk.layer[2]
            q, k, v, o = attn(sa.SelfAttention)
            cq, ck, cv, co = attn(ca.EncDecAttention)
            dec[i] = native.DecLayerWeights(p(sa.layer_norm.weight), q, k, v, o, p(ca.layer_norm.weight), cq, ck, cv, co,
                                            p(ff.layer_norm.weight), p(ff.DenseReluDense.wi_0.weight),
                                            p(ff.DenseReluDense.wi_1.weight), p(ff.DenseReluDense.wo.weight))
        w = native.T5Weights(
            p(t.shared.weight), p(t.lm_head.weight),
            p(t.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight),
            p(t.decoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight),
            p(t.encoder.final_layer_norm.weight), p(t.decoder.final_layer_norm.weight), enc, dec)
        geom = native.T5GeometryC(g.d_model, g.d_ff, g.num_layers, g.num_decoder_layers, g.num_heads, g.d_kv,
                                  g.vocab_size, g.num_buckets, g.max_distance, g.pad_token_id, g.eos_token_id,
                                  g.decoder_start_token_id, g.eps)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            native.check(lib.m2m_model_create(C.byref(geom), C.byref(w), _PRECISIONS[self.precision],
                                              native.stream_handle(dev), C.byref(h)), "m2m_model_create")
        del keep
        self._model_handle, self._model_key = h, key
        return h

    def device_weights_checksum(self) -> int:
        """64-bit checksum of the REPACKED device weights the kernels read (``m2m_model_checksum``).  After the multi-GPU weight
        broadcast every rank's value must be the same (``distributed.verify_replicas``)."""
        h = self._get_model()
        out = C.c_uint64(0)
        dev = self.transformer.device
        with torch.cuda.device(dev):
            native.check(native.load().m2m_model_checksum(h, C.byref(out), native.stream_handle(dev)), "m2m_model_checksum")
        return int(out.value)

    def _get_session(self, B: int, S: int, L: int):
        model = self._get_model()
        lib = native.load()
        if self._session is not None:
            mb, ms, ml = self._session_key
            if B <= mb and S <= ms and L <= ml:
                return self._session
            B, S, L = max(B, mb), max(S, ms), max(L, ml)
            lib.m2m_session_destroy(self._session)
            self._session, self._workspace = None, None
        dev = self.transformer.device
        nbytes = lib.m2m_session_workspace_bytes(model, B, S, L)
        if nbytes < 0:
            native.check(int(nbytes), "m2m_session_workspace_bytes")
        self._workspace = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)
        base = (self._workspace.data_ptr() + 255) // 256 * 256
        h = C.c_void_p()
        with torch.cuda.device(dev):
            native.check(lib.m2m_session_create(model, B, S, L, base, int(nbytes), C.byref(h)), "m2m_session_create")
        self._session, self._session_key = h, (B, S, L)
        return h

    # -- pipeline pieces -----------------------------------------------------
    def encoder_inputs(self, inputs: ModelInputs) -> torch.Tensor:
        """waveform + cond_index -> [B, n_cond + frames, d_model], written in place by the two
        frontend kernels (ref transformer.py:42-43 = spectrogram then conditioning concat)."""
        wav = inputs.input_waveform
        dev = self.transformer.device
        wav = wav.to(dev)
        n_cond = len(self.conditioning.embeds)
        F = self.spectrogram.num_frames(wav.shape[1])
        buf = torch.empty((wav.shape[0], n_cond + F, self.geometry.d_model), device=dev, dtype=torch.float32)
        self.spectrogram.forward_into(wav, buf, n_cond)
        self.conditioning.write_rows(inputs.cond_index, buf)
        return buf

    def _encode(self, x: torch.Tensor, max_dec: int, want_states: bool = False, rows: Optional[int] = None):
        B, S, _ = x.shape
        sess = self._get_session(max(B, rows or 0), S, max_dec)
        enc_out = torch.empty_like(x) if want_states else None
        with torch.cuda.device(x.device):
            native.check(native.load().m2m_encode(sess, x.data_ptr(), B, S,
                                                  enc_out.data_ptr() if want_states else None,
                                                  native.stream_handle(x.device)), "m2m_encode")
        return sess, enc_out

    @torch.no_grad()
    def encode(self, inputs_embeds: torch.Tensor) -> torch.Tensor:
        """Encoder stack only: [B, S, d] -> final encoder states [B, S, d] fp32 (parity hook)."""
        with self._lock:
            x = inputs_embeds.to(self.transformer.device, torch.float32).contiguous()
            _, out = self._encode(x, 8, want_states=True)
            return out

    @torch.no_grad()
    def generate_from_embeds(self, inputs_embeds: torch.Tensor, max_length: int = 20, **kwargs):
        """Decode from encoder inputs [B, S, d].  Keywords as :meth:`generate` (``do_sample``, ``temperature``, ``top_k``,
        ``top_p``, ``num_return_sequences``, the logits processors, ``max_new_tokens``, ``return_dict_in_generate`` with
        ``output_scores`` / ``output_logprobs``, ``midi_grammar``); without ``do_sample=True`` this is the greedy decode."""
        cfg = (resolve_generate_kwargs(kwargs, default_max_length=max_length, vocab_size=self.geometry.vocab_size,
                                       grammar=self.tokenizer.grammar if kwargs.get("midi_grammar") is True else None) if kwargs
               else GenerateConfig(max_length=max_length))
        return self._decode(inputs_embeds, cfg)

    @staticmethod
    def _process_params(pc: ProcessConfig) -> "native.ProcessParams":
        """The ``m2m_process_params`` block of the resolved processors (the block keeps its id lists alive)."""
        def ids(v):
            return (C.c_int32 * max(len(v), 1))(*v), len(v)

        supp, n_supp = ids(pc.suppress_tokens)
        begin, n_begin = ids(pc.begin_suppress_tokens)
        bad, _ = ids([i for w in pc.bad_words_ids for i in w])
        bad_len, n_bad = ids([len(w) for w in pc.bad_words_ids])
        pp = native.ProcessParams(pc.repetition_penalty, pc.no_repeat_ngram_size, pc.min_length, pc.min_new_tokens,
                                  pc.forced_bos_token_id, pc.forced_eos_token_id, supp, n_supp, begin, n_begin, bad, bad_len, n_bad)
        pp._lists = (supp, begin, bad, bad_len)
        return pp

    @torch.no_grad()
    def _decode(self, inputs_embeds: torch.Tensor, cfg: GenerateConfig):
        """Greedy, sampled or processed decode of encoder inputs [B, S, d] as the resolved ``cfg`` asks."""
        sp = pp = None
        if cfg.do_sample:
            # the call's seed: one draw from torch's default CPU generator, so torch.manual_seed(n) makes the call reproducible
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())
            sp = native.SampleParams(cfg.temperature, cfg.top_k, cfg.top_p, seed)
        if cfg.process is not None:
            pp = self._process_params(cfg.process)
            export, params = "m2m_generate_processed", (C.byref(pp), C.byref(sp) if sp is not None else None)
        elif sp is not None:
            export, params = "m2m_generate_sample", (C.byref(sp),)
        else:
            export, params = "m2m_generate_greedy", ()
        if cfg.return_dict:    # the scored head writes the outputs as it selects the token (the library zeroes both buffers first)
            export, params = "m2m_generate_scored", (C.byref(pp) if pp is not None else None, C.byref(sp) if sp is not None else None)
        if cfg.midi_grammar:   # the processed (or scored) head with the token grammar's mask; without a processor, over a neutral block
            gr = self.tokenizer.grammar             # (its limits: resolve_generate_kwargs; the library checks the block again)
            if self.geometry.eos_token_id != EOS:
                raise ValueError(f"`midi_grammar` ends a sequence with the tokenizer's EOS ({EOS}); the model's eos_token_id is "
                                 f"{self.geometry.eos_token_id}")
            gp = native.GrammarParams(gr.pitch_offset, gr.n_pitch, gr.n_time)
            export, params = "m2m_generate_grammar", (C.byref(gp), C.byref(pp) if pp is not None else None,
                                                      C.byref(sp) if sp is not None else None)
        with self._lock:
            x = inputs_embeds.to(self.transformer.device, torch.float32)
            if cfg.num_return_sequences > 1:      # HF's expansion: the n sequences of a clip are consecutive rows
                x = x.repeat_interleave(cfg.num_return_sequences, dim=0)
            x = x.contiguous()
            sess, _ = self._encode(x, cfg.max_length)
            rows, steps, dev = x.shape[0], cfg.max_length - 1, x.device
            tokens = torch.empty((rows, cfg.max_length), dtype=torch.long, device=dev)
            scores = logprobs = None
            outs = ()
            if cfg.return_dict:
                if cfg.output_scores:
                    scores = torch.empty((steps, rows, self.geometry.vocab_size), dtype=torch.float32, device=dev)
                if cfg.output_logprobs:
                    logprobs = torch.empty((rows, steps), dtype=torch.float32, device=dev)
                outs = tuple(t.data_ptr() if t is not None and t.numel() else None for t in (scores, logprobs))
            elif cfg.midi_grammar:
                outs = (None, None)
            out_len = C.c_int(0)
            with torch.cuda.device(dev):
                native.check(getattr(native.load(), export)(sess, cfg.max_length, *params, tokens.data_ptr(), *outs, C.byref(out_len),
                                                            native.stream_handle(dev)), export)
            n = out_len.value
            if not cfg.return_dict:
                return tokens[:, :n]
            return GenerateOutput(sequences=tokens[:, :n],
                                  scores=tuple(scores[: n - 1].unbind(0)) if scores is not None else None,
                                  logprobs=logprobs[:, : n - 1] if logprobs is not None else None)

    @staticmethod
    def compute_transition_scores(sequences: torch.Tensor, scores, beam_indices=None, normalize_logits: bool = False) -> torch.Tensor:
        """transformers 4.34's ``GenerationMixin.compute_transition_scores`` for the non-beam case: the score of every generated
        token, [B, len(scores)] - ``scores[t][b, sequences[b, t - len(scores)]]``, after a ``log_softmax`` over the vocabulary with
        ``normalize_logits=True`` (then equal to ``generate(output_logprobs=True).logprobs`` up to rounding, wherever a row had
        not finished: finished rows hold zeros here, see :meth:`generate`).  ``beam_indices`` raises ``NotImplementedError``."""
        if beam_indices is not None:
            raise NotImplementedError("compute_transition_scores with beam_indices: beam_search returns sequences_scores only")
        stacked = torch.stack(tuple(scores)).transpose(0, 1)                  # [B, T, V]
        if normalize_logits:
            stacked = torch.nn.functional.log_softmax(stacked, dim=-1)
        idx = sequences[:, sequences.shape[-1] - stacked.shape[1]:].to(stacked.device)
        return stacked.gather(2, idx.unsqueeze(-1)).squeeze(-1)

    @torch.no_grad()
    def beam_search_from_embeds(self, inputs_embeds: torch.Tensor, num_beams: int, max_length: int = 20,
                                length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                                return_scores: bool = False):
        """Beam search from encoder inputs [B, S, d]; keywords and result as :meth:`beam_search`."""
        cfg = resolve_beam_kwargs(num_beams, max_length, length_penalty, early_stopping, num_return_sequences)
        with self._lock:
            x = inputs_embeds.to(self.transformer.device, torch.float32).contiguous()
            B, n = x.shape[0], cfg.num_return_sequences
            sess, _ = self._encode(x, cfg.max_length, rows=B * cfg.num_beams)   # encoded once per clip, decoded as B x nb rows
            tokens = torch.empty((B * n, cfg.max_length), dtype=torch.long, device=x.device)
            scores = torch.empty((B * n,), dtype=torch.float32, device=x.device) if return_scores else None
            out_len = C.c_int(0)
            p = native.BeamParams(cfg.num_beams, cfg.length_penalty, cfg.early_stopping_code, n)
            with torch.cuda.device(x.device):
                native.check(native.load().m2m_generate_beam(sess, cfg.max_length, C.byref(p), tokens.data_ptr(),
                                                             scores.data_ptr() if return_scores else None, C.byref(out_len),
                                                             native.stream_handle(x.device)), "m2m_generate_beam")
            ids = tokens[:, : out_len.value]
            return (ids, scores) if return_scores else ids

    def beam_search(self, inputs: ModelInputs, num_beams: int, max_length: int = 20, length_penalty: float = 1.0,
                    early_stopping=False, num_return_sequences: int = 1, return_scores: bool = False):
        """Beam search decoding with transformers 4.34 semantics (``generate(num_beams=..., do_sample=False)``).

        Returns ``LongTensor [B * num_return_sequences, L]`` in HF's order: the n sequences of a clip are consecutive rows,
        best first, EOS-terminated and right-padded with pad_token_id.  With ``return_scores=True`` also HF's
        ``sequences_scores`` (float32 [B * n], length-normalised: sum of log-probs / len ** length_penalty).
        ``early_stopping`` is True, False or "never"; ``num_beams`` is 2..32.  Each clip is encoded once; its beams share
        its cross-attention K/V and read their self-attention K/V through an ancestry table on the GPU.
        ``generate(num_beams > 1)`` still raises ``NotImplementedError``; beam sampling and group / diverse beams are not
        implemented.  The token grammar and the logits processors under beams: :meth:`beam_search_processed`."""
        encoder_inputs = self.encoder_inputs(inputs)
        return self.beam_search_from_embeds(encoder_inputs, num_beams, max_length=max_length, length_penalty=length_penalty,
                                            early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                                            return_scores=return_scores)

    @torch.no_grad()
    def beam_search_processed_from_embeds(self, inputs_embeds: torch.Tensor, num_beams: int, max_length: int = 20,
                                          length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1,
                                          return_scores: bool = False, midi_grammar: bool = False, **processor_keywords):
        """Beam search under the token grammar and the logits processors from encoder inputs [B, S, d]; keywords and result as
        :meth:`beam_search_processed`."""
        kw = dict(processor_keywords)
        max_new = kw.pop("max_new_tokens", None)
        if max_new is not None:                                      # as generate: the decoder prompt is the start token
            if isinstance(max_new, bool) or not isinstance(max_new, int) or max_new <= 0:
                raise ValueError(f"`max_new_tokens` must be greater than 0, but is {max_new}.")
            max_length = max_new + 1
        cfg = resolve_beam_kwargs(num_beams, max_length, length_penalty, early_stopping, num_return_sequences)
        kw["midi_grammar"] = midi_grammar
        pc, gram = resolve_beam_process_kwargs(kw, self.geometry.vocab_size, self.tokenizer.grammar if midi_grammar is True else None,
                                               max_length=cfg.max_length)
        pp = self._process_params(pc) if pc is not None else None
        gp = None
        if gram:
            gr = self.tokenizer.grammar
            if self.geometry.eos_token_id != EOS:
                raise ValueError(f"`midi_grammar` ends a sequence with the tokenizer's EOS ({EOS}); the model's eos_token_id is "
                                 f"{self.geometry.eos_token_id}")
            gp = native.GrammarParams(gr.pitch_offset, gr.n_pitch, gr.n_time)
        with self._lock:
            x = inputs_embeds.to(self.transformer.device, torch.float32).contiguous()
            B, n = x.shape[0], cfg.num_return_sequences
            sess, _ = self._encode(x, cfg.max_length, rows=B * cfg.num_beams)   # encoded once per clip, decoded as B x nb rows
            tokens = torch.empty((B * n, cfg.max_length), dtype=torch.long, device=x.device)
            scores = torch.empty((B * n,), dtype=torch.float32, device=x.device) if return_scores else None
            out_len = C.c_int(0)
            p = native.BeamParams(cfg.num_beams, cfg.length_penalty, cfg.early_stopping_code, n)
            with torch.cuda.device(x.device):
                native.check(native.load().m2m_generate_beam_processed(
                    sess, cfg.max_length, C.byref(p), C.byref(gp) if gp is not None else None, C.byref(pp) if pp is not None else None,
                    tokens.data_ptr(), scores.data_ptr() if return_scores else None, C.byref(out_len),
                    native.stream_handle(x.device)), "m2m_generate_beam_processed")
            ids = tokens[:, : out_len.value]
            return (ids, scores) if return_scores else ids

    def beam_search_processed(self, inputs: ModelInputs, num_beams: int, max_length: int = 20, length_penalty: float = 1.0,
                              early_stopping=False, num_return_sequences: int = 1, return_scores: bool = False,
                              midi_grammar: bool = False, **processor_keywords):
        """:meth:`beam_search` with a non-empty ``logits_processor`` (transformers 4.34 ``generate(num_beams=...,
        prefix_allowed_tokens_fn=..., min_length=..., forced_eos_token_id=...)``): the most probable WELL-FORMED transcription.

        Every step processes a row's ``log_softmax`` against its own beam's prefix before the beam score is added, in 4.34's
        order: one-id ``bad_words_ids``, ``min_length``, ``min_new_tokens``, the MIDI token grammar (``midi_grammar=True``, at
        ``PrefixConstrainedLogitsProcessor``'s place; a per-row state on the GPU that follows its parent when beams reorder),
        ``forced_bos_token_id``, ``forced_eos_token_id`` (a forced id wins over the grammar), ``suppress_tokens``,
        ``begin_suppress_tokens``.  ``max_new_tokens`` sets ``max_length = max_new_tokens + 1``.  ``repetition_penalty``,
        ``no_repeat_ngram_size`` and ``bad_words_ids`` sequences of two or more ids raise ``NotImplementedError`` (they read a row's
        history); invalid values raise ``ValueError``.  Shapes, order and ``return_scores`` are :meth:`beam_search`'s.  Where a clip
        has fewer than ``num_beams`` finite candidates (the ``forced_eos_token_id`` step) its beams are filled from candidates at
        ``-inf`` as in HF, and a returned sequence may have the score ``-inf``.  Without a processor and with
        ``midi_grammar=False`` the call is :meth:`beam_search`."""
        encoder_inputs = self.encoder_inputs(inputs)
        return self.beam_search_processed_from_embeds(encoder_inputs, num_beams, max_length=max_length, length_penalty=length_penalty,
                                                      early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                                                      return_scores=return_scores, midi_grammar=midi_grammar, **processor_keywords)

    @torch.no_grad()
    def logits_from_embeds(self, inputs_embeds: torch.Tensor, decoder_input_ids: torch.Tensor) -> torch.Tensor:
        with self._lock:
            x = inputs_embeds.to(self.transformer.device, torch.float32).contiguous()
            ids = decoder_input_ids.to(x.device, torch.long).contiguous()
            B, Ld = ids.shape
            sess, _ = self._encode(x, Ld)
            logits = torch.empty((B, Ld, self.geometry.vocab_size), dtype=torch.float32, device=x.device)
            with torch.cuda.device(x.device):
                native.check(native.load().m2m_decode_forced(sess, ids.data_ptr(), Ld, logits.data_ptr(),
                                                             native.stream_handle(x.device)), "m2m_decode_forced")
            return logits

    def repack_stats(self):
        """(re-packings, rows moved) of the last greedy or sampled decode on the current session: how often the live rows were moved into
        the first slots after a quarter of them had emitted EOS (``m2m_session_repack_stats``)."""
        with self._lock:
            if self._session is None:
                return 0, 0
            a, b = C.c_int(0), C.c_int(0)
            native.check(native.load().m2m_session_repack_stats(self._session, C.byref(a), C.byref(b)), "m2m_session_repack_stats")
            return int(a.value), int(b.value)

    def bench_kernel(self, which: int, self_len: int, iters: int):
        """Time one decode kernel in isolation on the current session (after an encode):
        returns (avg microseconds per launch, algorithmic bytes per launch)."""
        with self._lock:
            if self._session is None:
                raise native.NativeError("bench_kernel needs a prior generate/encode on this model")
            us, nbytes = C.c_float(0), C.c_int64(0)
            dev = self.transformer.device
            with torch.cuda.device(dev):
                native.check(native.load().m2m_bench_kernel(self._session, which, self_len, iters, C.byref(us),
                                                            C.byref(nbytes), native.stream_handle(dev)),
                             "m2m_bench_kernel")
            return float(us.value), int(nbytes.value)

    # -- labels ----------------------------------------------------------------
    _label_stream = None

    def device_labels(self, notes_batch, bucket: int = 1, enabled: Optional[bool] = None):
        """With ``config.trainer.device_labels: true`` (absent: off; ``enabled`` is the key as the caller's own config has it, None:
        this module's), the model on a GPU and notes ``tokenize.notes_eligible`` accepts:
        ``tokenizer(notes_batch)`` with PAD -> -100, rounded up to ``bucket`` columns with -100, written on the device
        (``music2midi_amd.tokenize``) - equal to the tensor the host builds.  Otherwise None, and the caller takes the host path.
        The kernel runs on a side stream of this model, so the read-back of the row lengths waits for that stream alone and not for
        the training step in flight; the current stream is ordered behind the kernel's event before it reads the labels."""
        device = self.transformer.device
        if enabled is None:
            enabled = bool(self.config.get("trainer", {}).get("device_labels", False))
        if device.type != "cuda" or not enabled:
            return None
        from .tokenize import training_labels
        if self._label_stream is None or self._label_stream.device != device:
            self._label_stream = torch.cuda.Stream(device=device)
        return training_labels(self.tokenizer, notes_batch, device, self.geometry.pad_token_id, bucket, self._label_stream)

    # -- reference API -------------------------------------------------------
    def forward(self, inputs: ModelInputs, **kwargs):
        """Teacher-forced pass (ref transformer.py:28-39): labels from the tokenizer, pad -> -100,
        decoder inputs = shift_right(labels) (hf: modeling_t5.py:618-637), loss = mean CE over
        non-ignored positions.  Inference-only: no autograd graph is built (training is a
        later row of SURVEY.md §8f)."""
        if kwargs:
            raise NotImplementedError(f"unsupported forward kwargs on the MI355X path: {sorted(kwargs)}")
        g = self.geometry
        labels = self.device_labels(inputs.notes_batch)
        if labels is None:
            labels = self.tokenizer(inputs.notes_batch)
            labels[labels == g.pad_token_id] = -100
            labels = labels.to(self.transformer.device)
        encoder_inputs = self.encoder_inputs(inputs)
        dec_in = torch.full_like(labels, g.decoder_start_token_id)
        dec_in[:, 1:] = labels[:, :-1]
        dec_in[dec_in == -100] = g.pad_token_id
        logits = self.logits_from_embeds(encoder_inputs, dec_in)
        loss = torch.nn.functional.cross_entropy(logits.reshape(-1, g.vocab_size), labels.reshape(-1), ignore_index=-100)
        return Seq2SeqOutput(loss=loss, logits=logits)

    _GENERATE_DEFAULT_MAX_LENGTH = 20   # HF GenerationConfig default when max_length is not given

    def generate(self, inputs: ModelInputs, **kwargs):
        """Decode (ref transformer.py:41-45, which forwards every keyword to HF ``generate``).

        Greedy by default (``do_sample=False``; the reference itself only ever passes ``max_length``, ref
        model.py:58,134).  ``do_sample=True`` samples with transformers 4.34's logits warpers and defaults:
        ``temperature=1.0``, ``top_k=50``, ``top_p=1.0`` (``top_k=0`` / ``top_p=1.0`` disable a filter), and
        ``num_return_sequences=n`` returns n sequences per clip as consecutive rows ([B * n, L], HF's order) - the clips
        are repeated before the encoder, so that costs n encoder passes per clip.  The call's seed is one
        ``torch.randint`` from torch's default CPU generator, so ``torch.manual_seed`` makes a call reproducible; the ids
        are NOT HF's samples for the same seed (the draws come from a counter-based hash on the GPU, not torch's
        generator).  The logits processors of 4.34 run on the GPU before the greedy or sampled select:
        ``repetition_penalty``, ``no_repeat_ngram_size``, ``bad_words_ids``, ``min_length``, ``min_new_tokens``,
        ``forced_bos_token_id``, ``forced_eos_token_id``, ``suppress_tokens``, ``begin_suppress_tokens``; ``max_new_tokens``
        sets ``max_length = max_new_tokens + 1``.  ``return_dict_in_generate=True`` returns an attribute-access dict instead of
        the tensor: ``sequences`` [B * n, L]; with ``output_scores=True`` ``scores``, a tuple of L - 1 float32 tensors [B * n, V] -
        the row each token was selected from, as HF appends it (raw logits for greedy, after the processors, after the warpers
        with removed entries at ``-inf`` for sampling); with ``output_logprobs=True`` (a keyword of this project, the cheap
        form: no V-wide row is written) ``logprobs`` [B * n, L - 1], ``log_softmax(scores[t])[token]``, what
        :meth:`compute_transition_scores` with ``normalize_logits=True`` gives.  Both are written by the decode step as it
        selects the token.  Unlike HF, a row that has emitted EOS is no longer scored: its later positions are 0.0 in both.
        Without ``return_dict_in_generate=True`` ``output_scores`` is ignored (4.34) and ``output_logprobs`` raises
        ``ValueError``.  ``midi_grammar=True`` (a keyword of this project) constrains every step to the MIDI token grammar of
        ``music2midi_amd.grammar`` (``self.tokenizer.grammar``): the ids that cannot follow the row's prefix go to ``-inf`` after the
        ``min_length`` / ``min_new_tokens`` bans and before ``forced_bos_token_id`` - exactly HF's
        ``prefix_allowed_tokens_fn=grammar.prefix_allowed_tokens_fn()``, as a per-clip state machine on the GPU; it combines with
        sampling, every processor and the per-token outputs, and is off by default.  :meth:`beam_search` is unchanged (``sequences_scores`` only;
        :meth:`beam_search_processed` is the beam search that takes the grammar), and ``Music2MIDI.generate_notes`` does not
        carry per-note confidences yet (the tokenizer would have to keep token positions through ``decode``).  Invalid values
        raise ``ValueError``; beam search (``num_beams != 1``) and any other keyword raise ``NotImplementedError``."""
        cfg = resolve_generate_kwargs(kwargs, default_max_length=self._GENERATE_DEFAULT_MAX_LENGTH,
                                      vocab_size=self.geometry.vocab_size,
                                      grammar=self.tokenizer.grammar if kwargs.get("midi_grammar") is True else None)
        return self._decode(self.encoder_inputs(inputs), cfg)

    @torch.no_grad()
    def generate_consensus_from_embeds(self, inputs_embeds: torch.Tensor, num_samples: int, max_length: int = 20, temperature: float = 1.0,
                                       top_k: int = 50, top_p: float = 1.0, midi_grammar: bool = False, return_candidates: bool = False,
                                       **processor_keywords):
        """:meth:`generate_consensus` from encoder inputs [B, S, d]."""
        K = _consensus_arguments(num_samples, processor_keywords)
        from .scoring import _consensus_tensors
        common = dict(processor_keywords, midi_grammar=True) if midi_grammar else dict(processor_keywords)
        greedy = self.generate_from_embeds(inputs_embeds, max_length=max_length, **common)
        sampled = self.generate_from_embeds(inputs_embeds, max_length=max_length, do_sample=True, num_return_sequences=K - 1,
                                            temperature=temperature, top_k=top_k, top_p=top_p, **common)
        B, pad = int(greedy.shape[0]), self.geometry.pad_token_id
        W = max(int(greedy.shape[1]), int(sampled.shape[1]))
        greedy = torch.nn.functional.pad(greedy, (0, W - int(greedy.shape[1])), value=pad)
        sampled = torch.nn.functional.pad(sampled, (0, W - int(sampled.shape[1])), value=pad)
        candidates = torch.cat([greedy.unsqueeze(1), sampled.reshape(B, K - 1, W)], dim=1).contiguous()      # [B, K, W], greedy first
        tp, n, _, chosen, utility = _consensus_tensors("generate_consensus", self.tokenizer, candidates.reshape(B * K, W), K,
                                                       self.geometry.vocab_size, 0.05, 0.2, 0.05, choose=True)
        # (a generated id is inside the vocabulary, so no clip is marked; the clamp keeps the gather in bounds regardless)
        pick = chosen.clamp_min(0).long().reshape(B, 1, 1).expand(B, 1, W)
        sequences = candidates.gather(1, pick).squeeze(1)
        if not return_candidates:
            return sequences
        return ConsensusOutput(sequences=sequences, candidates=candidates, chosen=chosen, utility=utility, tp=tp, n=n)

    def generate_consensus(self, inputs: ModelInputs, num_samples: int, max_length: int = 20, temperature: float = 1.0, top_k: int = 50,
                           top_p: float = 1.0, midi_grammar: bool = False, return_candidates: bool = False, **processor_keywords):
        """Consensus (minimum-Bayes-risk) decode: per clip, the greedy row and ``num_samples - 1`` sampled rows (``temperature``,
        ``top_k``, ``top_p`` as in :meth:`generate`; ``midi_grammar`` and the logits-processor keywords go to both decodes) are
        detokenised on their own in batched mode and scored against each other with the note-level metric of
        ``music2midi_amd.note_metrics``; the row the others agree with most (``music2midi_amd.consensus``; ties go to the greedy row)
        is returned, [B, W] with W the wider of the two decodes, PAD-filled.  The scoring and the selection run on the GPU
        (csrc/consensus.hip) and nothing is copied to the host.  ``return_candidates=True`` returns a :class:`ConsensusOutput` that
        also carries ``candidates`` [B, K, W], ``chosen``, ``utility``, ``tp`` and ``n``.  ``torch.manual_seed`` makes a call
        reproducible, as for sampling.  ``num_samples`` outside 2..16 and ``num_beams`` raise ``ValueError``; a process group of
        more than one rank raises ``NotImplementedError``.  Whether the chosen row is a better transcription than the greedy one
        on a trained model has not been measured."""
        _consensus_arguments(num_samples, processor_keywords)
        return self.generate_consensus_from_embeds(self.encoder_inputs(inputs), num_samples, max_length, temperature, top_k, top_p,
                                                   midi_grammar, return_candidates, **processor_keywords)
