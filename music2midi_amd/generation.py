"""Keyword surface of ``T5Transformer.generate`` (pure Python: no torch, no library).

``resolve_generate_kwargs`` turns the keywords a caller of HF's ``generate`` may pass into the decoding mode the
MI355X path runs, with transformers 4.34's ``GenerationConfig`` defaults (hf: generation/configuration_utils.py:
``max_length=20``, ``do_sample=False``, ``temperature=1.0``, ``top_k=50``, ``top_p=1.0``, ``num_return_sequences=1``)
and the argument checks of its logits warpers (hf: generation/logits_process.py ``TemperatureLogitsWarper``,
``TopKLogitsWarper``, ``TopPLogitsWarper``), which raise ``ValueError``.  The logits-processor keywords (``repetition_penalty``,
``no_repeat_ngram_size``, ``bad_words_ids``, ``min_length``, ``min_new_tokens``, ``forced_bos_token_id``,
``forced_eos_token_id``, ``suppress_tokens``, ``begin_suppress_tokens``) and ``max_new_tokens`` follow 4.34's
``_get_logits_processor`` and its processors' checks.  Beam search and every other keyword raise
``NotImplementedError`` there (``return_dict_in_generate``, ``output_scores`` and the project keyword ``output_logprobs`` select
the per-token outputs of the scored head; ``midi_grammar`` the token grammar of ``grammar.py``); beam search has its own entry point (``T5Transformer.beam_search``), whose keywords
``resolve_beam_kwargs`` checks, and ``T5Transformer.beam_search_processed`` takes the grammar and the processors that do not read a
row's history under beams (``resolve_beam_process_kwargs``).
"""
from __future__ import annotations

import math
import numbers
import operator
from dataclasses import dataclass

DEFAULT_MAX_LENGTH = 20
DEFAULT_TEMPERATURE = 1.0
DEFAULT_TOP_K = 50
DEFAULT_TOP_P = 1.0

# device limits of the processed head (music2midi_amd/csrc/t5.h PROC_*)
PROCESS_MAX_VOCAB = 4096
PROCESS_MAX_LENGTH = 2048
PROCESS_MAX_BAD_SEQUENCES = 64      # bad-words sequences of two or more ids
PROCESS_MAX_BAD_IDS = 512           # ids in those sequences together


@dataclass(frozen=True)
class ProcessConfig:
    """The active logits processors of a call (transformers 4.34 ``_get_logits_processor``); neutral values are absent ones."""
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    bad_words_ids: tuple = ()            # tuple of tuples of ids, as given (the [eos] entry is filtered where it is applied)
    min_length: int = 0
    min_new_tokens: int = 0
    forced_bos_token_id: int = -1
    forced_eos_token_id: int = -1
    suppress_tokens: tuple = ()
    begin_suppress_tokens: tuple = ()

    @property
    def begin_index(self) -> int:
        """cur_len at which begin_suppress_tokens apply: the decoder prompt length (1), + 1 with forced_bos_token_id (4.34)."""
        return 2 if self.forced_bos_token_id >= 0 else 1


@dataclass(frozen=True)
class GenerateConfig:
    max_length: int = DEFAULT_MAX_LENGTH
    do_sample: bool = False
    temperature: float = DEFAULT_TEMPERATURE
    top_k: int = DEFAULT_TOP_K           # 0: no top-k filter
    top_p: float = DEFAULT_TOP_P         # 1.0: no nucleus filter
    num_return_sequences: int = 1
    process: "ProcessConfig | None" = None   # None: no logits processor (the plain greedy / sampling head)
    return_dict: bool = False            # return_dict_in_generate=True: an output with .sequences / .scores / .logprobs
    output_scores: bool = False          # ... with the row every token was selected from (only with return_dict)
    output_logprobs: bool = False        # ... with every token's log-probability under that row (only with return_dict)
    midi_grammar: bool = False           # mask every step with the MIDI token grammar (grammar.py), at PrefixConstrainedLogitsProcessor's place


def _is_int(v) -> bool:
    if isinstance(v, bool):
        return False
    try:
        operator.index(v)
    except TypeError:
        return False
    return True


def _is_real(v) -> bool:
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def _id_list(name, v, vocab_size):
    if not isinstance(v, (list, tuple)) or not all(_is_int(i) for i in v):
        raise ValueError(f"`{name}` has to be a list of token ids, but is {v!r}")
    ids = tuple(operator.index(i) for i in v)
    _check_ids(name, ids, vocab_size)
    return ids


def _check_ids(name, ids, vocab_size):
    if any(i < 0 for i in ids):
        raise ValueError(f"`{name}` has to hold non-negative token ids, but is {list(ids)!r}")
    if vocab_size is not None and any(i >= vocab_size for i in ids):
        raise ValueError(f"The model vocabulary size is {vocab_size}, but `{name}` holds the ids "
                         f"{sorted({i for i in ids if i >= vocab_size})}")


def resolve_process_kwargs(kw: dict, vocab_size=None) -> "ProcessConfig | None":
    """Pop the logits-processor keywords from ``kw`` and check them (4.34's gates and ``ValueError`` messages; ids outside
    the vocabulary raise too).  -> ``None`` when no processor is active."""
    p = {}
    rp = kw.pop("repetition_penalty", None)
    if rp is not None and rp != 1.0:
        if not isinstance(rp, float) or not (rp > 0):            # RepetitionPenaltyLogitsProcessor
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {rp}")
        if not math.isfinite(rp):
            raise ValueError(f"`repetition_penalty` has to be finite on the MI355X path, but is {rp}")
        p["repetition_penalty"] = float(rp)
    n = kw.pop("no_repeat_ngram_size", None)
    if n is not None and n > 0:
        if not _is_int(n):                                       # NoRepeatNGramLogitsProcessor
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {n}")
        p["no_repeat_ngram_size"] = operator.index(n)
    bw = kw.pop("bad_words_ids", None)
    if bw is not None:                                           # NoBadWordsLogitsProcessor._validate_arguments
        if not isinstance(bw, list) or len(bw) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
        if any(not isinstance(s, list) for s in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
        if any(any(not _is_int(i) or i < 0 for i in s) for s in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
        if any(len(s) == 0 for s in bw):
            raise ValueError(f"`bad_words_ids` holds an empty sequence: {bw}")
        seqs = tuple(tuple(operator.index(i) for i in s) for s in bw)
        _check_ids("bad_words_ids", tuple(i for s in seqs for i in s), vocab_size)
        long_ = [s for s in seqs if len(s) >= 2]
        if len(long_) > PROCESS_MAX_BAD_SEQUENCES or sum(map(len, long_)) > PROCESS_MAX_BAD_IDS:
            raise ValueError(f"`bad_words_ids` holds {len(long_)} sequences of two or more ids with {sum(map(len, long_))} ids: "
                             f"the MI355X processed head takes at most {PROCESS_MAX_BAD_SEQUENCES} such sequences and "
                             f"{PROCESS_MAX_BAD_IDS} ids")
        p["bad_words_ids"] = seqs
    for name in ("min_length", "min_new_tokens"):
        v = kw.pop(name, None)
        if v is not None and v > 0:
            if not _is_int(v):                                   # MinLength / MinNewTokensLength LogitsProcessor
                raise ValueError(f"`{name}` has to be a positive integer, but is {v}" if name == "min_new_tokens" else
                                 f"`min_length` has to be a non-negative integer, but is {v}")
            p[name] = operator.index(v)
    for name in ("forced_bos_token_id", "forced_eos_token_id"):
        v = kw.pop(name, None)
        if v is None:
            continue
        if name == "forced_eos_token_id" and isinstance(v, (list, tuple)):
            if len(v) != 1:
                raise ValueError(f"`forced_eos_token_id` = {v!r}: the MI355X processed head forces one EOS id")
            v = v[0]
        if not _is_int(v):
            raise ValueError(f"`{name}` has to be a token id, but is {v!r}")
        _check_ids(name, (operator.index(v),), vocab_size)
        p[name] = operator.index(v)
    for name in ("suppress_tokens", "begin_suppress_tokens"):
        v = kw.pop(name, None)
        if v is not None:
            ids = _id_list(name, v, vocab_size)
            if ids:
                p[name] = ids
    if not p:
        return None
    if vocab_size is not None and vocab_size > PROCESS_MAX_VOCAB:
        raise ValueError(f"logits processors on the MI355X path need a vocabulary of at most {PROCESS_MAX_VOCAB} ids "
                         f"(the model has {vocab_size})")
    return ProcessConfig(**p)


def resolve_generate_kwargs(kwargs: dict, default_max_length: int = DEFAULT_MAX_LENGTH, vocab_size=None, grammar=None) -> GenerateConfig:
    """Validate ``generate`` keywords and fill in HF's defaults.  ``kwargs`` is not modified.

    ``None`` for temperature / top_k / top_p means "no such warper", as in HF (the warper is only built when the value is
    not None).  With ``do_sample=False`` the sampling keywords are ignored (HF warns and decodes greedily).
    ``max_new_tokens`` sets ``max_length = max_new_tokens + 1`` (the decoder prompt is the start token) and wins over
    ``max_length``, as in 4.34.  ``vocab_size`` (optional) range-checks the processors' token ids.
    ``return_dict_in_generate`` and ``output_scores`` have 4.34's meaning: without ``return_dict_in_generate=True`` the call
    returns the plain tensor and ``output_scores`` is ignored.  ``output_logprobs`` (a keyword of this project: the tokens'
    log-probabilities without the V-wide rows) raises ``ValueError`` unless ``return_dict_in_generate=True``.
    ``midi_grammar`` (a keyword of this project, a bool) constrains every step to the MIDI token grammar, what HF does with
    ``prefix_allowed_tokens_fn=grammar.prefix_allowed_tokens_fn()``; ``grammar`` (the tokenizer's ``MidiGrammar``, optional) is
    checked against the device limits then.  The flag is a field of ``GenerateConfig``, not a processor of ``ProcessConfig``."""
    kw = dict(kwargs)
    max_length = int(kw.pop("max_length", default_max_length))   # range-checked by the library, as before
    max_new = kw.pop("max_new_tokens", None)
    if max_new is not None:
        if not _is_int(max_new) or max_new <= 0:                 # GenerationConfig.validate
            raise ValueError(f"`max_new_tokens` must be greater than 0, but is {max_new}.")
        max_length = operator.index(max_new) + 1
    process = resolve_process_kwargs(kw, vocab_size)
    if process is not None and max_length > PROCESS_MAX_LENGTH:
        raise ValueError(f"logits processors on the MI355X path take max_length <= {PROCESS_MAX_LENGTH}, got {max_length}")
    midi_grammar = kw.pop("midi_grammar", False)
    if not isinstance(midi_grammar, bool):
        raise ValueError(f"`midi_grammar` has to be a bool, but is {midi_grammar!r}")
    if midi_grammar:
        if max_length > PROCESS_MAX_LENGTH:
            raise ValueError(f"`midi_grammar` on the MI355X path takes max_length <= {PROCESS_MAX_LENGTH}, got {max_length}")
        if grammar is not None and vocab_size is not None:
            grammar.check_device_limits(vocab_size)       # pitch ids, special + pitch + time <= vocab_size <= PROCESS_MAX_VOCAB
    do_sample = bool(kw.pop("do_sample", False))
    if int(kw.pop("num_beams", 1)) != 1:
        raise NotImplementedError("generate() does not decode with num_beams > 1 on the MI355X path; "
                                  "use T5Transformer.beam_search (or do_sample=False / do_sample=True)")
    temperature = kw.pop("temperature", DEFAULT_TEMPERATURE)
    top_k = kw.pop("top_k", DEFAULT_TOP_K)
    top_p = kw.pop("top_p", DEFAULT_TOP_P)
    n = kw.pop("num_return_sequences", 1)
    if n is None:
        n = 1
    return_dict = bool(kw.pop("return_dict_in_generate", False))
    output_scores = bool(kw.pop("output_scores", False)) and return_dict
    output_logprobs = bool(kw.pop("output_logprobs", False))
    if kw:
        raise NotImplementedError(f"unsupported generate kwargs on the MI355X path: {sorted(kw)}")
    if output_logprobs and not return_dict:
        raise ValueError("`output_logprobs=True` needs `return_dict_in_generate=True` (a plain tensor has no place for them)")
    if (output_scores or output_logprobs) and vocab_size is not None and vocab_size > PROCESS_MAX_VOCAB:
        raise ValueError(f"per-token scores on the MI355X path need a vocabulary of at most {PROCESS_MAX_VOCAB} ids "
                         f"(the model has {vocab_size})")
    out = dict(return_dict=return_dict, output_scores=output_scores, output_logprobs=output_logprobs, midi_grammar=midi_grammar)
    if not _is_int(n) or n < 1:
        raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {n!r}")
    if not do_sample:
        if n != 1:   # hf: generation/utils.py (greedy mode) raises the same
            raise ValueError("Greedy methods without beam search do not support `num_return_sequences` different than 1 "
                             f"(got {n}).")
        return GenerateConfig(max_length=max_length, process=process, **out)
    # TemperatureLogitsWarper: a strictly positive float
    if temperature is None:
        temperature = DEFAULT_TEMPERATURE
    if not _is_real(temperature) or not math.isfinite(float(temperature)) or not float(temperature) > 0:
        msg = f"`temperature` (={temperature!r}) has to be a strictly positive float, otherwise your next token scores will be invalid."
        if _is_real(temperature) and float(temperature) == 0.0:
            msg += " If you're looking for greedy decoding strategies, set `do_sample=False`."
        raise ValueError(msg)
    # TopKLogitsWarper: a non-negative integer (0 disables it, as HF skips the warper for top_k == 0)
    if top_k is None:
        top_k = 0
    if not _is_int(top_k) or top_k < 0:
        raise ValueError(f"`top_k` has to be a strictly positive integer, but is {top_k!r}")
    # TopPLogitsWarper: a float in [0, 1]
    if top_p is None:
        top_p = DEFAULT_TOP_P
    if not _is_real(top_p) or not (0.0 <= float(top_p) <= 1.0):
        raise ValueError(f"`top_p` has to be a float >= 0 and <= 1, but is {top_p!r}")
    return GenerateConfig(max_length=max_length, do_sample=True, temperature=float(temperature), top_k=operator.index(top_k),
                          top_p=float(top_p), num_return_sequences=operator.index(n), process=process, **out)


BEAM_MAX = 32   # beams per clip the device beam head supports


@dataclass(frozen=True)
class BeamConfig:
    num_beams: int
    max_length: int = DEFAULT_MAX_LENGTH
    length_penalty: float = 1.0
    early_stopping: object = False       # True, False or "never" (transformers 4.34 BeamSearchScorer)
    num_return_sequences: int = 1

    @property
    def early_stopping_code(self) -> int:
        """m2m_beam_params.early_stopping: 0 False, 1 True, 2 "never"."""
        return 2 if self.early_stopping == "never" else int(bool(self.early_stopping))


def resolve_beam_kwargs(num_beams, max_length=DEFAULT_MAX_LENGTH, length_penalty=1.0, early_stopping=False,
                        num_return_sequences=1) -> BeamConfig:
    """Validate ``beam_search`` keywords (transformers 4.34 semantics; raises ``ValueError``)."""
    if not _is_int(num_beams) or num_beams < 1:
        raise ValueError(f"`num_beams` has to be a strictly positive integer, but is {num_beams!r}")
    if num_beams == 1:
        raise ValueError("`num_beams` = 1 is greedy decoding (as in HF): use generate() / generate_from_embeds()")
    if num_beams > BEAM_MAX:
        raise ValueError(f"`num_beams` = {num_beams} is above the {BEAM_MAX} beams per clip the MI355X beam head supports")
    if num_return_sequences is None:
        num_return_sequences = 1
    if not _is_int(num_return_sequences) or num_return_sequences < 1:
        raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {num_return_sequences!r}")
    if num_return_sequences > num_beams:   # hf generation/beam_search.py BeamSearchScorer
        raise ValueError(f"`num_return_sequences` ({num_return_sequences}) has to be smaller or equal to `num_beams` ({num_beams}).")
    if not (early_stopping is True or early_stopping is False or early_stopping == "never"):
        raise ValueError(f"`early_stopping` has to be True, False or \"never\", but is {early_stopping!r}")
    if not _is_real(length_penalty) or not math.isfinite(float(length_penalty)):
        raise ValueError(f"`length_penalty` has to be a finite float, but is {length_penalty!r}")
    if not _is_int(max_length) or max_length < 1:
        raise ValueError(f"`max_length` has to be a strictly positive integer, but is {max_length!r}")
    return BeamConfig(num_beams=operator.index(num_beams), max_length=operator.index(max_length),
                      length_penalty=float(length_penalty), early_stopping=early_stopping,
                      num_return_sequences=operator.index(num_return_sequences))


def resolve_beam_process_kwargs(kwargs: dict, vocab_size=None, grammar=None, max_length=None):
    """The processor keywords and ``midi_grammar`` of ``T5Transformer.beam_search_processed`` -> ``(ProcessConfig | None,
    midi_grammar)``.  ``kwargs`` is not modified.  The checks are ``resolve_process_kwargs``'s and ``grammar.check_device_limits``
    (``ValueError``, as the greedy path raises them; ``max_length``, when given, is held to the processed head's limit too).
    ``repetition_penalty``, ``no_repeat_ngram_size`` and ``bad_words_ids`` sequences of two or more ids raise
    ``NotImplementedError``: they read a row's history, which the beam head does not stage; any other keyword does as well."""
    kw = dict(kwargs)
    midi_grammar = kw.pop("midi_grammar", False)
    if not isinstance(midi_grammar, bool):
        raise ValueError(f"`midi_grammar` has to be a bool, but is {midi_grammar!r}")
    process = resolve_process_kwargs(kw, vocab_size)
    if kw:
        raise NotImplementedError(f"unsupported beam_search_processed kwargs on the MI355X path: {sorted(kw)}")
    if process is not None:
        active = [name for name, on in (("repetition_penalty", process.repetition_penalty != 1.0),
                                        ("no_repeat_ngram_size", process.no_repeat_ngram_size > 0),
                                        ("bad_words_ids", any(len(w) >= 2 for w in process.bad_words_ids))) if on]
        if active:
            raise NotImplementedError(f"beam search on the MI355X path does not apply {', '.join(f'`{a}`' for a in active)} "
                                      "(bad_words_ids: sequences of two or more ids): they read a row's history, which a beam keeps "
                                      "scattered through the ancestry table")
    if (process is not None or midi_grammar) and max_length is not None and max_length > PROCESS_MAX_LENGTH:
        raise ValueError(f"logits processors and `midi_grammar` on the MI355X path take max_length <= {PROCESS_MAX_LENGTH}, got {max_length}")
    if midi_grammar and grammar is not None and vocab_size is not None:
        grammar.check_device_limits(vocab_size)
    return process, midi_grammar
