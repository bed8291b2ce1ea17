"""Keyword surface of ``T5Transformer.generate`` (pure Python: no torch, no library).

``resolve_generate_kwargs`` turns the keywords a caller of HF's ``generate`` may pass into the decoding mode the
MI355X path runs, with transformers 4.34's ``GenerationConfig`` defaults (hf: generation/configuration_utils.py:
``max_length=20``, ``do_sample=False``, ``temperature=1.0``, ``top_k=50``, ``top_p=1.0``, ``num_return_sequences=1``)
and the argument checks of its logits warpers (hf: generation/logits_process.py ``TemperatureLogitsWarper``,
``TopKLogitsWarper``, ``TopPLogitsWarper``), which raise ``ValueError``.  Beam search and every other keyword raise
``NotImplementedError`` there; beam search has its own entry point (``T5Transformer.beam_search``), whose keywords
``resolve_beam_kwargs`` checks.
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


@dataclass(frozen=True)
class GenerateConfig:
    max_length: int = DEFAULT_MAX_LENGTH
    do_sample: bool = False
    temperature: float = DEFAULT_TEMPERATURE
    top_k: int = DEFAULT_TOP_K           # 0: no top-k filter
    top_p: float = DEFAULT_TOP_P         # 1.0: no nucleus filter
    num_return_sequences: int = 1


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


def resolve_generate_kwargs(kwargs: dict, default_max_length: int = DEFAULT_MAX_LENGTH) -> GenerateConfig:
    """Validate ``generate`` keywords and fill in HF's defaults.  ``kwargs`` is not modified.

    ``None`` for temperature / top_k / top_p means "no such warper", as in HF (the warper is only built when the value is
    not None).  With ``do_sample=False`` the sampling keywords are ignored (HF warns and decodes greedily)."""
    kw = dict(kwargs)
    max_length = int(kw.pop("max_length", default_max_length))   # range-checked by the library, as before
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
    if kw:
        raise NotImplementedError(f"unsupported generate kwargs on the MI355X path: {sorted(kw)}")
    if not _is_int(n) or n < 1:
        raise ValueError(f"`num_return_sequences` has to be a strictly positive integer, but is {n!r}")
    if not do_sample:
        if n != 1:   # hf: generation/utils.py (greedy mode) raises the same
            raise ValueError("Greedy methods without beam search do not support `num_return_sequences` different than 1 "
                             f"(got {n}).")
        return GenerateConfig(max_length=max_length)
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
                          top_p=float(top_p), num_return_sequences=operator.index(n))


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
