"""The processed oracle decode (tests/process_ref.py) with the MIDI token grammar's mask where transformers 4.34 puts
``PrefixConstrainedLogitsProcessor`` in ``_get_logits_processor``: after ``MinNewTokensLengthLogitsProcessor``, before
``ForcedBOSTokenLogitsProcessor``.  Its arithmetic is HF's: ``scores + mask`` with the mask ``-inf`` outside the allowed ids of the
row's prefix and 0 inside.  ``grammar=None`` is ``process_ref.process``."""
from __future__ import annotations

import torch

from music2midi_amd.generation import ProcessConfig

import process_ref as pr

NEG = pr.NEG
_HEAD = ("repetition_penalty", "no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens")


def _split(pc: ProcessConfig):
    """(the processors before the grammar's place, those after it) as two ProcessConfigs"""
    d = {k: getattr(pc, k) for k in ProcessConfig.__dataclass_fields__}
    head = ProcessConfig(**{k: v for k, v in d.items() if k in _HEAD})
    tail = ProcessConfig(**{k: v for k, v in d.items() if k not in _HEAD})
    return head, tail


def grammar_mask(input_ids: torch.Tensor, vocab_size: int, grammar) -> torch.Tensor:
    """[B, V] float: 0 at the ids ``grammar`` allows after each row of ``input_ids`` (the start token first), -inf elsewhere"""
    mask = torch.full((input_ids.shape[0], vocab_size), NEG)
    for b, row in enumerate(input_ids.tolist()):
        mask[b, grammar.allowed(grammar.state_of(row))] = 0
    return mask


def process(input_ids: torch.Tensor, scores: torch.Tensor, pc, eos: int, max_length: int, grammar=None) -> torch.Tensor:
    pc = pc if pc is not None else ProcessConfig()
    if grammar is None:
        return pr.process(input_ids, scores, pc, eos, max_length)
    head, tail = _split(pc)
    s = pr.process(input_ids, scores, head, eos, max_length)
    s = s + grammar_mask(input_ids, s.shape[-1], grammar)
    return pr.process(input_ids, s, tail, eos, max_length)     # begin_index depends on forced_bos_token_id alone: it is in `tail`


@torch.no_grad()
def oracle_generate(orc, inputs_embeds: torch.Tensor, max_length: int, pc, grammar, return_margins: bool = False):
    """HF greedy_search on ``T5Oracle`` with the processors and the grammar: ``process_ref.oracle_generate`` with ``process`` above."""
    g = orc.g
    enc = orc.encode(inputs_embeds)
    B = enc.shape[0]
    cross = orc._cross_kv(enc)
    cache = orc._new_cache(B, max_length)
    bias_tab = orc._dec_bias_table(max_length)
    ids = torch.full((B, 1), g.decoder_start_token_id, dtype=torch.long)
    unfinished = torch.ones(B, dtype=torch.long)
    margins = []
    t = 0
    while ids.shape[1] < max_length:
        logits = orc.decode_step(ids[:, -1], t, cache, cross, bias_tab)
        s = process(ids, logits, pc, g.eos_token_id, max_length, grammar)
        nxt = torch.argmax(s, dim=-1)
        if return_margins:
            top2 = torch.topk(s, 2, dim=-1).values
            margins.append(top2[:, 0] - top2[:, 1])
        nxt = nxt * unfinished + g.pad_token_id * (1 - unfinished)
        ids = torch.cat([ids, nxt[:, None]], dim=1)
        unfinished = unfinished & (nxt != g.eos_token_id).long()
        t += 1
        if unfinished.max() == 0:
            break
    if return_margins:
        return ids, (torch.stack(margins, 1) if margins else torch.zeros(B, 0))
    return ids
