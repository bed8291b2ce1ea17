"""transformers 4.34 logits processors (generation/logits_process.py), restated in pure torch for the processed decode tests, in the
order of ``_get_logits_processor`` for an encoder-decoder (generation/utils.py): repetition penalty, no-repeat n-gram, bad words,
min length, min new tokens, forced BOS, forced EOS, suppress, begin-suppress.  ``input_ids`` are the decoder ids so far (the start
token first), so cur_len = input_ids.shape[1].  ``oracle_generate`` runs the greedy / sampling loop of HF on ``T5Oracle``."""
from __future__ import annotations

import torch

from music2midi_amd.generation import ProcessConfig

NEG = -float("inf")


def repetition_penalty(input_ids, scores, penalty):
    score = torch.gather(scores, 1, input_ids)
    score = torch.where(score < 0, score * penalty, score / penalty)
    return scores.scatter(1, input_ids, score)


def no_repeat_ngram(input_ids, scores, n):
    scores = scores.clone()
    cur = input_ids.shape[1]
    if cur + 1 < n:
        return scores
    for b in range(input_ids.shape[0]):
        h = input_ids[b].tolist()
        prefix = h[cur - n + 1:] if n > 1 else []
        for i in range(cur - n + 1):
            if h[i:i + n - 1] == prefix:
                scores[b, h[i + n - 1]] = NEG
    return scores


def bad_words(input_ids, scores, bad_words_ids, eos):
    scores = scores.clone()
    cur = input_ids.shape[1]
    for seq in [list(s) for s in bad_words_ids if list(s) != [eos]]:
        if len(seq) == 1:
            scores[:, seq[0]] = NEG
            continue
        if len(seq) > cur:
            continue
        hit = (input_ids[:, cur - len(seq) + 1:] == torch.tensor(seq[:-1])).all(1)
        scores[hit, seq[-1]] = NEG
    return scores


def process(input_ids: torch.Tensor, scores: torch.Tensor, pc: ProcessConfig, eos: int, max_length: int) -> torch.Tensor:
    cur = input_ids.shape[1]
    s = scores.float().clone()
    if pc.repetition_penalty != 1.0:
        s = repetition_penalty(input_ids, s, pc.repetition_penalty)
    if pc.no_repeat_ngram_size > 0:
        s = no_repeat_ngram(input_ids, s, pc.no_repeat_ngram_size)
    if pc.bad_words_ids:
        s = bad_words(input_ids, s, pc.bad_words_ids, eos)
    if pc.min_length > 0 and cur < pc.min_length:
        s[:, eos] = NEG
    if pc.min_new_tokens > 0 and cur - 1 < pc.min_new_tokens:
        s[:, eos] = NEG
    if pc.forced_bos_token_id >= 0 and cur == 1:
        s[:] = NEG
        s[:, pc.forced_bos_token_id] = 0
    if pc.forced_eos_token_id >= 0 and cur == max_length - 1:
        s[:] = NEG
        s[:, pc.forced_eos_token_id] = 0
    if pc.suppress_tokens:
        s[:, list(pc.suppress_tokens)] = NEG
    if pc.begin_suppress_tokens and cur == pc.begin_index:
        s[:, list(pc.begin_suppress_tokens)] = NEG
    return s


@torch.no_grad()
def oracle_generate(orc, inputs_embeds: torch.Tensor, max_length: int, pc: ProcessConfig, return_margins: bool = False):
    """HF greedy_search with the processors: arg-max of the processed scores; finished rows emit pad; stops when every row has
    emitted EOS.  ``return_margins``: also the processed top-2 margin of every step [B, L - 1]."""
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
        s = process(ids, logits, pc, g.eos_token_id, max_length)
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
