"""``beam_ref.beam_search`` (transformers 4.34 ``_beam_search`` for an encoder-decoder) restated with one hook: a non-empty
``logits_processor``.  hf: generation/utils.py ``_beam_search``:

    next_token_scores = log_softmax(logits)
    next_token_scores_processed = logits_processor(input_ids, next_token_scores)
    next_token_scores = next_token_scores_processed + beam_scores[:, None]

The hook is ``grammar_ref.process(ids_rows, logp, pc, eos, max_length, grammar)`` - the processors of ``process_ref`` in
``_get_logits_processor``'s order with the MIDI token grammar's mask at ``PrefixConstrainedLogitsProcessor``'s place - applied to
every row against its own beam's prefix.  Everything after the top 2 nb (``BeamSearchScorer.process``, ``is_done``, ``finalize``) is
``beam_ref``'s: its ``_Hyps``, ``pick_best`` and ``oracle_step`` are imported, not copied.

New with masks: a clip can have fewer than nb finite non-EOS candidates.  The stable descending sort puts the ``-inf`` candidates
behind every finite one, in flat (beam-major) order; such a beam carries ``-inf`` from there on.  The decision-gap bookkeeping
skips a pair that is ``-inf`` on both sides (``inf - inf`` is NaN: there is no decision between them, the flat index decides); a
finite value against ``-inf`` is an infinite gap.
"""
from __future__ import annotations

import math

import torch

import grammar_ref as gref
from beam_ref import _Hyps, oracle_step, pick_best


def beam_search(step, B: int, nb: int, V: int, max_length: int, length_penalty: float = 1.0, early_stopping=False,
                num_return_sequences: int = 1, eos: int = 1, pad: int = 0, start: int = 0, pc=None, grammar=None, hook=None):
    """-> (ids LongTensor [B * n, W], sequences_scores float32 [B * n], min_gap float).  ``hook(ids_rows, logp) -> logp``
    replaces the default ``grammar_ref.process`` with ``pc`` and ``grammar`` (both None: the neutral hook)."""
    if hook is None:
        def hook(ids_rows, logp):
            return gref.process(ids_rows, logp, pc, eos, max_length, grammar)
    gaps = []
    n = num_return_sequences
    hyps = [_Hyps(nb, length_penalty, early_stopping, max_length, gaps) for _ in range(B)]
    done = [False] * B
    ids = torch.full((B * nb, 1), start, dtype=torch.long)
    beam_scores = torch.zeros(B, nb, dtype=torch.float32)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    beam_idx = None
    t = 0
    while ids.shape[1] < max_length:
        logits = step(ids[:, -1], t, beam_idx).float()
        logp = hook(ids, torch.log_softmax(logits, dim=-1))
        scores = logp + beam_scores[:, None]
        flat = scores.view(B, nb * V)
        vals, order = torch.sort(flat, dim=1, descending=True, stable=True)
        K = 2 * nb
        for b in range(B):
            if done[b]:
                continue
            d = (vals[b, : K + 1][:-1] - vals[b, : K + 1][1:]).abs()      # NaN for a pair at -inf: not > 0, skipped
            gaps.extend(float(x) for x in d if x > 0)
        top_s, top_i = vals[:, :K], order[:, :K]
        cur_len = ids.shape[1]
        nxt_scores = torch.zeros(B, nb, dtype=torch.float32)
        nxt_tokens = torch.full((B, nb), pad, dtype=torch.long)
        nxt_idx = torch.zeros(B, nb, dtype=torch.long)
        for b in range(B):
            if done[b]:
                nxt_idx[b] = b * nb
                continue
            bi = 0
            for rank in range(K):
                tok = int(top_i[b, rank]) % V
                beam = int(top_i[b, rank]) // V
                row = b * nb + beam
                sc = float(top_s[b, rank])
                if tok == eos:
                    if rank >= nb:
                        continue
                    hyps[b].add(ids[row].tolist(), sc)
                else:
                    nxt_scores[b, bi], nxt_tokens[b, bi], nxt_idx[b, bi] = top_s[b, rank], tok, row
                    bi += 1
                if bi == nb:
                    break
            assert bi == nb
            done[b] = done[b] or hyps[b].is_done(float(top_s[b].max()), cur_len)
        beam_scores = nxt_scores.view(-1)
        beam_idx = nxt_idx.view(-1)
        ids = torch.cat([ids[beam_idx], nxt_tokens.view(-1, 1)], dim=1)
        t += 1
        if all(done):
            break
    for b in range(B):
        if done[b]:
            continue
        for i in range(nb):
            hyps[b].add(ids[b * nb + i].tolist(), float(beam_scores[b * nb + i]))
    best, best_scores = [], []
    for b in range(B):
        for s, h in pick_best(hyps[b].beams, n, gaps):
            best.append(h)
            best_scores.append(s)
    lens = [len(h) for h in best]
    W = min(max(lens) + 1, max_length)
    out = torch.full((B * n, W), pad, dtype=torch.long)
    for i, h in enumerate(best):
        out[i, : len(h)] = torch.tensor(h, dtype=torch.long)
        if len(h) < W:
            out[i, len(h)] = eos
    gaps = [x for x in gaps if x == x]                                   # the imported bookkeeping's inf - inf pairs
    return out, torch.tensor(best_scores, dtype=torch.float32), (min(gaps) if gaps else math.inf)


@torch.no_grad()
def oracle_beam_search(orc, inputs_embeds: torch.Tensor, num_beams: int, max_length: int, length_penalty=1.0, early_stopping=False,
                       num_return_sequences=1, pc=None, grammar=None):
    g = orc.g
    enc = orc.encode(inputs_embeds)
    step = oracle_step(orc, enc, num_beams, max_length)
    return beam_search(step, inputs_embeds.shape[0], num_beams, g.vocab_size, max_length, length_penalty, early_stopping,
                       num_return_sequences, eos=g.eos_token_id, pad=g.pad_token_id, start=g.decoder_start_token_id, pc=pc,
                       grammar=grammar)
