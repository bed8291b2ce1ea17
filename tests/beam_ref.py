"""Beam search as transformers 4.34 runs it for an encoder-decoder, restated on a step function (pure torch, CPU).

hf: generation/utils.py ``_beam_search`` and generation/beam_search.py ``BeamSearchScorer.process / finalize`` and
``BeamHypotheses.add / is_done``.  The running beam scores are fp32 tensors; hypothesis scores are Python floats (double), as in
HF.  The top 2 nb candidates are taken by a stable descending sort, so exact ties go to the lower flat (beam-major) index.
Besides the ids and ``sequences_scores`` the restatement reports the smallest decision gap it met: the smallest non-zero
difference between two scores it compared (adjacent candidates around the top-2 nb boundary and inside it, a new hypothesis
against the worst kept one, ``is_done``, the final picks).  A device run in other arithmetic can only take another decision
where that gap is of the size of its rounding error.

``step(tokens [R], t, beam_idx [R] or None) -> logits [R, V]`` feeds position t of every row; ``beam_idx`` (from the second step
on) tells the step function which row each row continues, so it can reorder its caches first (HF's ``_reorder_cache``).
"""
from __future__ import annotations

import math
from typing import Callable, Optional

import torch

from oracle.t5 import T5Oracle


class _Hyps:
    """BeamHypotheses (4.34): a list in insertion order, at most nb entries."""

    def __init__(self, nb, lp, early, max_length, gaps):
        self.nb, self.lp, self.early, self.max_length = nb, lp, early, max_length
        self.beams = []          # (score, tokens)
        self.worst = 1e9
        self.gaps = gaps

    def add(self, hyp, sum_logprobs):
        score = sum_logprobs / (len(hyp) ** self.lp)
        if len(self.beams) >= self.nb:
            self.gaps.append(abs(score - self.worst))
        if len(self.beams) < self.nb or score > self.worst:
            self.beams.append((score, list(hyp)))
            if len(self.beams) > self.nb:
                srt = sorted([(s, i) for i, (s, _) in enumerate(self.beams)])
                del self.beams[srt[0][1]]
                self.worst = srt[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self.beams) < self.nb:
            return False
        if self.early is True:
            return True
        length = self.max_length if (self.early == "never" and self.lp > 0.0) else cur_len
        bound = best_sum_logprobs / length ** self.lp
        self.gaps.append(abs(self.worst - bound))
        return self.worst >= bound


def pick_best(beams, n, gaps=None):
    """BeamSearchScorer.finalize's choice: ``sorted(beams, key=score)`` then n x ``pop()`` - the best first, and among equal
    scores the one added later first (the sort is stable)."""
    srt = sorted(beams, key=lambda x: x[0])
    if gaps is not None and len(srt) > n:
        gaps.extend(abs(srt[-j - 1][0] - srt[-j - 2][0]) for j in range(n) if srt[-j - 1][0] != srt[-j - 2][0])
    return [srt.pop() for _ in range(n)]


def beam_search(step: Callable, B: int, nb: int, V: int, max_length: int, length_penalty: float = 1.0,
                early_stopping=False, num_return_sequences: int = 1, eos: int = 1, pad: int = 0, start: int = 0):
    """-> (ids LongTensor [B * n, W], sequences_scores float32 [B * n], min_gap float)."""
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
        scores = torch.log_softmax(logits, dim=-1) + beam_scores[:, None]
        flat = scores.view(B, nb * V)
        vals, order = torch.sort(flat, dim=1, descending=True, stable=True)
        K = 2 * nb
        for b in range(B):
            if done[b]:
                continue
            d = (vals[b, : K + 1][:-1] - vals[b, : K + 1][1:]).abs()
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
    # finalize
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
    return out, torch.tensor(best_scores, dtype=torch.float32), (min(gaps) if gaps else math.inf)


def oracle_step(orc: T5Oracle, enc_out: torch.Tensor, nb: int, max_length: int):
    """A step function over ``T5Oracle``: the clip's cross K/V repeated for its beams, self caches reordered by index_select."""
    cross = [(k.repeat_interleave(nb, 0), v.repeat_interleave(nb, 0)) for k, v in orc._cross_kv(enc_out)]
    state = {"cache": orc._new_cache(enc_out.shape[0] * nb, max_length)}
    bias_tab = orc._dec_bias_table(max_length)

    def step(tokens, t, beam_idx: Optional[torch.Tensor]):
        if beam_idx is not None:
            state["cache"] = [(k.index_select(0, beam_idx), v.index_select(0, beam_idx)) for k, v in state["cache"]]
        return orc.decode_step(tokens, t, state["cache"], cross, bias_tab)

    return step


@torch.no_grad()
def oracle_beam_search(orc: T5Oracle, inputs_embeds: torch.Tensor, num_beams: int, max_length: int, length_penalty=1.0,
                       early_stopping=False, num_return_sequences=1):
    g = orc.g
    enc = orc.encode(inputs_embeds)
    step = oracle_step(orc, enc, num_beams, max_length)
    return beam_search(step, inputs_embeds.shape[0], num_beams, g.vocab_size, max_length, length_penalty, early_stopping,
                       num_return_sequences, eos=g.eos_token_id, pad=g.pad_token_id, start=g.decoder_start_token_id)
