"""GPU: the consensus selection on the device (scoring.pairwise_note_counts / consensus_choice, csrc/consensus.hip) against its
definition on the host (music2midi_amd.consensus): the integers with ``==``, the utilities bit for bit - on generated and hand-made
clips at every shape the kernel treats differently, on a dirty workspace and a side stream - then ``generate_consensus`` on the tiny
model and ``Music2MIDI.generate_notes(consensus=K)`` on random-init weights."""
import numpy as np
import pytest
import torch

import consensus_cases as cs
import note_metrics_cases as nc
from music2midi_amd import consensus, native, scoring, synth
from test_t5_gpu import build, embeds, tiny_config

pytestmark = pytest.mark.gpu
TOK = nc.TOK
EMPTY = []


def _generated(seed, B, K):
    return [c for clip in cs.clips(seed, B, K)[1] for c in clip]


def _chain(rng, notes):
    """About 300 notes of one pitch at consecutive onset indices (every sixth index twice), durations 2..16 steps."""
    out = []
    for i in range(notes):
        on = i * 5 // 6
        out.append((on, min(on + int(rng.integers(2, 17)), 266), 60))
    return out


def _groups():
    """name -> (ids [B * K, L] int64, K)."""
    rng = np.random.default_rng(77)
    groups = {}
    groups["B=1 K=2, the asymmetric pair"] = (nc.id_rows([[(0, 40, 60)], [(0, 32, 60)]], 7), 2)
    crafted = [list(nc.CRAFTED["augmenting path"][1]), [(20, 40, 60), (21, 36, 60)]]
    groups["B=3 K=5"] = (nc.id_rows(_generated(31, 2, 5) + crafted + [EMPTY, [(20, 37, 60)], crafted[1]], 6 * 18 + 1), 5)
    special = [[(3, 9, 60), (4, 8, 62)]] + [EMPTY] * 15                                       # one spurious candidate among empty ones
    special += [EMPTY] * 16                                                                   # all empty
    special += [EMPTY if k in (2, 7, 8, 15) else cs.candidate(rng, cs.hidden_label(rng)) for k in range(16)]      # several empty
    edge = cs.hidden_label(rng)
    edge[:, 2] = rng.choice([0, 127, 1, 126], len(edge))                                      # the first and the last pitch
    special += [cs.candidate(rng, edge) for _ in range(16)]
    rows = _generated(32, 5, 16) + special
    groups["B=9 K=16 id_rows"] = (nc.id_rows(rows, 6 * 18 + 1), 16)
    groups["B=9 K=16 tokenised"] = (nc.tokenised(rows, 64), 16)
    groups["L=1"] = (np.array([[2], [0], [140], [5], [3], [1]], dtype=np.int64), 3)
    groups["L=7"] = (nc.id_rows([[(1, 4, 60)], [(2, 4, 60)], [(2, 5, 60)], EMPTY, [(9, 12, 0)], [(9, 13, 127)], [(9, 13, 127)], [(8, 13, 127)]], 7), 4)
    groups["L=2048, chains"] = (nc.id_rows([_chain(rng, n) for n in (300, 297, 290)], 2048), 3)
    return groups


GROUPS = _groups()
SETTINGS = [dict(), dict(offset_ratio=None), dict(onset_tolerance=0.0), dict(onset_tolerance=0.1), dict(offset_ratio=None, onset_tolerance=0.1)]


def _want(ids, K, **kw):
    decoded = TOK.decode(ids)
    B = len(ids) // K
    pairs = [consensus.pairwise_counts(decoded[b * K:(b + 1) * K], **kw) for b in range(B)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@pytest.fixture(scope="module")
def wanted():
    """The definition's (tp, n) of every group under every setting, computed once."""
    return {(name, i): _want(ids, K, **kw) for name, (ids, K) in GROUPS.items() for i, kw in enumerate(SETTINGS)}


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("name", list(GROUPS))
def test_pairwise_counts_and_selection_equal_the_definition(name, wanted):
    ids, K = GROUPS[name]
    ids_dev = torch.from_numpy(ids).cuda()
    B = len(ids) // K
    decoded = scoring.detokenize(TOK, ids_dev).to_numpy()
    assert all(np.array_equal(a, b) for a, b in zip(decoded, TOK.decode(ids)))
    for i, kw in enumerate(SETTINGS):
        tp, n = wanted[name, i]
        got = scoring.pairwise_note_counts(TOK, ids_dev, K, **kw)
        assert got.tp.dtype == np.int64 and got.tp.shape == (B, K, K) and got.n.shape == (B, K)
        assert np.array_equal(got.n, n), (name, kw)
        assert np.array_equal(got.tp, tp), (name, kw, np.argwhere(got.tp != tp)[:8].tolist())
        chosen, utility = scoring.consensus_choice(TOK, ids_dev, K, **kw)
        assert chosen.is_cuda and utility.is_cuda and chosen.dtype == torch.int32 and utility.dtype == torch.float64
        picks = [consensus.select(tp[b], n[b]) for b in range(B)]
        assert chosen.cpu().tolist() == [p[0] for p in picks], (name, kw)
        assert torch.equal(_bits(utility.cpu()), _bits(torch.from_numpy(np.stack([p[1] for p in picks])))), (name, kw)
    print(f"{name}: {B} clips of {K}, n up to {int(n.max())}, tp sum {int(tp.sum())}")


def test_the_hand_made_clips_choose_what_the_definition_says():
    tp, n = scoring.pairwise_note_counts(TOK, torch.from_numpy(GROUPS["B=1 K=2, the asymmetric pair"][0]).cuda(), 2).tp, None
    assert tp.tolist() == [[[1, 0], [1, 1]]]
    ids, K = GROUPS["B=9 K=16 id_rows"]
    chosen, utility = scoring.consensus_choice(TOK, torch.from_numpy(ids).cuda(), K)
    assert int(chosen[5]) == 1 and utility[5].tolist() == [0.0] + [14 / 15] * 15          # the spurious candidate loses to an empty one
    assert int(chosen[6]) == 0 and utility[6].tolist() == [1.0] * 16                      # all silent: the greedy row
    same = nc.id_rows([[(0, 10, 60), (5, 9, 64)]] * 6, 13)
    chosen, utility = scoring.consensus_choice(TOK, torch.from_numpy(same).cuda(), 3)
    assert chosen.tolist() == [0, 0] and utility.tolist() == [[1.0] * 3] * 2              # a tie goes to candidate 0


def _raw(dn, K, workspace, **kw):
    R, L = int(dn.notes.shape[0]), int(dn.notes.shape[1])
    tp = torch.full((R // K, K, K), 99, dtype=torch.int32, device="cuda")
    n = torch.full((R // K, K), 99, dtype=torch.int32, device="cuda")
    native.check(native.load().m2m_consensus_pairwise_counts(
        dn.notes.data_ptr(), dn.counts.data_ptr(), R, L, K, TOK.time_step, kw.get("onset", 0.05), kw.get("ratio", 0.2), 0.05,
        workspace.data_ptr(), workspace.numel() * 8, tp.data_ptr(), n.data_ptr(), native.stream_handle(tp.device)), "pairwise")
    return tp, n


def test_a_dirty_workspace_and_a_side_stream(wanted):
    name = "B=9 K=16 id_rows"
    ids, K = GROUPS[name]
    dn = scoring.detokenize(TOK, torch.from_numpy(ids).cuda())
    need = native.load().m2m_consensus_workspace_bytes(len(ids), ids.shape[1], K)
    assert ids.size % 2 == 0 and need == 28 * ids.size + 16 * 15 * ids.size
    workspace = torch.full((need // 8,), 0x7f7f7f7f7f7f7f7f, dtype=torch.int64, device="cuda")
    first = _raw(dn, K, workspace)
    other = _raw(dn, K, workspace, ratio=-1.0, onset=0.1)                  # leaves other matchings behind
    second = _raw(dn, K, workspace)
    for got in (first, second):
        assert np.array_equal(got[0].cpu().numpy(), wanted[name, 0][0]) and np.array_equal(got[1].cpu().numpy(), wanted[name, 0][1])
    assert np.array_equal(other[0].cpu().numpy(), wanted[name, 4][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ids_dev = torch.from_numpy(ids).cuda()
        got = scoring.pairwise_note_counts(TOK, ids_dev, K)
        chosen, utility = scoring.consensus_choice(TOK, ids_dev, K)
    side.synchronize()
    assert np.array_equal(got.tp, wanted[name, 0][0]) and np.array_equal(got.n, wanted[name, 0][1])
    assert chosen.cpu().tolist() == [consensus.select(t, m)[0] for t, m in zip(*wanted[name, 0])]


def test_a_row_with_an_id_outside_the_vocabulary():
    ids = GROUPS["B=3 K=5"][0].copy()
    ids[7, 3] = TOK.model_vocab_size                                         # clip 1, candidate 2
    ids_dev = torch.from_numpy(ids).cuda()
    with pytest.raises(ValueError, match="token row 7 holds an id outside"):
        scoring.pairwise_note_counts(TOK, ids_dev, 5)
    chosen, utility = scoring.consensus_choice(TOK, ids_dev, 5)
    good_c, good_u = scoring.consensus_choice(TOK, torch.from_numpy(GROUPS["B=3 K=5"][0]).cuda(), 5)
    assert int(chosen[1]) == -1 and not utility[1].any()
    assert chosen[[0, 2]].tolist() == good_c[[0, 2]].tolist() and torch.equal(utility[[0, 2]], good_u[[0, 2]])
    none = scoring.pairwise_note_counts(TOK, torch.zeros((0, 5), dtype=torch.long).cuda(), 4)
    assert none.tp.shape == (0, 4, 4) and none.n.shape == (0, 4)


# ------------------------------------------------------------------------------------------------ generate_consensus
@pytest.mark.parametrize("K", [2, 4])
def test_generate_consensus_on_the_tiny_model(K):
    model, _, g = build(tiny_config(), "fp32")
    B, L = 3, 48
    x = embeds(B, 21, g.d_model).cuda()
    greedy = model.generate_from_embeds(x, max_length=L, midi_grammar=True)
    torch.manual_seed(11)
    out = model.generate_consensus_from_embeds(x, K, max_length=L, midi_grammar=True, return_candidates=True)
    W = int(out.candidates.shape[2])
    assert tuple(out.candidates.shape) == (B, K, W) and tuple(out.sequences.shape) == (B, W) and W >= int(greedy.shape[1])
    assert out.sequences.is_cuda and out.chosen.is_cuda and out.utility.is_cuda
    padded = torch.nn.functional.pad(greedy, (0, W - int(greedy.shape[1])), value=g.pad_token_id)
    assert torch.equal(out.candidates[:, 0], padded)                          # candidate 0 is the greedy row
    chosen = out.chosen.cpu().tolist()
    for b in range(B):
        assert torch.equal(out.sequences[b], out.candidates[b, chosen[b]])
    rows = out.candidates.reshape(B * K, W).cpu()
    decoded = TOK.decode(rows)
    assert sum(len(d) for d in decoded) > 0                                   # under the grammar the rows decode to notes
    for b in range(B):
        tp, n = consensus.pairwise_counts(decoded[b * K:(b + 1) * K])
        index, u = consensus.select(tp, n)
        assert chosen[b] == index and np.array_equal(out.tp[b].cpu().numpy(), tp) and np.array_equal(out.n[b].cpu().numpy(), n)
        assert torch.equal(_bits(out.utility[b].cpu()), _bits(torch.from_numpy(u)))
    torch.manual_seed(11)
    again = model.generate_consensus_from_embeds(x, K, max_length=L, midi_grammar=True, return_candidates=True)
    assert torch.equal(again.candidates, out.candidates) and torch.equal(again.sequences, out.sequences)
    torch.manual_seed(11)
    assert torch.equal(model.generate_consensus_from_embeds(x, K, max_length=L, midi_grammar=True), out.sequences)
    print(f"K={K}: widths {int(greedy.shape[1])} -> {W}, chosen {chosen}, notes per row {[len(d) for d in decoded]}")


def test_generate_notes_with_consensus():
    from music2midi_amd.model import Music2MIDI
    cfg = tiny_config()
    cfg["inference"]["midi_grammar"] = True                                   # random weights write no valid note otherwise
    torch.manual_seed(5)
    m = Music2MIDI(cfg).cuda().eval()
    seg = m._segment_length()
    audio = synth.waveform(3, 2 * seg, "music")
    duration = m.config.dataset.segment_duration
    calls, returned = [], []
    inner = m.model.generate_consensus

    def spy(inputs, **kw):
        calls.append(kw)
        returned.append(inner(inputs, **kw))
        return returned[-1]
    m.model.generate_consensus = spy
    plain = m.generate_notes(audio_y=audio)
    assert not calls                                                          # neither the keyword nor the config key: as before
    padded, _ = m._padded_segments(None, audio, None)
    assert np.array_equal(plain, TOK.decode(m.sample_token_rows(padded, seg), mode="sequential", duration_per_batch=duration))
    torch.manual_seed(3)
    notes = m.generate_notes(audio_y=audio, consensus=3)
    assert calls == [dict(max_length=1024, num_samples=3, midi_grammar=True)] and tuple(returned[0].shape)[0] == 2
    assert np.array_equal(notes, TOK.decode(returned[0].cpu(), mode="sequential", duration_per_batch=duration)) and len(notes) > 0
    torch.manual_seed(3)
    assert np.array_equal(m.generate_notes(audio_y=audio, consensus=3), notes)
    cfg["inference"]["consensus_samples"] = 3
    configured = Music2MIDI(cfg).cuda().eval()
    configured.load_state_dict(m.state_dict())
    torch.manual_seed(3)
    assert np.array_equal(configured.generate_notes(audio_y=audio), notes)    # the config key routes the same way
    assert np.array_equal(configured.generate_notes(audio_y=audio, consensus=1), plain)
    print(f"generate_notes: {len(plain)} notes greedy, {len(notes)} by consensus of 3")
