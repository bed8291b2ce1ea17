"""GPU: the decode loop's look-ahead across a host poll (M2M_POLL_LOOKAHEAD, default 1) against the draining poll (=0).

The look-ahead launches the first graph of the next chunk before the host waits for a poll's snapshot; the poll schedule and every
decision (stop, re-pack, which rows move) stay functions of the step count and the snapshot at the poll, so ids, output lengths and
repack_stats() must be IDENTICAL between the two settings - every comparison below is torch.equal.  The switch is read once per
decode call, so both legs run on one model.  Polls come after 16, 32, 64, 96, 128 steps, then every 64; a graph is 8 steps.
(The loop leaves the look-ahead out where two chains stream the same cross-K/V layers non-temporally, decode.hip
decode_chains_may_drift.  No case here does: 32 clips x (61 + 400) positions in bf16 are 181e6 bytes of K/V per step, below that
route's 200e6, and where a session that has grown to 400 positions takes the route with 24 clips x S = 8 in fp32, a layer of cross
K/V is 0.8 MB and all six stay resident - so the two legs differ in every case.  tests/test_kv_resident_stagger_gpu.py runs
sessions that stream.)"""
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

pytestmark = pytest.mark.gpu

GEOM = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
LEG_ENV = ("M2M_POLL_LOOKAHEAD", "M2M_COMPACT", "M2M_NO_GRAPH", "M2M_GRAPH_STEPS", "M2M_GROUP_ROWS")


def state_dict(eos_scale=None):
    sd = synth.t5_state_dict(GEOM, seed=0)
    synth.perturb_layer_norms(sd, 0)
    if eos_scale is not None:
        synth.force_eos_head(sd, GEOM, active=340, eos_scale=eos_scale)
    return sd


def model_of(sd, precision):
    m = T5Transformer(DEFAULT_CONFIG, precision=precision)
    load_t5_state(m, sd, strict=False)
    return m.cuda().eval()


def embeds(B, S, seed):
    return torch.from_numpy(synth.normal(seed, "embeds", (B, S, GEOM.d_model), 3.0))


def oracle_ids(sd, x, L):
    from oracle.t5 import T5Oracle
    return T5Oracle(GEOM, sd).generate(x, L)


def leg(monkeypatch, **env):
    for k in LEG_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def last_eos_column(ids):
    """per row the column of its EOS (-1: none)"""
    hit = ids == GEOM.eos_token_id
    return [int(hit[r].float().argmax()) if bool(hit[r].any()) else -1 for r in range(ids.shape[0])]


# ------------------------------------------------------------------ 1. no row ends: the schedule alone ---
@pytest.fixture(scope="module")
def plain():
    sd = state_dict()
    x3 = embeds(3, 8, 7)
    return {"sd": sd, "fp32": model_of(sd, "fp32"), "bf16": model_of(sd, "bf16"), "x3": x3, "want3": oracle_ids(sd, x3, 130)}


@pytest.mark.parametrize("max_length", [2, 8, 9, 10, 17, 18, 25, 33, 34, 130])
@pytest.mark.parametrize("B", [3, 24])
def test_no_eos_every_schedule_edge(monkeypatch, plain, B, max_length):
    """steps = max_length - 1: 1; 7; 8 (exactly one graph); 9; 16 (the end coincides with the first poll); 17 (a look-ahead mostly past
    the end); 24; 32; 33; 129 (into the 64-step chunks).  One chain of 3 clips in fp32 (also the oracle's ids: without EOS the ids of
    a shorter call are a prefix of the longest one's), two chains of 12 in bf16."""
    m = plain["fp32" if B == 3 else "bf16"]
    x = plain["x3"] if B == 3 else embeds(B, 8, 8)
    out = {}
    for la in ("1", "0"):
        leg(monkeypatch, M2M_POLL_LOOKAHEAD=la)
        out[la] = m.generate_from_embeds(x.cuda(), max_length=max_length).cpu()
    assert out["1"].shape == (B, max_length)
    assert torch.equal(out["1"], out["0"])
    if B == 3:
        assert torch.equal(out["1"], plain["want3"][:, :max_length])


# ------------------------------------------------------------------ 2. rows that end ---
@pytest.fixture(scope="module")
def ragged():
    sd = state_dict(1.6)
    x9 = embeds(9, 61, 21)
    return {"sd": sd, "fp32": model_of(sd, "fp32"), "bf16": model_of(sd, "bf16"), "x9": x9, "want9": oracle_ids(sd, x9, 400)}


@pytest.mark.parametrize("precision,B", [("fp32", 9), ("bf16", 32)])
def test_rows_that_end_four_legs(monkeypatch, ragged, precision, B):
    """look-ahead on / off x re-packing on / off: ids and output length equal across the four legs, repack_stats() equal between
    look-ahead on and off (with re-packing: it really happens), fp32 equal to the oracle; then a batch without EOS on the same
    session equals a fresh model's."""
    m = ragged[precision]
    x = ragged["x9"] if B == 9 else embeds(B, 61, 21)
    out, stats = {}, {}
    for compact in ("1", "0"):
        for la in ("1", "0"):
            leg(monkeypatch, M2M_POLL_LOOKAHEAD=la, M2M_COMPACT=compact)
            out[la, compact] = m.generate_from_embeds(x.cuda(), max_length=400).cpu()
            stats[la, compact] = m.repack_stats()
    print(f"rows that end {precision} B={B}: output length {out['1', '1'].shape[1]}, re-packings {stats['1', '1']}")
    for k, v in out.items():
        assert v.shape == out["0", "0"].shape and torch.equal(v, out["0", "0"]), k
    assert stats["1", "1"] == stats["0", "1"] and stats["1", "0"] == stats["0", "0"] == (0, 0)
    assert stats["1", "1"][0] >= 1 and stats["1", "1"][1] >= 1
    ends = last_eos_column(out["1", "1"])
    assert len(set(ends)) > 2                                   # rows end at different steps
    if precision == "fp32":
        assert torch.equal(out["1", "1"], ragged["want9"])
    sd2 = state_dict()
    want = model_of(sd2, precision).generate_from_embeds(x.cuda(), max_length=96).cpu()
    leg(monkeypatch)
    load_t5_state(m, sd2, strict=False)
    try:
        got = m.generate_from_embeds(x.cuda(), max_length=96).cpu()
    finally:
        load_t5_state(m, ragged["sd"], strict=False)             # the module's model goes on with the EOS head
    assert torch.equal(got, want)


# Two batches of 4 clips (S = 8), chosen with the fp32 CPU oracle: (eos_scale, embeds seed, the window of the LAST row's EOS column).
#  - 1 .. 15: every row has ended when the first poll (16 steps) reads its snapshot: the call stops with a look-ahead in flight;
#  - 17 .. 24: two of the four rows have ended at that poll, so it wants a re-packing (max_length 130: >= 64 steps remain), and the
#    other two end INSIDE the look-ahead (steps 16 .. 24): the rows move between chains that have already ended.
@pytest.mark.parametrize("eos_scale,seed,lo,hi", [(2.5, 19, 1, 15), (2.0, 30, 17, 24)])
def test_last_eos_around_the_first_poll(monkeypatch, eos_scale, seed, lo, hi):
    sd = state_dict(eos_scale)
    m = model_of(sd, "fp32")
    x = embeds(4, 8, seed)
    out, stats = {}, {}
    for compact in ("1", "0"):
        for la in ("1", "0"):
            leg(monkeypatch, M2M_POLL_LOOKAHEAD=la, M2M_COMPACT=compact)
            out[la, compact] = m.generate_from_embeds(x.cuda(), max_length=130).cpu()
            stats[la, compact] = m.repack_stats()
    ends = last_eos_column(out["0", "0"])
    print(f"eos_scale {eos_scale} seed {seed}: EOS columns {ends}, re-packings {stats['1', '1']}")
    assert min(ends) >= 1 and lo <= max(ends) <= hi, ends       # the fixture still exercises what it was chosen for
    if lo > 16:
        assert sum(1 for e in ends if e < 16) * 4 >= len(ends)  # ... a quarter of the rows ended before the first poll
    for k, v in out.items():
        assert v.shape == out["0", "0"].shape and torch.equal(v, out["0", "0"]), k
    assert stats["1", "1"] == stats["0", "1"] and stats["1", "0"] == stats["0", "0"] == (0, 0)
    assert torch.equal(out["1", "1"], oracle_ids(sd, x, 130))


# ------------------------------------------------------------------ 3. launch modes ---
@pytest.mark.parametrize("mode", [{"M2M_NO_GRAPH": 1}, {"M2M_GRAPH_STEPS": 3}, {"M2M_GRAPH_STEPS": 64}, {"M2M_GROUP_ROWS": 8},
                                  {"M2M_NO_GRAPH": 1, "M2M_GRAPH_STEPS": 64}], ids=str)
def test_launch_modes(monkeypatch, ragged, mode):
    """direct launches (the look-ahead is then 8 direct steps; with M2M_GRAPH_STEPS=64 it is capped by the coming chunk), graphs that
    do not divide a chunk (3) or exceed it (64), two chains of 8 + 1 clips: same ids, same re-packings"""
    m, x = ragged["fp32"], ragged["x9"]
    out, stats = {}, {}
    for la in ("1", "0"):
        leg(monkeypatch, M2M_POLL_LOOKAHEAD=la, **mode)
        out[la] = m.generate_from_embeds(x.cuda(), max_length=400).cpu()
        stats[la] = m.repack_stats()
    print(f"{mode}: re-packings {stats['1']}")
    assert torch.equal(out["1"], out["0"]) and torch.equal(out["1"], ragged["want9"])
    assert stats["1"] == stats["0"] and stats["1"][0] >= 1


# ------------------------------------------------------------------ 4. the other head forms run the same loop ---
def _both(monkeypatch, call):
    res = []
    for la in ("1", "0"):
        leg(monkeypatch, M2M_POLL_LOOKAHEAD=la)
        res.append(call())
    return res


def test_sampled_with_a_fixed_seed(monkeypatch, ragged):
    m, x = ragged["fp32"], embeds(24, 8, 5)

    def call():
        torch.manual_seed(11)
        ids = m.generate_from_embeds(x.cuda(), max_length=140, do_sample=True, temperature=1.5, top_k=40, top_p=0.95).cpu()
        return ids, m.repack_stats()
    (a, sa), (b, sb) = _both(monkeypatch, call)
    assert a.shape == b.shape and torch.equal(a, b) and sa == sb


def test_processed(monkeypatch, ragged):
    m, x = ragged["fp32"], embeds(24, 8, 5)

    def call():
        return m.generate_from_embeds(x.cuda(), max_length=140, repetition_penalty=1.3).cpu(), m.repack_stats()
    (a, sa), (b, sb) = _both(monkeypatch, call)
    assert a.shape == b.shape and torch.equal(a, b) and sa == sb


def test_scored(monkeypatch, ragged):
    m, x = ragged["fp32"], embeds(24, 8, 5)

    def call():
        out = m.generate_from_embeds(x.cuda(), max_length=140, return_dict_in_generate=True, output_scores=True, output_logprobs=True)
        return out.sequences.cpu(), torch.stack(out.scores).cpu(), out.logprobs.cpu(), m.repack_stats()
    (ia, sa, la, ra), (ib, sb, lb, rb) = _both(monkeypatch, call)
    assert ia.shape == ib.shape and torch.equal(ia, ib) and ra == rb
    assert torch.equal(sa, sb) and torch.equal(la, lb)           # the zeros of finished rows included
    done = (ia[:, 1:] == GEOM.eos_token_id).cumsum(1) > 0
    after = torch.cat([torch.zeros_like(done[:, :1]), done[:, :-1]], dim=1)
    assert bool(after.any()) and bool((la[after] == 0).all()) and bool((sa.permute(1, 0, 2)[after] == 0).all())


def test_beam(monkeypatch, ragged):
    m, x = ragged["fp32"], embeds(12, 8, 5)                      # 12 clips x 2 beams: two chains of 12 rows

    def call():
        seq, sc = m.beam_search_from_embeds(x.cuda(), num_beams=2, max_length=60, return_scores=True)
        return seq.cpu(), sc.cpu()
    (a, sa), (b, sb) = _both(monkeypatch, call)
    assert a.shape == b.shape and torch.equal(a, b) and torch.equal(sa, sb)
