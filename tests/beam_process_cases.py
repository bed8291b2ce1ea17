"""The case table of tests/test_beam_process_gpu.py and the helpers both beam-process test files share (no GPU needed to import).

A case: (name, eos head, B, S, nb, n, length_penalty, early_stopping, max_length, input seed, midi_grammar, processor keywords).
The seeds were chosen on the CPU so that the restatement alone (tests/beam_process_ref.py on the fp32 oracle) meets
test_beam_gpu's decision-gap condition, > 1e-4; the recorded gaps are in the trailing comments.  early_stopping in {False, True,
"never"} and length_penalty in {0, 1, 2} are spread over the cases, not crossed.  EOS is id 2 (the tokenizer's), ONSET 3, the
pitch ids 5 .. 132, the time ids 133 .. 332.
"""
from __future__ import annotations

import copy

import torch

from music2midi_amd import synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.generation import resolve_beam_process_kwargs
from music2midi_amd.grammar import EOS, MidiGrammar

# forced_bos_token_id = ONSET: an id the grammar bans at the start (only a time id or EOS may open a sequence) - the forced id wins
# and the state takes the total transition (-> ONSET_OPEN: pitches).  begin_suppress_tokens then act at cur_len 2 on pitch ids.
ALL_KW = dict(min_length=12, forced_eos_token_id=EOS, suppress_tokens=[9, 140, 141, 250], begin_suppress_tokens=[5, 6, 7, 64, 65],
              bad_words_ids=[[66]], forced_bos_token_id=3)
PLAIN_KW = dict(min_length=6, min_new_tokens=8, forced_eos_token_id=EOS, suppress_tokens=[4, 9], begin_suppress_tokens=[6, 7],
                bad_words_ids=[[5]])

FP32_CASES = [
    ("grammar-1x2", False, 1, 19, 2, 1, 1.0, False, 24, 7, True, {}),              # gap 1.2e-1
    ("grammar-3x4", True, 3, 30, 4, 4, 0.0, True, 40, 8, True, {}),                # gap 4.1e-2; every row ends with an EOS of its own
    ("grammar-2x32", False, 2, 30, 32, 2, 2.0, "never", 24, 57, True, {}),         # gap 1.9e-4; nb = 32: every wave's second beam
    ("grammar-all", False, 3, 30, 8, 8, 1.0, False, 32, 10, True, ALL_KW),         # gap 6.6e-4
    ("processors", True, 3, 30, 4, 2, 2.0, "never", 24, 9, False, PLAIN_KW),       # gap 3.0e-4
    # ONSET suppressed: after its first time id a row is in phase TIME with nothing sounding, the grammar allows ONSET alone and
    # EVERY candidate of the clip is at -inf from the second step on - the beams, the EOS candidates of rank < nb and the
    # hypotheses they become are all ranked by the flat index alone, and the returned scores are -inf
    ("minus-inf", False, 2, 19, 4, 4, 1.0, False, 12, 8, True, dict(suppress_tokens=[3])),       # gap 9.4e-2; 6 of 8 scores -inf
]

# V / (special, pitch, time): test_grammar_gpu.test_vocabulary_bands_fp32's shapes (NPL = 8, 32, 64)
BAND_CASES = [(400, (5, 128, 200), 14), (2048, (5, 100, 1900), 14), (4096, (7, 128, 3900), 14)]     # (V, sizes, input seed): gaps 9.3e-4, 7.6e-4, 4.8e-4
BAND_SHAPE = dict(B=2, S=19, nb=4, n=2, L=16)


def tiny_config():
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    return cfg


def band_config(V, sizes):
    cfg = tiny_config()
    cfg["model"]["t5"]["vocab_size"] = V
    cfg["tokenizer"]["vocab_size"] = dict(special=sizes[0], pitch=sizes[1], time=sizes[2])
    return cfg


def grammar_of(cfg_dict) -> MidiGrammar:
    return MidiGrammar.from_vocab(load_config(cfg_dict).tokenizer.vocab_size)


def oracle(cfg_dict, precision="fp32", eos=False, seed=0):
    """(T5Oracle, geometry) with the weights test_t5_gpu.build loads into the model under test"""
    from oracle.t5 import T5Oracle
    geom = T5Geometry(load_config(cfg_dict).model.t5)
    sd = synth.t5_state_dict(geom, seed=seed)
    synth.perturb_layer_norms(sd, seed)
    if eos:
        synth.force_eos_head(sd, geom)
    return T5Oracle(geom, sd, emulate=precision), geom


def embeds(B, S, d, seed=7):
    return torch.from_numpy(synth.normal(seed, "embeds", (B, S, d), 3.0))


def process_config(kw, V=400):
    return resolve_beam_process_kwargs(dict(kw), V, None)[0] if kw else None


def walks_inside(grammar: MidiGrammar, row) -> bool:
    """every id after the start token, up to and including the first EOS, is in allowed(state) - walked with MidiGrammar.step"""
    state = grammar.start()
    for tok in [int(v) for v in row][1:]:
        if tok not in grammar.allowed(state):
            return False
        if tok == EOS:
            return True
        state = grammar.step(state, tok)
    return True
