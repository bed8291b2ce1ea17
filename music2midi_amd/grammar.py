"""The MIDI token grammar: which id may follow a decoder prefix (pure Python: no torch, no library).

``MidiTokenizer._tokenize`` writes one shape of sequence: groups in strictly increasing time, each ``time, [ONSET pitch+],
[OFFSET pitch+]`` with at least one of the two lists, ``EOS`` last.  ``MidiTokenizer._decode_tokens`` silently drops whatever does
not fit (a pitch before a time or a mode token, an OFFSET of a pitch that is not sounding, a time that goes backwards, the ids
past the last time id).  ``MidiGrammar`` is that shape as a state machine over (phase, last_time, open_old, open_new):

    phase        allowed next ids
    START        any time id; EOS
    TIME         ONSET; OFFSET iff open_old is not empty
    ONSET_OPEN   pitch not in open_new
    ONSET_LIST   pitch not in open_new; OFFSET iff open_old is not empty; time > last_time; EOS
    OFFSET_OPEN  pitch in open_old
    OFFSET_LIST  pitch in open_old; time > last_time; EOS

``open_old`` are the sounding pitches whose onset lies before the current group, ``open_new`` the onsets of the current group: the
decoder closes only notes with ``onset_t < time_idx``, so an OFFSET can only end a pitch of ``open_old``.  PAD, BOS and the ids from
``special + n_pitch + n_time`` upwards are never allowed.

The allowed set is never empty along a walk that only takes allowed ids: START, ONSET_LIST and OFFSET_LIST always allow EOS and TIME
always allows ONSET; ONSET_OPEN is only entered from TIME, right after the time id cleared ``open_new``, so every pitch is allowed
there, and OFFSET_OPEN is only entered through an OFFSET, which is allowed only while ``open_old`` holds a pitch.

The transition function is total (an id forced by another processor never leaves the state undefined): a time id t sets
``last_time = t``, moves ``open_new`` into ``open_old`` and goes to TIME; ONSET goes to ONSET_OPEN, OFFSET to OFFSET_OPEN; a pitch in
an ONSET phase joins ``open_new`` and goes to ONSET_LIST, in an OFFSET phase it leaves ``open_old`` and goes to OFFSET_LIST, in
START or TIME it changes nothing; PAD, BOS, EOS and the unused ids change nothing.

Out of scope: EOS while notes are still sounding stays legal (the decoder drops those notes, as it does without the grammar;
forbidding it would make empty allowed sets reachable once the last time id is used).  The pitch sets are sets: two notes of one
pitch that sound at the same time are one sounding pitch to the decoder (its first OFFSET closes both), so a second OFFSET of that
pitch is not in the language although ``_tokenize`` writes it for such input.

``T5Transformer.generate(midi_grammar=True)`` applies the same machine on the GPU (csrc/decode.hip); ``prefix_allowed_tokens_fn``
is the callable transformers' ``generate(prefix_allowed_tokens_fn=...)`` takes.
"""
from __future__ import annotations

from typing import Iterable, List, NamedTuple

PAD, BOS, EOS, ONSET, OFFSET = 0, 1, 2, 3, 4          # music2midi_amd.tokenizer (not imported: that module needs torch)

START, TIME, ONSET_OPEN, ONSET_LIST, OFFSET_OPEN, OFFSET_LIST = range(6)
PHASE_NAMES = ("START", "TIME", "ONSET_OPEN", "ONSET_LIST", "OFFSET_OPEN", "OFFSET_LIST")

# device limits (music2midi_amd/csrc/t5.h GrammarState: 128 pitch bits per set; the processed head's vocabulary)
GRAMMAR_MAX_PITCH = 128
GRAMMAR_MAX_VOCAB = 4096


class GrammarState(NamedTuple):
    phase: int = START
    last_time: int = -1
    open_old: frozenset = frozenset()
    open_new: frozenset = frozenset()


class MidiGrammar:
    def __init__(self, special: int, n_pitch: int, n_time: int):
        special, n_pitch, n_time = int(special), int(n_pitch), int(n_time)
        if special <= OFFSET:
            raise ValueError(f"`special` = {special}: the grammar needs the ids PAD, BOS, EOS, ONSET, OFFSET (0 .. {OFFSET}) below the pitch ids")
        if n_pitch < 1 or n_time < 1:
            raise ValueError(f"the grammar needs at least one pitch id and one time id, got n_pitch = {n_pitch}, n_time = {n_time}")
        self.special, self.n_pitch, self.n_time = special, n_pitch, n_time
        self.pitch_offset = special
        self.time_offset = special + n_pitch
        self.end = special + n_pitch + n_time          # the first id past the tokenizer's vocabulary

    @classmethod
    def from_vocab(cls, vocab_size) -> "MidiGrammar":
        """From ``config.tokenizer.vocab_size`` (special / pitch / time)."""
        return cls(vocab_size.special, vocab_size.pitch, vocab_size.time)

    def check_device_limits(self, vocab_size: int) -> None:
        """``ValueError`` unless the GPU head can hold this grammar for a model of ``vocab_size`` ids."""
        if self.n_pitch > GRAMMAR_MAX_PITCH:
            raise ValueError(f"`midi_grammar` on the MI355X path takes at most {GRAMMAR_MAX_PITCH} pitch ids, the tokenizer has {self.n_pitch}")
        if not self.end <= vocab_size <= GRAMMAR_MAX_VOCAB:
            raise ValueError(f"`midi_grammar` on the MI355X path needs special + pitch + time = {self.end} <= vocab_size <= "
                             f"{GRAMMAR_MAX_VOCAB} (the model has {vocab_size})")

    # ------------------------------------------------------------------ machine
    def start(self) -> GrammarState:
        return GrammarState()

    def step(self, state: GrammarState, token: int) -> GrammarState:
        token = int(token)
        phase, last_time, old, new = state
        if self.time_offset <= token < self.end:
            return GrammarState(TIME, token - self.time_offset, old | new, frozenset())
        if token == ONSET:
            return GrammarState(ONSET_OPEN, last_time, old, new)
        if token == OFFSET:
            return GrammarState(OFFSET_OPEN, last_time, old, new)
        if self.pitch_offset <= token < self.time_offset:
            p = token - self.pitch_offset
            if phase in (ONSET_OPEN, ONSET_LIST):
                return GrammarState(ONSET_LIST, last_time, old, new | {p})
            if phase in (OFFSET_OPEN, OFFSET_LIST):
                return GrammarState(OFFSET_LIST, last_time, old - {p}, new)
        return state

    def allowed(self, state: GrammarState) -> List[int]:
        phase, last_time, old, new = state
        out: List[int] = []
        if phase in (START, ONSET_LIST, OFFSET_LIST):
            out.append(EOS)
        if phase == TIME:
            out.append(ONSET)
        if phase in (TIME, ONSET_LIST) and old:
            out.append(OFFSET)
        if phase in (ONSET_OPEN, ONSET_LIST):
            out.extend(self.pitch_offset + p for p in range(self.n_pitch) if p not in new)
        if phase in (OFFSET_OPEN, OFFSET_LIST):
            out.extend(self.pitch_offset + p for p in sorted(old))
        if phase in (START, ONSET_LIST, OFFSET_LIST):
            out.extend(range(self.time_offset + last_time + 1, self.end))
        return out                                     # ascending: specials < pitches < times

    def state_of(self, ids: Iterable[int]) -> GrammarState:
        """The state after a decoder prefix (the start token first; it changes nothing)."""
        state = self.start()
        for token in ids:
            state = self.step(state, token)
        return state

    def accepts(self, ids: Iterable[int]) -> bool:
        """Every id after the start token, up to and including the first EOS, is allowed where it stands (what follows EOS is not
        looked at: a finished row is padded)."""
        ids = [int(i) for i in ids]
        state = self.start()
        for token in ids[1:]:
            if token not in self.allowed(state):
                return False
            if token == EOS:
                return True
            state = self.step(state, token)
        return True

    def prefix_allowed_tokens_fn(self):
        """``(batch_id, input_ids) -> list`` for transformers' ``generate(prefix_allowed_tokens_fn=...)``."""
        def fn(batch_id, input_ids):
            return self.allowed(self.state_of(int(i) for i in input_ids))
        return fn
