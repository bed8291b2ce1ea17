"""Note array -> MIDI object (ref: music2midi/utils.py:5-20).

With ``pretty_midi`` installed this returns a real ``PrettyMIDI`` exactly as the
reference does (resolution 384, 120 bpm, one piano instrument, invalid notes
removed).  The image used for the MI355X build has no pretty_midi, so a small
stand-in with the members the reference's callers touch (``instruments[0].notes``,
``get_end_time``, ``write``, ``synthesize``, ``fluidsynth``) is returned instead; its two
audio methods go through ``music2midi_amd.render``: the built-in wavetable voice, not a
SoundFont.
"""
from __future__ import annotations

import struct
from typing import List

import numpy as np

try:  # optional
    import pretty_midi as _pm
except Exception:  # pragma: no cover - depends on the image
    _pm = None


class SimpleNote:
    __slots__ = ("start", "end", "pitch", "velocity")

    def __init__(self, start, end, pitch, velocity):
        self.start, self.end, self.pitch, self.velocity = float(start), float(end), int(pitch), int(velocity)


class SimpleInstrument:
    def __init__(self, program=0, name="Piano"):
        self.program, self.name, self.is_drum = program, name, False
        self.notes: List[SimpleNote] = []


class SimpleMIDI:
    """Just enough of PrettyMIDI for the callers of Music2MIDI.generate."""

    def __init__(self, resolution=384, initial_tempo=120.0):
        self.resolution, self.initial_tempo = resolution, initial_tempo
        self.instruments: List[SimpleInstrument] = []
        self.beat_times = None               # two or more beat times (seconds): ``write`` lays a tempo map along them

    def remove_invalid_notes(self):
        for inst in self.instruments:
            inst.notes = [n for n in inst.notes if n.end > n.start]

    def get_end_time(self) -> float:
        ends = [n.end for inst in self.instruments for n in inst.notes]
        return max(ends) if ends else 0.0

    def note_array(self) -> np.ndarray:
        rows = [[n.start, n.end, n.pitch, n.velocity] for inst in self.instruments for n in inst.notes]
        return np.asarray(rows, dtype=np.float64).reshape(-1, 4)

    def write(self, path) -> None:
        """Standard MIDI file.  One instrument (or none): format 0, one track.  Several: format 1 - a tempo track, then one track
        per instrument with its name (a track-name meta event), its program change and its notes on channel ``index % 16``.

        With ``beat_times`` of two or more beats the file carries a tempo map and its bars and beats follow the music: beat k lies
        at tick ``(k + 1) * resolution`` (``k * resolution`` when the first beat is at time 0), there is one set-tempo event per beat
        with ``round(1e6 * interval)`` microseconds per quarter, the span from time 0 to the first beat has a tempo of its own and
        after the last beat the last interval continues.  Every event's tick goes through that piecewise-linear map, so absolute
        times are preserved and the file still plays in sync with the recording.  An interval outside the 24-bit tempo range
        (1 .. 16777215 microseconds) raises ``ValueError``.  Without ``beat_times`` the bytes are what they always were."""
        ticks_per_second = self.resolution * self.initial_tempo / 60.0
        to_tick = lambda seconds: int(round(seconds * ticks_per_second))           # noqa: E731
        tempo_events = []
        if self.beat_times is not None and len(self.beat_times) >= 2:
            to_tick, tempo_events = self._tempo_map()

        def vlq(v):
            out = [v & 0x7F]
            v >>= 7
            while v:
                out.append((v & 0x7F) | 0x80)
                v >>= 7
            return bytes(reversed(out))

        def note_events(instruments, channel, extra=()) -> bytes:
            events = list(extra)
            for inst in instruments:
                for n in inst.notes:
                    events.append((to_tick(n.start), 1, 0x90 | channel, n.pitch, max(1, min(127, n.velocity))))
                    events.append((to_tick(n.end), 0, 0x80 | channel, n.pitch, 0))
            events.sort(key=lambda e: (e[0], e[1]))
            data, last = b"", 0
            for tick, _, status, pitch, vel in events:
                if status == 0xFF:                                              # a set-tempo event: `pitch` holds the microseconds
                    data += vlq(tick - last) + b"\xff\x51\x03" + struct.pack(">I", pitch)[1:]
                else:
                    data += vlq(tick - last) + bytes([status, pitch & 0x7F, vel & 0x7F])
                last = tick
            return data

        tempo = b"\x00\xff\x51\x03" + struct.pack(">I", int(round(60_000_000 / self.initial_tempo)))[1:]
        end = b"\x00\xff\x2f\x00"
        if tempo_events:
            tempo = b""                                                         # the map's first event stands at tick 0
        if len(self.instruments) <= 1:
            program = b"\x00\xc0" + bytes([self.instruments[0].program if self.instruments else 0])
            tracks = [tempo + program + note_events(self.instruments, 0, tempo_events) + end]     # format 0: the map shares the track
        else:
            tracks = [tempo + note_events([], 0, tempo_events) + end]
            for index, inst in enumerate(self.instruments):
                channel, name = index % 16, str(inst.name or "").encode("utf-8")
                tracks.append(b"\x00\xff\x03" + vlq(len(name)) + name + b"\x00" + bytes([0xC0 | channel, int(inst.program) & 0x7F])
                              + note_events([inst], channel) + end)
        with open(path, "wb") as f:
            f.write(b"MThd" + struct.pack(">IHHH", 6, 0 if len(tracks) == 1 else 1, len(tracks), self.resolution))
            for track in tracks:
                f.write(b"MTrk" + struct.pack(">I", len(track)) + track)

    def _tempo_map(self):
        """(seconds -> tick, the set-tempo events as (tick, -1, 0xFF, microseconds, 0)) of ``beat_times``."""
        beats = np.asarray(self.beat_times, dtype=np.float64).reshape(-1)
        if not np.isfinite(beats).all() or beats[0] < 0 or not (np.diff(beats) > 0).all():
            raise ValueError("SimpleMIDI.write: beat_times have to be finite, not negative and strictly increasing")
        res = int(self.resolution)
        lead = 0 if beats[0] == 0 else 1                                        # quarters before the first beat
        spans = ([float(beats[0])] if lead else []) + [float(d) for d in np.diff(beats)] + [float(beats[-1] - beats[-2])]
        starts = np.concatenate([[0.0] if lead else [], beats])                 # where span i begins; span i begins at tick i * res
        events = []
        for i, span in enumerate(spans):
            us = int(round(1e6 * span))
            if not 1 <= us <= 0xFFFFFF:
                raise ValueError(f"SimpleMIDI.write: a beat interval of {span} s is outside the 24-bit tempo range")
            events.append((i * res, -1, 0xFF, us, 0))

        def to_tick(seconds: float) -> int:
            i = min(max(int(np.searchsorted(starts, seconds, side="right")) - 1, 0), len(spans) - 1)
            return int(round(i * res + (seconds - starts[i]) / spans[i] * res))
        return to_tick, events

    def synthesize(self, fs=44100) -> np.ndarray:
        """The notes as audio at ``fs``, float64 like ``PrettyMIDI.synthesize``: the wavetable voice of ``music2midi_amd.render``,
        rendered on the GPU when one is present and by the host definition otherwise (the same samples bit for bit)."""
        return self._render(fs, normalize=False)

    def fluidsynth(self, fs=44100, sf2_path=None) -> np.ndarray:
        """``synthesize(fs)`` divided by its peak, as ``PrettyMIDI.fluidsynth`` normalises.  The timbre is the built-in voice of
        ``music2midi_amd.render`` and NOT a SoundFont: a given ``sf2_path`` needs the real pretty_midi + fluidsynth packages."""
        if sf2_path is not None:
            raise ImportError("rendering through a SoundFont needs the real pretty_midi + fluidsynth packages")
        return self._render(fs, normalize=True)

    def _render(self, fs, normalize: bool) -> np.ndarray:
        import torch
        from . import render
        device = "cuda" if torch.cuda.is_available() else "cpu"
        return render.render(self.note_array(), fs, normalize=normalize, device=device).cpu().numpy().astype(np.float64)


def simple_midi(notes: np.ndarray) -> SimpleMIDI:
    """rows (onset_s, offset_s, pitch, velocity) -> the stand-in, whether or not pretty_midi is installed."""
    midi = SimpleMIDI(resolution=384, initial_tempo=120.0)
    inst = SimpleInstrument(program=0, name="Piano")
    inst.notes = [SimpleNote(s, e, p, v) for s, e, p, v in notes]
    midi.instruments.append(inst)
    midi.remove_invalid_notes()
    return midi


def numpy_to_midi(notes: np.ndarray):
    """rows (onset_s, offset_s, pitch, velocity) -> PrettyMIDI (or the stand-in above)."""
    if _pm is None:
        return simple_midi(notes)
    midi = _pm.PrettyMIDI(resolution=384, initial_tempo=120.0)
    inst = _pm.Instrument(program=0, name="Piano")
    inst.notes = [_pm.Note(start=s, end=e, pitch=int(p), velocity=int(v)) for s, e, p, v in notes]
    midi.instruments.append(inst)
    midi.remove_invalid_notes()
    return midi
