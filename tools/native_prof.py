"""Reference-native geometry under rocprofv3: 128 x 48 000 samples, S = 190, 256 tokens (kernel-stats run).

    python tools/native_prof.py [clips [max_length [precision [samples]]]]        (220500 samples: S = 864)"""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
from music2midi_amd.input import ModelInputs
from music2midi_amd.transformer import T5Transformer
arg = dict(enumerate(sys.argv[1:]))
B, L, prec, T = int(arg.get(0, 128)), int(arg.get(1, 1024)), arg.get(2, "bf16"), int(arg.get(3, 48000))
g = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
m = T5Transformer(DEFAULT_CONFIG, precision=prec); load_t5_state(m, synth.t5_state_dict(g, seed=0), strict=False); m = m.cuda().eval()
wav = torch.from_numpy(synth.waveform_batch(1000, B, T)).cuda(); cond = torch.from_numpy(synth.cond_index_batch(1000, B)).cuda()
for _ in range(2): t = m.generate(ModelInputs(input_waveform=wav, cond_index=cond), max_length=L)
torch.cuda.synchronize(); print(t.shape)
