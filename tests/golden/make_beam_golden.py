"""Record HF beam search on the tiny config into tests/golden/beam.npz (run by hand; needs transformers).

    python tests/golden/make_beam_golden.py

For every (num_beams, num_return_sequences, length_penalty, early_stopping) of the grid it stores the installed
``T5ForConditionalGeneration.generate(num_beams=..., return_dict_in_generate=True, output_scores=True)``'s sequences and
sequences_scores, on the tiny config with ``synth.force_eos_head`` so that hypotheses finish.  tests/test_beam_cpu.py holds
tests/beam_ref.py (the transformers 4.34 restatement) to them, reading only this file.

Newer transformers releases pad a finished hypothesis with EOS where 4.34 writes pad_token_id; rows are compared only up to
and including their first EOS.
"""
from __future__ import annotations

import itertools
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parents[1]))

from make_golden import build_hf, embeds, ref_config, tiny_t5  # noqa: E402
from music2midi_amd import synth  # noqa: E402
from music2midi_amd.config import T5Geometry  # noqa: E402

B, S, L = 3, 30, 32
GRID = list(itertools.product((2, 4), ("1", "nb"), (0.0, 1.0, 2.0), (False, True, "never")))


def main(out_path=HERE / "beam.npz"):
    t5 = tiny_t5(ref_config())
    geom = T5Geometry(t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom)
    hf = build_hf(t5, sd)
    x = embeds(B, S, geom.d_model)
    out = {"meta": np.asarray([B, S, L], dtype=np.int32)}
    for nb, n_s, lp, es in GRID:
        n = 1 if n_s == "1" else nb
        with torch.no_grad():
            r = hf.generate(inputs_embeds=x, max_length=L, num_beams=nb, num_return_sequences=n, length_penalty=lp,
                            early_stopping=es, do_sample=False, return_dict_in_generate=True, output_scores=True)
        key = f"nb{nb}_n{n}_lp{lp:g}_es{es}"
        out[key + "_ids"] = r.sequences.numpy().astype(np.int16)
        out[key + "_scores"] = r.sequences_scores.numpy().astype(np.float32)
        print(key, tuple(r.sequences.shape), r.sequences_scores.tolist())
    np.savez_compressed(out_path, **out)
    print("wrote", out_path, out_path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
