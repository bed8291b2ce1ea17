#!/usr/bin/env python3
"""SHA-256 over loss, logits and the flat gradient buffer of the forward_backward calls of a case, per kernel family of the training
attention and per host path of the pass (grouped, per-product, accumulating, split), with the launches of the captured graph and
the bytes of the trainer's arena.  For host-side changes of the training pass: run once per build and compare the lines.

    M2M_LIBRARY=<the other build> python tools/train_step_digest.py > a.txt;  python tools/train_step_digest.py > b.txt;  diff a.txt b.txt

Weights, inputs and the dropout seed are fixed; the bits depend on the ROCm build, so the digests are compared, never stored.
(tiny model; the trainer's switches are latched when it is created, so every case sets its environment before it creates one)

For changes of the encoder-side kernels (enc_gemm.hip, enc_attn.hip) run it a second time with
M2M_GEMM_SMALL_BELOW=0 M2M_NORM_GEMM=0 M2M_RESID_PANEL=0 M2M_ATTN_WIDE=0 set for the whole process: every product then takes
gemm_kernel's 128x128 tile and the bf16 attention takes attn_kernel, forms the default run does not launch."""
import hashlib
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from music2midi_amd import native, synth  # noqa: E402
from music2midi_amd.checkpoint import load_t5_state  # noqa: E402
from music2midi_amd.config import T5Geometry, load_config  # noqa: E402
from music2midi_amd.training import NativeTrainer  # noqa: E402
from music2midi_amd.transformer import T5Transformer  # noqa: E402
from test_t5_gpu import tiny_config  # noqa: E402

SWITCHES = ("M2M_TRAIN_GRAPH", "M2M_TRAIN_ATTN", "M2M_TRAIN_DW_GROUP", "M2M_TRAIN_SIDE")
# (precision, B, F, Ld, dropout, environment, mode): stripes; unfused past 512 keys; whole-head; the same on stripes; mixed (402 > AH_MAX_S); fp8
SHAPES = [("fp32", 3, 21, 14, 0.0, {}, ""), ("fp32", 3, 21, 14, 0.1, {}, ""), ("fp32", 1, 530, 5, 0.0, {}, ""), ("fp32", 1, 530, 5, 0.1, {}, ""),
          ("bf16", 2, 70, 33, 0.1, {}, ""), ("bf16", 2, 70, 33, 0.1, {"M2M_TRAIN_ATTN": "stripes"}, ""), ("bf16", 2, 400, 37, 0.1, {}, ""),
          ("fp8", 3, 21, 14, 0.0, {}, ""),
          # the host paths beside the grouped single pass: a launch per weight gradient on the side stream (the two alternating ring
          # sets) and on one stream; accumulation (mode "accum": a scaled overwriting call, then a scaled adding one); the split pass of
          # the data-parallel overlap (mode "split": a sync stream set, the second half of the tables, the second graph)
          ("bf16", 3, 21, 14, 0.1, {"M2M_TRAIN_DW_GROUP": "0"}, ""), ("bf16", 3, 21, 14, 0.1, {"M2M_TRAIN_DW_GROUP": "0", "M2M_TRAIN_SIDE": "0"}, ""),
          ("bf16", 3, 21, 14, 0.1, {}, "accum"), ("fp32", 3, 21, 14, 0.1, {}, "accum"), ("bf16", 3, 21, 14, 0.1, {}, "split")]
CASES = SHAPES + [(*c[:5], {**c[5], "M2M_TRAIN_GRAPH": "0"}, c[6]) for c in SHAPES]


def main():
    cfg = tiny_config()
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    model = T5Transformer(cfg, precision="fp32")
    load_t5_state(model, sd, strict=False)
    model = model.cuda()
    for prec, B, F, Ld, p, env, mode in CASES:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        x = torch.zeros((B, F + 2, geom.d_model))
        x[:, 2:] = torch.from_numpy(synth.normal(5, "feats", (B, F, geom.d_model), 2.0))
        cond = torch.from_numpy(synth.cond_index_batch(2, B)).cuda()
        labels = (torch.from_numpy((synth.uniform01(4, "labels", B * Ld) * 330).astype(np.int64).reshape(B, Ld)) + 3).cuda()
        x = x.cuda()
        tr = NativeTrainer(model, B, F + 2, Ld, precision=prec)
        h = hashlib.sha256()
        if p:
            tr.set_dropout(p, seed=1234)
        if mode == "split":
            tr.set_sync_stream(torch.cuda.Stream())
        # the calls of one round; a graph build replays the captured graph of a key from that key's second call on: three rounds
        calls = [dict(grad_scale=0.5, accumulate=False), dict(grad_scale=0.5, accumulate=True)] if mode == "accum" else [{}]
        for _ in range(3):
            for kw in calls:
                loss, logits = tr.forward_backward(x, cond, labels, want_logits=True, **kw)
                torch.cuda.synchronize()
                for a in (loss, logits, tr.grads):
                    h.update(a.cpu().numpy().tobytes())
        what = " ".join([f"{k}={v}" for k, v in env.items()] + ([mode] if mode else [])) or "-"
        ws = int(native.load().m2m_trainer_workspace_bytes(tr.handle))
        print(f"{prec} B={B} F={F} Ld={Ld} p={p} {what}: graph nodes {tr.graph_nodes()} workspace {ws} sha256 {h.hexdigest()}", flush=True)
        tr.close()


if __name__ == "__main__":
    main()
