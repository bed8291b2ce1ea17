"""GPU parity of the training step AT BASELINE configs[4]'s own per-GPU shape and dtypes: the full model (ref config.yaml
model.t5), 16 clips per GPU (batch 128 over 8 GPUs; ref config.yaml:44 trains batches of 16 too), 3 s segments at
dataset.sample_rate 22 050 Hz -> 66 150 samples -> 259 frames -> S = 261 (ref config.yaml:2,4), 256 label positions per clip with
ragged ignored tails (-100, ref transformer.py:30).  ref: music2midi/model.py:32-38, transformer.py:28-39.

The oracle (autograd over oracle/train.py, pinned to HuggingFace by tests/golden/train.npz) runs ONCE per module on the host
(~15 s each for the plain and the MX-emulating pass on 8-16 threads)."""
import copy
import os
import time

import numpy as np
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry

from test_train_gpu import fp8_self_consistency

pytestmark = pytest.mark.gpu

B, F, LD = 16, 259, 256          # S = F + 2 = 261


@pytest.fixture(scope="module")
def c4():
    from oracle.train import T5TrainOracle, leaf_params
    torch.set_num_threads(min(16, os.cpu_count() or 16))
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    feats = torch.from_numpy(synth.normal(5, "feats", (B, F, geom.d_model), 2.0))
    cond = torch.from_numpy(synth.cond_index_batch(2, B))
    labels = torch.from_numpy((synth.uniform01(4, "labels", B * LD) * 330).astype(np.int64).reshape(B, LD)) + 3
    for b in range(B):                       # ragged label lengths as a real batch has them: up to 90 ignored positions at the tail
        cut = (b * 37) % 91
        if cut:
            labels[b, LD - cut:] = -100
    x = torch.zeros((B, F + 2, geom.d_model))
    x[:, 2:] = feats
    orc = T5TrainOracle(geom, leaf_params(sd))
    t0 = time.perf_counter()
    loss, logits, grads = orc.loss_and_grads(feats, cond, labels)
    t_plain = time.perf_counter() - t0
    print(f"[configs4] oracle forward+backward on the host: {t_plain:.1f} s ({torch.get_num_threads()} threads), loss {loss.item():.5f}")
    return dict(geom=geom, sd=sd, feats=feats, cond=cond, labels=labels, x=x, orc=orc, loss=loss, logits=logits, grads=grads)


def _trainer(c4, precision, **env):
    from music2midi_amd.training import NativeTrainer
    from music2midi_amd.transformer import T5Transformer
    model = T5Transformer(copy.deepcopy(DEFAULT_CONFIG), precision="fp32")
    load_t5_state(model, c4["sd"], strict=False)
    model = model.cuda()
    return model, NativeTrainer(model, B, F + 2, LD, precision=precision)


def _agreement(tr, ref):
    cs, ws, worst_max = [], [], 0.0
    for name, (off, shape) in tr.layout.items():
        g = tr.grads[off:off + int(np.prod(shape))].cpu().double()
        r = ref[name].reshape(-1).double()
        if r.norm() < 1e-12:
            continue
        cs.append((float(torch.dot(g, r) / (g.norm() * r.norm() + 1e-30)), name))
        ws.append(float((g - r).norm() / r.norm()))
        worst_max = max(worst_max, float((g - r).abs().max() / (r.abs().max() + 1e-30)))
    return cs, ws, worst_max


def test_fp32_mode_every_gradient_matches_autograd_at_the_config_shape(c4):
    model, tr = _trainer(c4, "fp32")
    loss, logits = tr.forward_backward(c4["x"].cuda(), c4["cond"].cuda(), c4["labels"].cuda(), want_logits=True)
    assert abs(loss.item() - c4["loss"].item()) < 1e-4 * abs(c4["loss"].item()), (loss.item(), c4["loss"].item())
    assert (logits.cpu() - c4["logits"]).abs().max() < 2e-3
    worst = {}
    for name, (off, shape) in tr.layout.items():
        g = tr.grads[off:off + int(np.prod(shape))].view(shape).cpu()
        r = c4["grads"][name]
        worst[name] = float((g - r).abs().max() / (r.abs().max() + 1e-20))
    bad = {k: v for k, v in worst.items() if v > 1e-4}
    print(f"configs[4] shape, fp32: loss {loss.item():.6f} (autograd {c4['loss'].item():.6f}); worst gradient rel err {max(worst.values()):.2e} "
          f"over {len(worst)} tensors")
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:5]
    g1 = tr.grads.clone()                                   # deterministic
    tr.forward_backward(c4["x"].cuda(), c4["cond"].cuda(), c4["labels"].cuda())
    assert torch.equal(g1, tr.grads)
    tr.close()


def test_bf16_mode_tracks_autograd_at_the_config_shape(c4):
    model, tr = _trainer(c4, "bf16")
    loss, _ = tr.forward_backward(c4["x"].cuda(), c4["cond"].cuda(), c4["labels"].cuda())
    cs, ws, _ = _agreement(tr, c4["grads"])
    cmin = min(cs)
    print(f"configs[4] shape, bf16: loss {loss.item():.4f} vs fp32 autograd {c4['loss'].item():.4f}; gradient cosine min {cmin[0]:.5f} ({cmin[1]}), "
          f"median {np.median([c for c, _ in cs]):.5f}, worst rel l2 {max(ws):.3e}")
    assert abs(loss.item() - c4["loss"].item()) < 2e-2 * abs(c4["loss"].item())
    assert cmin[0] > 0.995 and max(ws) < 0.1
    # ... and against the oracle that rounds to bfloat16 wherever this mode stores bfloat16 (values and gradients): what is left is
    # accumulation order, the hardware exp2 of the softmax and the bf16 copies of derived operands
    orc = c4["orc"]
    orc.bf16 = True
    try:
        loss_e, _, grads_e = orc.loss_and_grads(c4["feats"], c4["cond"], c4["labels"])
    finally:
        orc.bf16 = False
    cs_e, ws_e, _ = _agreement(tr, grads_e)
    print(f"configs[4] shape, bf16 vs the bf16-emulating autograd: loss {loss.item():.5f} vs {loss_e.item():.5f}; gradient cosine min {min(cs_e)[0]:.6f} "
          f"({min(cs_e)[1]}), worst rel l2 {max(ws_e):.3e}")
    assert abs(loss.item() - loss_e.item()) < 2e-3 * abs(loss_e.item())
    assert min(cs_e)[0] > 0.9995 and max(ws_e) < 0.05
    # the emulation agrees with ITSELF under a 1e-4 input perturbation to the same 2.7e-2 (bf16 roundings flip and compound over
    # twelve layers): the device is as close to the emulation as anything that is not bit-identical can be
    noise = torch.from_numpy(synth.normal(77, "bf16_floor", tuple(c4["feats"].shape), 1.0))
    orc.bf16 = True
    try:
        _, _, grads_n = orc.loss_and_grads(c4["feats"] * (1.0 + 1e-4 * noise), c4["cond"], c4["labels"])
    finally:
        orc.bf16 = False
    floor = max(float((grads_n[k] - grads_e[k]).norm() / grads_e[k].norm()) for k in grads_e if grads_e[k].norm() > 1e-12)
    print(f"configs[4] shape, bf16: the emulation vs itself under 1e-4 input noise: worst rel l2 {floor:.3e} (device vs emulation {max(ws_e):.3e})")
    assert max(ws_e) < 1.5 * floor
    tr.close()


@pytest.mark.parametrize("parts", [None, "fwd,dx,dw"])
def test_fp8_mode_matches_the_mx_emulating_autograd_at_the_config_shape(c4, parts, monkeypatch):
    """configs[4]'s dtype.  The emulating oracle quantises every product's operands the way that product does on the device
    (oracle/train.py _MxLinear: forward along K, dX along N with dY quantised too, dW bf16 or along M) from bf16-stored values, so
    the comparison is device arithmetic against the same function differentiated on the host.  The bar is the emulation's own
    self-consistency under a 1e-4 input perturbation (test_train_gpu.fp8_self_consistency: fp8 quantiser flips compound with depth,
    ~0.95 / 0.96 at 6 + 6 layers); the per-layer arithmetic is held to 0.98 by test_train_gpu's one-layer case."""
    if parts:
        monkeypatch.setenv("M2M_FP8_PARTS", parts)
    model, tr = _trainer(c4, "fp8")
    loss, _ = tr.forward_backward(c4["x"].cuda(), c4["cond"].cuda(), c4["labels"].cuda())
    g1 = tr.grads.clone()
    loss_b, _ = tr.forward_backward(c4["x"].cuda(), c4["cond"].cuda(), c4["labels"].cuda())
    assert torch.equal(g1, tr.grads) and loss.item() == loss_b.item()
    orc = c4["orc"]
    orc.mx8, orc.mx8_dw, orc.bf16 = True, bool(parts), True
    try:
        t0 = time.perf_counter()
        loss_o, _, grads_o = orc.loss_and_grads(c4["feats"], c4["cond"], c4["labels"])
        dt = time.perf_counter() - t0
        fmin, fmed = fp8_self_consistency(orc, c4["feats"], c4["cond"], c4["labels"], grads_o)
    finally:
        orc.mx8, orc.mx8_dw, orc.bf16 = False, False, False
    cs, ws, _ = _agreement(tr, grads_o)
    ps, _, _ = _agreement(tr, c4["grads"])
    cmin = min(cs)
    print(f"configs[4] shape, fp8 ({parts or 'fwd,dx'}): loss {loss.item():.4f} (MX-emulating autograd {loss_o.item():.4f} in {dt:.0f} s, fp32 autograd "
          f"{c4['loss'].item():.4f}); gradient cosine vs the emulation min {cmin[0]:.4f} ({cmin[1]}) / median {np.median([c for c, _ in cs]):.4f}, "
          f"worst rel l2 {max(ws):.3f}; the emulation vs itself under 1e-4 input noise min {fmin:.4f} / median {fmed:.4f}; "
          f"vs unquantised autograd min {min(ps)[0]:.4f} / median {np.median([c for c, _ in ps]):.4f}")
    assert abs(loss.item() - loss_o.item()) < 5e-3 * abs(loss_o.item())
    assert np.median([c for c, _ in cs]) > fmed - 0.015 and cmin[0] > fmin - 0.03      # (the minimum over 146 tensors is itself a noisy draw: wider)
    # absolute floors beside the relative bar (measured 0.958 / 0.975 against the emulation, 0.92 / 0.94 against plain autograd)
    assert cmin[0] > 0.93 and np.median([c for c, _ in cs]) > 0.95
    assert min(ps)[0] > 0.88 and np.median([c for c, _ in ps]) > 0.91
    tr.close()


FP8_PRODUCTS = ["encoder.block.0.layer.0.SelfAttention.q.weight", "encoder.block.0.layer.1.DenseReluDense.wi_0.weight",
                "encoder.block.0.layer.1.DenseReluDense.wo.weight", "encoder.block.5.layer.0.SelfAttention.v.weight",
                "encoder.block.5.layer.1.DenseReluDense.wi_1.weight", "encoder.block.5.layer.1.DenseReluDense.wo.weight",
                "decoder.block.5.layer.0.SelfAttention.q.weight", "decoder.block.5.layer.1.EncDecAttention.k.weight",
                "decoder.block.5.layer.1.EncDecAttention.o.weight", "decoder.block.5.layer.2.DenseReluDense.wo.weight"]


def test_fp8_products_of_layers_0_5_11_teacher_forced_at_the_config_shape(c4):
    """VERDICT r3 #5.  The end-to-end fp8 bar above is the emulation's own chaos floor (~0.95 at 6 + 6 layers): a wrong scale on ONE
    late product would hide under it.  Here the compounding is taken out: the MX-emulating oracle runs once at the config shape
    (16 x 261 x 256) and records, for ten projections of the first encoder layer, the last encoder layer and the last decoder layer
    (the 12th), the product's bf16 input x, its output gradient dy and its weight; the DEVICE then computes each of the three
    products from those same tensors and each is held to the emulation of THAT product: relative l2 <= 3e-4 (measured on MI355X:
    3.4e-6 ... 4.1e-5 over the 30 products — the matrix core's limited-precision accumulate; the one-layer whole-step bar is cosine
    0.98: a product on its own has no flips to compound, so it is held three orders tighter).  The legs:
      fwd      y = Qk(x) Qk(W)^T      m2m_mx8_matmul_bf16a fused: mxgemm_q_kernel, bf16 operand quantised in the staging; the WEIGHT goes
      dx       Qn(dy) Qn(W^T)^T       through the row quantiser here (W, resp. a pre-transposed W^T), not through the step's weight quantiser
      dw       Qm(dy^T) Qm(x^T)^T     m2m_mx8_matmul_f32 on PRE-TRANSPOSED operands: row quantiser + unsplit product, not the step's route
      dx_step  the step's dX route    m2m_mx8_step_product kind 1 (mx8_dx, what Ops::dX calls): weights from mxq_weights_kernel's
                                      transposed image, dy quantised in the staging
      dw_step  the step's dW route    m2m_mx8_step_product kind 2 (mx8_dw, what Ops::dW_on calls): the transposing quantiser mxq_cols on
                                      dy and x, then the split-K product + reduce under the step's own policy
    The forward outputs are also compared with what the oracle's own pass produced (same tensors: bit-for-bit the
    emulation formula)."""
    import ctypes as C
    from music2midi_amd import native
    from oracle.mx8 import mx_quant_dequant
    lib = native.load()
    orc = c4["orc"]
    orc.capture = {k: {} for k in FP8_PRODUCTS}
    orc.mx8, orc.mx8_dw, orc.bf16 = True, True, True
    try:
        orc.loss_and_grads(c4["feats"], c4["cond"], c4["labels"])
    finally:
        orc.mx8, orc.mx8_dw, orc.bf16 = False, False, False
        cap, orc.capture = orc.capture, None

    def dev_bf16a(a, b):            # a [M, K] (bf16-representable), b [N, K] fp32 -> fp32 [M, N]; the fused-quantisation kernel of the step
        a16 = a.to(torch.bfloat16).cuda().contiguous()
        b_d = b.cuda().contiguous()
        c_d = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device="cuda")
        native.check(lib.m2m_mx8_matmul_bf16a(a16.data_ptr(), b_d.data_ptr(), a.shape[0], b.shape[0], a.shape[1], 0, 1, c_d.data_ptr(), native.stream_handle()),
                     "m2m_mx8_matmul_bf16a")
        return c_d.cpu()

    def dev_f32(a, b):
        a_d, b_d = a.cuda().contiguous(), b.cuda().contiguous()
        c_d = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device="cuda")
        native.check(lib.m2m_mx8_matmul_f32(a_d.data_ptr(), b_d.data_ptr(), a.shape[0], b.shape[0], a.shape[1], 0, c_d.data_ptr(), native.stream_handle()),
                     "m2m_mx8_matmul_f32")
        return c_d.cpu()

    def dev_step(kind, a, b, M, N, K):      # the fp8 step's own route (include/music2midi_amd.h m2m_mx8_step_product), e4m3 gradients, fp32 store
        a16 = a.to(torch.bfloat16).cuda().contiguous()
        b_d = (b.to(torch.bfloat16) if kind == 2 else b).cuda().contiguous()
        c_d = torch.empty((M, K) if kind == 1 else (N, K), dtype=torch.float32, device="cuda")
        native.check(lib.m2m_mx8_step_product(kind, a16.data_ptr(), b_d.data_ptr(), M, N, K, 0, 1, 1, c_d.data_ptr(), None, 0.0, 0, 0, None, None,
                                              native.stream_handle()), "m2m_mx8_step_product")
        return c_d.cpu()

    def agree(got, want):
        g, w = got.reshape(-1).double(), want.reshape(-1).double()
        return float(torch.dot(g, w) / (g.norm() * w.norm() + 1e-300)), float((g - w).norm() / (w.norm() + 1e-300))

    worst = (1.0, 0.0, "")
    for name in FP8_PRODUCTS:
        rec = cap[name]
        assert {"x", "y", "dy"} <= set(rec), (name, sorted(rec))
        w = orc.w(name).detach()
        x2 = rec["x"].reshape(-1, rec["x"].shape[-1]).bfloat16().float()
        dy2 = rec["dy"].reshape(-1, rec["dy"].shape[-1]).bfloat16().float()
        want_y = mx_quant_dequant(x2, "e4m3") @ mx_quant_dequant(w, "e4m3").T
        assert torch.equal(want_y, rec["y"].reshape(want_y.shape)), name                     # the recorded pass used this very formula
        want_dx = mx_quant_dequant(dy2, "e4m3") @ mx_quant_dequant(w.T.contiguous(), "e4m3").T
        want_dw = mx_quant_dequant(dy2.T.contiguous(), "e4m3") @ mx_quant_dequant(x2.T.contiguous(), "e4m3").T
        res = {"fwd": agree(dev_bf16a(x2, w), want_y), "dx": agree(dev_bf16a(dy2, w.T.contiguous()), want_dx),
               "dw": agree(dev_f32(dy2.T.contiguous(), x2.T.contiguous()), want_dw),
               "dx_step": agree(dev_step(1, dy2, w, dy2.shape[0], w.shape[0], w.shape[1]), want_dx),
               "dw_step": agree(dev_step(2, dy2, x2, dy2.shape[0], w.shape[0], w.shape[1]), want_dw)}
        print(f"[fp8 product] {name} x {tuple(x2.shape)} dy {tuple(dy2.shape)}: " + "; ".join(f"{k} cos {c:.7f} rel l2 {r:.2e}" for k, (c, r) in res.items()))
        for k, (c, r) in res.items():
            assert np.isfinite(c) and c >= 0.999999 and r <= 3e-4, (name, k, c, r)
            if c < worst[0]:
                worst = (c, r, f"{name} {k}")
    print(f"[fp8 product] worst of {5 * len(FP8_PRODUCTS)} products: cosine {worst[0]:.7f} (rel l2 {worst[1]:.2e}) at {worst[2]}")


def test_dropout_step_is_reproducible_and_graph_replay_equals_direct_issue_at_the_config_shape(c4, monkeypatch):
    from music2midi_amd.training import NativeTrainer
    model, tr_graph = _trainer(c4, "bf16")
    monkeypatch.setenv("M2M_TRAIN_GRAPH", "0")
    tr_direct = NativeTrainer(model, B, F + 2, LD, precision="bf16")
    x, cond, labels = c4["x"].cuda(), c4["cond"].cuda(), c4["labels"].cuda()
    for tr in (tr_graph, tr_direct):
        tr.set_dropout(0.1, seed=21)
    losses = []
    for call in range(4):                                    # call 0 direct, call 1 captures, 2.. replay
        la, _ = tr_graph.forward_backward(x, cond, labels)
        ga = tr_graph.grads.clone()
        lb, _ = tr_direct.forward_backward(x, cond, labels)
        assert la.item() == lb.item() and torch.equal(ga, tr_direct.grads), f"call {call}: graph replay differs from direct issue"
        losses.append(la.item())
    assert len(set(losses)) == 4                             # the masks advance from call to call
    tr_graph.set_dropout(0.1, seed=21)                       # and the sequence restarts reproducibly
    l0, _ = tr_graph.forward_backward(x, cond, labels)
    assert l0.item() == losses[0]
    # the loss with dropout stays near the dropout-free one (a statistical bound, not a parity claim)
    assert abs(l0.item() - c4["loss"].item()) < 0.1 * abs(c4["loss"].item())
    tr_graph.close(); tr_direct.close()
