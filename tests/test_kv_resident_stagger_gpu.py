"""GPU: which cross-K/V layers a chain keeps cache-resident is a cache policy, never a result.

decode_launch_attn (csrc/decode.hip) loads K/V non-temporally once one decode step's K/V working set

    layers x 2 x B x inner x (S + max_dec) x element size  >  200e6 bytes

with B, S the encoded problem and max_dec the SESSION's decoder capacity; `resident` layers of cross K/V (M2M_KV_RESIDENT_LAYERS, or
180e6 / (2 x B x inner x S x element size)) then keep the default policy, and with exactly two chains and M2M_KV_RESIDENT_STAGGER
chain i keeps the window [i r, i r + r) mod 6 (t5.h kv_layer_resident).  The shape here is B = 24 (two chains of 12), S = 8,
max_length 40 on a session sized for 700 positions by a first call (a session keeps the largest capacity it was asked for):
6 x 2 x 24 x 512 x (8 + 700) x 2 = 208.8e6 in bf16, twice that in fp32 - the non-temporal route; at 40 positions alone it would be
14.2e6 and no launch would be non-temporal.  A layer is 2 x 24 x 512 x 8 x 2 = 0.39 MB, so the budget keeps all six (unset); the
legs 0 / 3 / 6 stream all, half (the two windows {0, 1, 2} and {3, 4, 5} with the stagger) and none.  Both switches are latched
per session: a model per leg."""
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

pytestmark = pytest.mark.gpu

GEOM = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
LEGS = [(stagger, layers) for stagger in ("0", "1") for layers in (None, "0", "3", "6")]


@pytest.mark.parametrize("eos", [False, True], ids=["no_eos", "repacks"])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_ids_do_not_depend_on_the_resident_windows(monkeypatch, precision, eos):
    sd = synth.t5_state_dict(GEOM, seed=0)
    synth.perturb_layer_norms(sd, 0)
    if eos:
        synth.force_eos_head(sd, GEOM, active=340, eos_scale=1.6)
    x = torch.from_numpy(synth.normal(9, "embeds", (24, 8, GEOM.d_model), 3.0)).cuda()
    want = None
    for stagger, layers in LEGS:
        monkeypatch.setenv("M2M_KV_RESIDENT_STAGGER", stagger)
        if layers is None:
            monkeypatch.delenv("M2M_KV_RESIDENT_LAYERS", raising=False)
        else:
            monkeypatch.setenv("M2M_KV_RESIDENT_LAYERS", layers)
        m = T5Transformer(DEFAULT_CONFIG, precision=precision)
        load_t5_state(m, sd, strict=False)
        m = m.cuda().eval()
        long_ids = m.generate_from_embeds(x, max_length=700).cpu()        # sizes the session; with the EOS head it re-packs
        stats = m.repack_stats()
        got = (long_ids, stats, m.generate_from_embeds(x, max_length=40).cpu())
        del m
        if eos:
            assert stats[0] >= 1 and stats[1] >= 1, (stagger, layers, stats)     # re-planned chains follow the same rule
        else:
            assert long_ids.shape[1] == 700 and torch.equal(got[2], long_ids[:, :40])
        if want is None:
            want = got
            continue
        assert got[1] == want[1], (stagger, layers)
        for a, b in ((got[0], want[0]), (got[2], want[2])):
            assert a.shape == b.shape and torch.equal(a, b), (stagger, layers)
