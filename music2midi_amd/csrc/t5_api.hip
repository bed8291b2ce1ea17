// C ABI of the T5 encoder/decoder path: model (repacked weights), session (workspace +
// captured decode-step graph), encode, greedy generate, teacher-forced decode, bench hooks.
#include "carver.h"
#include "env.h"
#include "t5.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <memory>
#include <vector>

using namespace m2m;

// ---------------------------------------------------------------- buckets ---
// T5 relative-position bucket (hf: models/t5/modeling_t5.py:217-262).  HF evaluates the log
// branch in float32 and truncates; the same float32 expression is used here and the result
// is pinned against the integer table of SURVEY.md §8a-A6 by tests/test_host_logic.py.
extern "C" int m2m_rel_bucket(int rel, int bidirectional, int num_buckets, int max_distance) {
  int bucket = 0;
  int nb = num_buckets;
  int n;
  if (bidirectional) {
    nb /= 2;
    if (rel > 0) bucket += nb;
    n = rel < 0 ? -rel : rel;
  } else {
    n = rel < 0 ? -rel : 0;
  }
  const int max_exact = nb / 2;
  if (n < max_exact) return bucket + n;
  const float ratio = logf((float)n / (float)max_exact) / (float)log((double)max_distance / (double)max_exact);
  int large = max_exact + (int)(ratio * (float)(nb - max_exact));
  if (large > nb - 1) large = nb - 1;
  return bucket + large;
}

// ------------------------------------------------------------------ model ---
extern "C" int m2m_model_create(const m2m_t5_geometry* geom, const m2m_t5_weights* w, int precision, void* stream,
                                m2m_model** out) {
  M2M_REQUIRE(geom && w && out, "m2m_model_create: null argument");
  M2M_REQUIRE(precision == M2M_PREC_FP32 || precision == M2M_PREC_BF16, "m2m_model_create: bad precision %d", precision);
  const m2m_t5_geometry& g = *geom;
  M2M_REQUIRE(g.d_kv == DK, "m2m_model_create: d_kv=%d unsupported (attention kernels are specialised for 64)", g.d_kv);
  M2M_REQUIRE(g.d_model == 128 || g.d_model == 256 || g.d_model == 384 || g.d_model == 512,
              "m2m_model_create: d_model=%d must be 128, 256, 384 or 512 (the reduction lengths the decode kernels are "
              "instantiated for; the fused decode attention projects with 2 lanes per output column of a 1024-thread workgroup)",
              g.d_model);
  M2M_REQUIRE(g.d_ff >= 64 && g.d_ff % 64 == 0, "m2m_model_create: d_ff=%d must be a multiple of 64", g.d_ff);
  M2M_REQUIRE((g.num_heads * g.d_kv) % 128 == 0 && g.num_heads * g.d_kv <= 1152, "m2m_model_create: num_heads*d_kv=%d must be a multiple of 128, <= 1152", g.num_heads * g.d_kv);
  M2M_REQUIRE(g.num_heads >= 1 && g.num_layers >= 1 && g.num_decoder_layers >= 1 && g.vocab_size >= 2,
              "m2m_model_create: bad geometry");
  // the decode kernels map an out-of-range token to pad_token_id and read its embedding row: every special id must be a row
  M2M_REQUIRE(g.pad_token_id >= 0 && g.pad_token_id < g.vocab_size && g.eos_token_id >= 0 && g.eos_token_id < g.vocab_size &&
                  g.decoder_start_token_id >= 0 && g.decoder_start_token_id < g.vocab_size,
              "m2m_model_create: pad_token_id=%d, eos_token_id=%d and decoder_start_token_id=%d must lie in [0, vocab_size=%d)",
              g.pad_token_id, g.eos_token_id, g.decoder_start_token_id, g.vocab_size);
  M2M_REQUIRE(g.num_buckets >= 4 && g.num_buckets % 2 == 0 && g.max_distance > g.num_buckets / 2,
              "m2m_model_create: bad relative-attention geometry");
  M2M_REQUIRE(w->shared && w->lm_head && w->enc_rel_bias && w->dec_rel_bias && w->enc_final_ln && w->dec_final_ln &&
                  w->enc && w->dec, "m2m_model_create: null weight pointer");
  hipStream_t st = (hipStream_t)stream;
  const int d = g.d_model, dff = g.d_ff, inner = g.num_heads * g.d_kv, V = g.vocab_size;
  const int Le = g.num_layers, Ld = g.num_decoder_layers;
  const size_t es = precision == M2M_PREC_BF16 ? 2 : 4;
  const int vocab_pad = ceil_div(V, 16) * 16;

  // ---- one blob: every packed tensor is declared once, in layout order ----
  m2m_model* m = new m2m_model();
  m->g = g; m->precision = precision; m->inner = inner; m->vocab_pad = vocab_pad; m->esize = es;
  m->enc.resize(Le); m->dec.resize(Ld);
  Carver c;
  auto F = [&](const float*& member, int64_t elems) { c.take(member, elems * 4); };
  auto T = [&](const void*& member, int64_t elems) { c.take(member, elems * es); };
  for (EncLayerPacked& L : m->enc) {
    F(L.ln0, d); T(L.wqkv, (int64_t)3 * inner * d); T(L.wo, (int64_t)d * inner);
    F(L.ln1, d); T(L.wi, (int64_t)2 * dff * d); T(L.wo_ff, (int64_t)d * dff);
  }
  for (DecLayerPacked& L : m->dec) {
    F(L.ln0, d); T(L.wqkv, (int64_t)3 * inner * d); T(L.wo, (int64_t)d * inner);
    F(L.ln1, d); T(L.wcq, (int64_t)inner * d); T(L.wco, (int64_t)d * inner);
    F(L.ln2, d); T(L.wi, (int64_t)2 * dff * d); T(L.wo_ff, (int64_t)d * dff); T(L.ff_img, (int64_t)3 * dff * d);
    T(L.wo_img, (int64_t)d * inner); T(L.wco_img, (int64_t)d * inner);
  }
  F(m->enc_final_ln, d); F(m->dec_final_ln, d);
  F(m->shared, (int64_t)V * d);
  T(m->lm_head, (int64_t)vocab_pad * d);
  T(m->wckv, (int64_t)Ld * 2 * inner * d);
  // the layer-0 token tables (t5.h): part of the blob, so m2m_model_checksum covers them like every other byte the kernels read
  const int64_t tab_elems = (int64_t)g.num_heads * V * DK;
  const bool tables = V <= 65535 && tab_elems * (int64_t)(4 + 2 * es) <= TOKEN_TABLES_MAX_BYTES;
  if (tables) { F(m->q0_tab, tab_elems); T(m->k0_tab, tab_elems); T(m->v0_tab, tab_elems); }
  m->blob_bytes = c.off;
  hipError_t e = hipMalloc(&m->blob, (size_t)c.off);
  if (e != hipSuccess) {
    set_error("m2m_model_create: hipMalloc(%lld) failed: %s", (long long)c.off, hipGetErrorString(e));
    delete m;
    return M2M_ERR_NOMEM;
  }
  c.bind((unsigned char*)m->blob);
  int rc = M2M_OK;
  // the alignment gaps between the packed tensors are part of what m2m_model_checksum covers: they must not be allocator garbage
  if (hipMemsetAsync(m->blob, 0, (size_t)c.off, st) != hipSuccess) { set_error("m2m_model_create: hipMemsetAsync failed"); rc = M2M_ERR_HIP; }
  // the blob is written through the members: `part` is the matrix's place in a declaration that packs several (q | k | v, ck | cv)
  auto at = [&](const void* member, int64_t part = 0) { return (unsigned char*)const_cast<void*>(member) + part * inner * d * (int64_t)es; };
  auto conv = [&](const float* src, void* dst, int64_t n) {
    if (rc == M2M_OK && !src) { set_error("m2m_model_create: null layer weight pointer"); rc = M2M_ERR_INVALID; }
    if (rc == M2M_OK) rc = launch_convert(precision, src, dst, n, st);
  };
  auto copyf = [&](const float* src, const float* dst, int64_t n) {
    if (rc == M2M_OK && !src) { set_error("m2m_model_create: null layer weight pointer"); rc = M2M_ERR_INVALID; }
    if (rc == M2M_OK) rc = launch_copy_f32(src, const_cast<float*>(dst), n, st);
  };
  auto interleave = [&](const float* wi0, const float* wi1, const void* dst, int half) {
    if (rc == M2M_OK && !(wi0 && wi1)) { set_error("m2m_model_create: null wi pointer"); rc = M2M_ERR_INVALID; }
    if (rc == M2M_OK) rc = launch_interleave(precision, wi0, wi1, at(dst), dff, d, half, st);
  };
  for (int l = 0; l < Le && rc == M2M_OK; ++l) {
    const m2m_enc_layer_weights& s = w->enc[l];
    const EncLayerPacked& L = m->enc[l];
    copyf(s.ln0, L.ln0, d); copyf(s.ln1, L.ln1, d);
    conv(s.q, at(L.wqkv, 0), (int64_t)inner * d); conv(s.k, at(L.wqkv, 1), (int64_t)inner * d); conv(s.v, at(L.wqkv, 2), (int64_t)inner * d);
    conv(s.o, at(L.wo), (int64_t)d * inner);
    interleave(s.wi0, s.wi1, L.wi, 32);
    conv(s.wo, at(L.wo_ff), (int64_t)d * dff);
  }
  for (int l = 0; l < Ld && rc == M2M_OK; ++l) {
    const m2m_dec_layer_weights& s = w->dec[l];
    const DecLayerPacked& L = m->dec[l];
    copyf(s.ln0, L.ln0, d); copyf(s.ln1, L.ln1, d); copyf(s.ln2, L.ln2, d);
    conv(s.q, at(L.wqkv, 0), (int64_t)inner * d); conv(s.k, at(L.wqkv, 1), (int64_t)inner * d); conv(s.v, at(L.wqkv, 2), (int64_t)inner * d);
    conv(s.o, at(L.wo), (int64_t)d * inner);
    conv(s.cq, at(L.wcq), (int64_t)inner * d);
    conv(s.co, at(L.wco), (int64_t)d * inner);
    if (rc == M2M_OK) rc = launch_attn_out_image(precision, L.wo, at(L.wo_img), g.num_heads, d, st);   // same stream: behind the conversions
    if (rc == M2M_OK) rc = launch_attn_out_image(precision, L.wco, at(L.wco_img), g.num_heads, d, st);
    interleave(s.wi0, s.wi1, L.wi, 8);
    conv(s.wo, at(L.wo_ff), (int64_t)d * dff);
    if (rc == M2M_OK) rc = launch_ff_image(precision, L.wi, L.wo_ff, at(L.ff_img), dff, d, st);   // same stream: behind the two conversions
    conv(s.ck, at(m->wckv, l * 2 + 0), (int64_t)inner * d); conv(s.cv, at(m->wckv, l * 2 + 1), (int64_t)inner * d);
  }
  copyf(w->enc_final_ln, m->enc_final_ln, d); copyf(w->dec_final_ln, m->dec_final_ln, d);
  copyf(w->shared, m->shared, (int64_t)V * d);
  if (rc == M2M_OK) rc = launch_fill_zero(at(m->lm_head), (int64_t)vocab_pad * d * es, st);
  conv(w->lm_head, at(m->lm_head), (int64_t)V * d);
  if (rc == M2M_OK && tables) rc = launch_token_tables(m, st);      // same stream: behind shared and the layer-0 conversions
  m->enc_rel_bias_host.resize((size_t)g.num_buckets * g.num_heads);
  m->dec_rel_bias_host.resize((size_t)g.num_buckets * g.num_heads);
  hipError_t he = hipSuccess;
  if (rc == M2M_OK) he = hipMemcpyAsync(m->enc_rel_bias_host.data(), w->enc_rel_bias, m->enc_rel_bias_host.size() * 4, hipMemcpyDeviceToHost, st);
  if (rc == M2M_OK && he == hipSuccess) he = hipMemcpyAsync(m->dec_rel_bias_host.data(), w->dec_rel_bias, m->dec_rel_bias_host.size() * 4, hipMemcpyDeviceToHost, st);
  if (rc == M2M_OK && he == hipSuccess) he = hipStreamSynchronize(st);
  if (rc == M2M_OK && he != hipSuccess) { set_error("m2m_model_create: %s", hipGetErrorString(he)); rc = M2M_ERR_HIP; }
  if (rc != M2M_OK) {
    (void)hipFree(m->blob);
    delete m;
    return rc;
  }
  *out = m;
  return M2M_OK;
}

extern "C" void m2m_model_destroy(m2m_model* m) {
  if (!m) return;
  if (m->blob) (void)hipFree(m->blob);
  delete m;
}
extern "C" int m2m_model_precision(const m2m_model* m) { return m ? m->precision : M2M_ERR_INVALID; }
extern "C" int64_t m2m_model_param_bytes(const m2m_model* m) { return m ? m->blob_bytes : (int64_t)M2M_ERR_INVALID; }

extern "C" int m2m_model_checksum(const m2m_model* m, uint64_t* out_host, void* stream) {
  M2M_REQUIRE(m && out_host, "m2m_model_checksum: null argument");
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* acc = nullptr;
  M2M_CHECK_HIP(hipMalloc((void**)&acc, sizeof(unsigned long long)));       // once per run, never on the hot path
  unsigned long long host = 0;
  hipError_t e = hipMemsetAsync(acc, 0, sizeof(unsigned long long), st);
  int rc = M2M_OK;
  if (e == hipSuccess) rc = launch_checksum(m->blob, m->blob_bytes, acc, st);
  if (e == hipSuccess && rc == M2M_OK) e = hipMemcpyAsync(&host, acc, sizeof(host), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && rc == M2M_OK) e = hipStreamSynchronize(st);
  (void)hipFree(acc);
  if (rc != M2M_OK) return rc;
  if (e != hipSuccess) { set_error("m2m_model_checksum: %s", hipGetErrorString(e)); return M2M_ERR_HIP; }
  *out_host = (uint64_t)host;
  return M2M_OK;
}

// ---------------------------------------------------------------- session ---
namespace {
// The session's workspace: every buffer declared once, on its member, in layout order (sizes from s->m and the session's maxima).
void carve_workspace(m2m_session* s, Carver& c) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int B = s->max_batch, S = s->max_enc, L = s->max_dec;
  // the activation buffers serve the encoder (S rows per clip) and the batched teacher-forced decoder pass (L rows)
  const int64_t es = (int64_t)m->esize, M = (int64_t)B * S, Ma = (int64_t)B * (S > L ? S : L), Bp = (int64_t)ceil_div(B, 32) * 32;
  const int64_t Spa = (int64_t)ceil_div(S > L ? S : L, 64) * 64;
  c.take(s->x_enc, Ma * g.d_model * 4);
  c.take(s->h_enc, Ma * g.d_model * es);
  c.take(s->qkv_enc, 3 * Ma * m->inner * es);
  c.take(s->vt_enc, (int64_t)B * m->inner * Spa * es);
  c.take(s->attn_enc, Ma * m->inner * es);
  c.take(s->mid_enc, Ma * g.d_ff * es);
  c.take(s->enc_bias_tab, (int64_t)g.num_heads * (2 * S - 1) * 4);
  c.take(s->dec_bias_tab, (int64_t)g.num_heads * L * 4);
  c.take(s->dec_bias_full_tab, (int64_t)g.num_heads * (2 * L - 1) * 4);
  c.take(s->cross_vt, (int64_t)B * m->inner * (ceil_div(S, 64) * 64) * es);
  c.take(s->cross_kv, (int64_t)g.num_decoder_layers * 2 * M * m->inner * es);
  c.take(s->self_k, (int64_t)g.num_decoder_layers * B * m->inner * L * es);
  c.take(s->self_v, (int64_t)g.num_decoder_layers * B * m->inner * L * es);
  c.take(s->x_dec, 3 * Bp * g.d_model * 8);   // int64 fixed-point residual stream, 3 rotating buffers
  c.take(s->logits, Bp * m->vocab_pad * 4);
  c.take(s->tokens, (int64_t)B * L * 8);
  c.take(s->finished, (int64_t)B * 4);
  c.take(s->tok_row, (int64_t)B * 4);
  c.take(s->keys, (int64_t)B * 8);
  c.take(s->states, sizeof(DecState) * MAX_GROUPS);
  c.take(s->forced_ids, (int64_t)B * L * 8);
  c.take(s->sample_dev, sizeof(SampleParams));
  c.take(s->proc_dev, sizeof(ProcessParams));
  c.take(s->beam_dev, sizeof(BeamParams));
  c.take(s->beam_clip, (int64_t)B * sizeof(BeamClip));
  c.take(s->beam_row, (int64_t)B * sizeof(BeamRow));
  c.take(s->anc, 2 * (int64_t)B * L);
  c.take(s->hyp_tok, (int64_t)B * L * 8);
  c.take(s->score_dev, sizeof(ScoreParams));
  c.take(s->gram_dev, sizeof(GrammarParams));
  c.take(s->gram_state, (int64_t)B * sizeof(GrammarState));
}

// a switch outside its range refuses the session
int check_switches(const SessionSwitches& sw) {
  M2M_REQUIRE(sw.attn_clips == 0 || sw.attn_clips == 1 || sw.attn_clips == 2 || sw.attn_clips == 4,
              "M2M_DA_CLIPS=%d: clips per decode-attention workgroup must be 0 (by chain size), 1, 2 or 4", sw.attn_clips);
  M2M_REQUIRE(sw.ff_rows == 0 || sw.ff_rows == 8 || sw.ff_rows == 16,
              "M2M_DEC_FF_ROWS=%d: rows per decode feed-forward workgroup must be 0 (by chain size), 8 or 16", sw.ff_rows);
  M2M_REQUIRE(sw.ff_slices == 0 || sw.ff_slices == 1 || sw.ff_slices == 2 || sw.ff_slices == 4,
              "M2M_DEC_FF_SLICES=%d: hidden slices per decode feed-forward workgroup must be 0 (by chain size), 1, 2 or 4", sw.ff_slices);
  M2M_REQUIRE(sw.mc_cif == 1 || sw.mc_cif == 2,
              "M2M_MC_CIF=%d: clips in flight in the multi-clip cross-attention must be 0 (default: 1), 1 or 2", sw.mc_cif);
  M2M_REQUIRE(sw.token_tables >= 0 && sw.token_tables <= 2,
              "M2M_DEC_TOKEN_TABLES=%d: the layer-0 token-table form must be 0 (off), 1 (this step's q, k, v) or 2 (and the cached K/V)", sw.token_tables);
  return M2M_OK;
}

// relative-position bias tables (fp32), built on the host from the bucket function, and how far out each becomes constant
hipError_t upload_bias_tables(m2m_session* s) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int H = g.num_heads, S = s->max_enc, L = s->max_dec;
  std::vector<float> et((size_t)H * (2 * S - 1)), dt((size_t)H * L);
  for (int rel = -(S - 1); rel <= S - 1; ++rel) {
    const int bk = m2m_rel_bucket(rel, 1, g.num_buckets, g.max_distance);
    for (int h = 0; h < H; ++h) et[(size_t)h * (2 * S - 1) + rel + S - 1] = m->enc_rel_bias_host[(size_t)bk * H + h];
  }
  for (int n = 0; n < L; ++n) {
    const int bk = m2m_rel_bucket(-n, 0, g.num_buckets, g.max_distance);
    for (int h = 0; h < H; ++h) dt[(size_t)h * L + n] = m->dec_rel_bias_host[(size_t)bk * H + h];
  }
  // distance from which on a table holds one value per side (the last bucket): the smallest D with bucket(-n) == bucket(-(len - 1))
  // and bucket(+n) == bucket(len - 1) for every n >= D; 0 if the table is too short to get there
  auto far_of = [&](int len, int bidir) {
    int d = len - 1;
    while (d > 0 && m2m_rel_bucket(-(d - 1), bidir, g.num_buckets, g.max_distance) == m2m_rel_bucket(-(len - 1), bidir, g.num_buckets, g.max_distance) &&
           m2m_rel_bucket(d - 1, bidir, g.num_buckets, g.max_distance) == m2m_rel_bucket(len - 1, bidir, g.num_buckets, g.max_distance)) --d;
    return d >= len - 1 ? 0 : d;
  };
  s->enc_bias_far = far_of(S, 1);
  s->dec_bias_far = far_of(L, 0);      // (the future half of the causal table is masked, never read by a wide step)
  // the same decoder bias as a (key - query) table for the batched causal pass: entry L-1-n = bias(n), n = q - k >= 0;
  // the upper half (future keys) is masked by the kernel and stays 0
  std::vector<float> df((size_t)H * (2 * L - 1), 0.f);
  for (int h = 0; h < H; ++h)
    for (int n = 0; n < L; ++n) df[(size_t)h * (2 * L - 1) + (L - 1 - n)] = dt[(size_t)h * L + n];
  hipError_t e = hipMemcpy(s->enc_bias_tab, et.data(), et.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->dec_bias_tab, dt.data(), dt.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(s->dec_bias_full_tab, df.data(), df.size() * 4, hipMemcpyHostToDevice);
  return e;
}
}  // namespace

extern "C" int64_t m2m_session_workspace_bytes(const m2m_model* m, int max_batch, int max_enc_len, int max_dec_len) {
  if (!m || max_batch < 1 || max_enc_len < 1 || max_dec_len < 1) {
    set_error("m2m_session_workspace_bytes: bad argument");
    return M2M_ERR_INVALID;
  }
  m2m_session scratch;                     // sized, never bound (no size depends on a switch)
  scratch.m = m; scratch.max_batch = max_batch; scratch.max_enc = max_enc_len; scratch.max_dec = max_dec_len;
  Carver c;
  carve_workspace(&scratch, c);
  return c.off;
}

// check, latch, carve, bias tables, streams
extern "C" int m2m_session_create(const m2m_model* m, int max_batch, int max_enc_len, int max_dec_len,
                                  void* workspace_dev, int64_t workspace_bytes, m2m_session** out) {
  M2M_REQUIRE(m && workspace_dev && out, "m2m_session_create: null argument");
  M2M_REQUIRE(max_batch >= 1 && max_enc_len >= 1 && max_dec_len >= 1, "m2m_session_create: bad geometry");
  M2M_REQUIRE(((uintptr_t)workspace_dev & 255) == 0, "m2m_session_create: workspace must be 256-byte aligned");
  // the switches are read ONCE per session, here, by the construction of its SessionSwitches; a refusal below frees the session
  std::unique_ptr<m2m_session, void (*)(m2m_session*)> s(new m2m_session(), m2m_session_destroy);
  s->m = m; s->max_batch = max_batch; s->max_enc = max_enc_len; s->max_dec = max_dec_len;
  s->ws = (unsigned char*)workspace_dev; s->ws_bytes = workspace_bytes;
  Carver c;
  carve_workspace(s.get(), c);
  if (workspace_bytes < c.off) {
    set_error("m2m_session_create: workspace %lld bytes < required %lld", (long long)workspace_bytes, (long long)c.off);
    return M2M_ERR_NOMEM;
  }
  M2M_REQUIRE((size_t)(2 * max_enc_len - 1) * 4 + 40 * 1024 <= 150 * 1024,
              "m2m_session_create: max_enc_len=%d too long (attention bias table must fit LDS)", max_enc_len);
  M2M_REQUIRE((size_t)max_enc_len * 4 <= 60 * 1024 && (size_t)max_dec_len * 4 <= 60 * 1024,
              "m2m_session_create: sequence too long for the decode attention score buffer");
  if (const int rc = check_switches(s->sw)) return rc;
  c.bind(s->ws);

  hipError_t e = upload_bias_tables(s.get());
  if (e == hipSuccess) e = hipMemset(s->states, 0, sizeof(DecState) * MAX_GROUPS);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc((void**)&s->call_host, sizeof(CallParams), hipHostMallocDefault);
  if (e == hipSuccess) s->call_host->gram = GrammarParams{};
  if (e == hipSuccess) e = hipHostMalloc((void**)&s->fin_host, (size_t)max_batch * sizeof(int), hipHostMallocDefault);
  for (int i = 0; i < MAX_GROUPS && e == hipSuccess; ++i) {
    DecGroup& gr = s->groups[i];
    gr.view.state = s->states + i;
    e = hipStreamCreateWithFlags(&gr.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&gr.ev_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipHostMalloc((void**)&gr.state_host, sizeof(DecState), hipHostMallocDefault);
  }
  if (e != hipSuccess) {
    set_error("m2m_session_create: %s", hipGetErrorString(e));
    return M2M_ERR_HIP;
  }
  *out = s.release();
  return M2M_OK;
}

extern "C" void m2m_session_destroy(m2m_session* s) {
  if (!s) return;
  for (int i = 0; i < MAX_GROUPS; ++i) {
    DecGroup& gr = s->groups[i];
    for (auto& ge : gr.graphs) {
      if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
      if (ge.graph) (void)hipGraphDestroy(ge.graph);
    }
    gr.graphs.clear();
    if (gr.ev_done) (void)hipEventDestroy(gr.ev_done);
    if (gr.stream) (void)hipStreamDestroy(gr.stream);
    if (gr.state_host) (void)hipHostFree(gr.state_host);
  }
  if (s->ev_in) (void)hipEventDestroy(s->ev_in);
  if (s->call_host) (void)hipHostFree(s->call_host);
  if (s->fin_host) (void)hipHostFree(s->fin_host);
  delete s;
}

// --------------------------------------------------------- batched layers ---
// One batched pass over the session's activation buffers: the encoder (S rows per clip) or the teacher-forced decoder pass (Ld rows).
// The sub-layers below are what the two passes share; each reads and updates the fp32 residual stream x_enc in place.
namespace {
struct BatchedPass {
  m2m_session* s;
  int P;            // precision
  int B, rows;      // clips, rows per clip
  int Sp;           // rows rounded up to the 64-key tile (row pitch of the transposed V)
  hipStream_t st;
  int M() const { return B * rows; }
};

// x_enc += A . W^T, A [M, K]
int resid_proj(const BatchedPass& p, const void* A, const void* W, int K) {
  const int d = p.s->m->g.d_model;
  GemmArgs a{}; a.vt_which = -1;
  a.A = A; a.W = W; a.M = p.M(); a.N = d; a.K = K; a.out = p.s->x_enc; a.ldo = d;
  return launch_gemm(p.P, EPI_RESID, a, p.st);
}

// RMSNorm + QKV projection into heads (V transposed), flash attention under the pass's bias table, output projection into the residual
int self_attn_sublayer(const BatchedPass& p, const float* ln, const void* wqkv, const void* wo, const float* bias_tab, int tab_len,
                       int bias_far, bool causal) {
  m2m_session* s = p.s;
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  int rc;
  // RMSNorm + QKV projection: one kernel in the bf16 mode (launch_norm_gemm), norm into h_enc + GEMM otherwise
  GemmArgs a{};
  a.A = s->h_enc; a.W = wqkv; a.M = p.M(); a.N = 3 * m->inner; a.K = g.d_model; a.out = s->qkv_enc;
  a.Bsz = p.B; a.S = p.rows; a.H = g.num_heads; a.inner = m->inner;
  a.vt_which = 2; a.vt_out = s->vt_enc; a.Sp = p.Sp;
  a.nx = s->x_enc; a.nw = ln; a.neps = g.layer_norm_eps;
  if ((rc = launch_norm_gemm(p.P, EPI_HEADS, a, p.st))) return rc;
  AttnArgs at{};
  at.Q = s->qkv_enc; at.K = (const unsigned char*)s->qkv_enc + (size_t)p.M() * m->inner * m->esize; at.Vt = s->vt_enc; at.Sp = p.Sp;
  at.bias_tab = bias_tab; at.tab_stride = 2 * tab_len - 1; at.tab_center = tab_len - 1; at.bias_far = bias_far;
  at.out = s->attn_enc; at.B = p.B; at.H = g.num_heads; at.Sq = p.rows; at.Sk = p.rows;
  if ((rc = launch_attn(p.P, at, causal, p.st))) return rc;
  return resid_proj(p, s->attn_enc, wo, m->inner);
}

// RMSNorm + gated wi (epi: EPI_GATED for the encoder's 64-row interleave of wi, EPI_GATED16 for the decoder's 16-row one), wo_ff into the residual
int feed_fwd_sublayer(const BatchedPass& p, const float* ln, const void* wi, const void* wo_ff, int epi) {
  m2m_session* s = p.s;
  const m2m_t5_geometry& g = s->m->g;
  GemmArgs a{}; a.vt_which = -1;
  a.A = s->h_enc; a.W = wi; a.M = p.M(); a.N = 2 * g.d_ff; a.K = g.d_model; a.out = s->mid_enc; a.ldo = g.d_ff;
  a.nx = s->x_enc; a.nw = ln; a.neps = g.layer_norm_eps;
  if (const int rc = launch_norm_gemm(p.P, epi, a, p.st)) return rc;
  return resid_proj(p, s->mid_enc, wo_ff, g.d_ff);
}

// decoder pass: cross-attention of layer l over the cached encoder K/V (V transposed here, once per layer)
int cross_attn_sublayer(const BatchedPass& p, const DecLayerPacked& L, int l) {
  m2m_session* s = p.s;
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int H = g.num_heads, S = s->S, Sp = ceil_div(S, 64) * 64;
  const size_t per_enc = (size_t)s->B * H * S * DK;                       // elements of one cross K (or V) block
  int rc;
  GemmArgs a{};
  a.A = s->h_enc; a.W = L.wcq; a.M = p.M(); a.N = m->inner; a.K = g.d_model; a.out = s->qkv_enc;
  a.Bsz = p.B; a.S = p.rows; a.H = H; a.inner = m->inner; a.vt_which = -1;
  a.nx = s->x_enc; a.nw = L.ln1; a.neps = g.layer_norm_eps;
  if ((rc = launch_norm_gemm(p.P, EPI_HEADS, a, p.st))) return rc;
  const unsigned char* ck = (const unsigned char*)s->cross_kv + ((size_t)l * 2 + 0) * per_enc * m->esize;
  const unsigned char* cv = (const unsigned char*)s->cross_kv + ((size_t)l * 2 + 1) * per_enc * m->esize;
  if ((rc = launch_transpose_v(p.P, cv, s->cross_vt, p.B * H, S, Sp, p.st))) return rc;
  AttnArgs at{};
  at.Q = s->qkv_enc; at.K = ck; at.Vt = s->cross_vt; at.Sp = Sp; at.bias_tab = nullptr;
  at.out = s->attn_enc; at.B = p.B; at.H = H; at.Sq = p.rows; at.Sk = S;
  if ((rc = launch_attn(p.P, at, false, p.st))) return rc;
  return resid_proj(p, s->attn_enc, L.wco, m->inner);
}
}  // namespace

// ----------------------------------------------------------------- encode ---
extern "C" int m2m_encode(m2m_session* s, const float* inputs_embeds_dev, int B, int S, float* enc_out_dev, void* stream) {
  M2M_REQUIRE(s && inputs_embeds_dev, "m2m_encode: null argument");
  M2M_REQUIRE(B >= 1 && B <= s->max_batch, "m2m_encode: batch %d exceeds session max_batch %d", B, s->max_batch);
  M2M_REQUIRE(S >= 1 && S <= s->max_enc, "m2m_encode: S=%d exceeds session max_enc_len %d", S, s->max_enc);
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int P = m->precision;
  hipStream_t st = (hipStream_t)stream;
  const int M = B * S, d = g.d_model;
  const EncSwitchScope sw_scope(&s->sw.enc);
  s->encoded = false;
  M2M_CHECK_HIP(hipMemcpyAsync(s->x_enc, inputs_embeds_dev, (size_t)M * d * 4, hipMemcpyDeviceToDevice, st));
  int rc;
  const BatchedPass p{s, P, B, S, ceil_div(S, 64) * 64, st};
  for (const EncLayerPacked& L : m->enc) {
    if ((rc = self_attn_sublayer(p, L.ln0, L.wqkv, L.wo, s->enc_bias_tab, s->max_enc, s->enc_bias_far, false))) return rc;
    if ((rc = feed_fwd_sublayer(p, L.ln1, L.wi, L.wo_ff, EPI_GATED))) return rc;
  }
  // final norm -> GEMM input (T) and, if asked, the fp32 encoder states
  // cross-attention K/V of every decoder layer in one GEMM, written in decode layout
  GemmArgs a{};
  a.vt_which = -1;
  a.A = s->h_enc; a.W = m->wckv; a.M = M; a.N = g.num_decoder_layers * 2 * m->inner; a.K = d; a.out = s->cross_kv;
  a.Bsz = B; a.S = S; a.H = g.num_heads; a.inner = m->inner;
  if (enc_out_dev) {        // the caller wants the fp32 encoder states too: the norm runs as its own kernel (both outputs), then the product
    if ((rc = launch_final_norm_f32(s->x_enc, m->enc_final_ln, enc_out_dev, s->h_enc, P, M, d, g.layer_norm_eps, st))) return rc;
    if ((rc = launch_gemm(P, EPI_HEADS, a, st))) return rc;
  } else {                  // generate(): the final norm is the cross-K/V product's own prologue
    a.nx = s->x_enc; a.nw = m->enc_final_ln; a.neps = g.layer_norm_eps;
    if ((rc = launch_norm_gemm(P, EPI_HEADS, a, st))) return rc;
  }
  s->B = B; s->S = S; s->encoded = true;
  return M2M_OK;
}

// ----------------------------------------------------------------- decode ---
// The switches tests and A/B runs flip between two calls on one session: read once at the top of a decode call, never inside it.
struct DecodeSwitches {
  int group_rows = env_int("M2M_GROUP_ROWS", 0);                       // clips per chain (0: plan_groups decides)
  bool graph = env_int("M2M_NO_GRAPH", 0) != 1;                        // 1: every step launched directly
  int graph_steps = std::max(1, env_int("M2M_GRAPH_STEPS", 8));        // decode steps per graph
  bool compact = env_int("M2M_COMPACT", 1) != 0;                       // 0: no live-row re-packing
  bool lookahead = env_int("M2M_POLL_LOOKAHEAD", 1) != 0;              // 0: every host poll drains the chains before the next launch
};

// Split the B encoded clips into independent chains: M2M_GROUP_ROWS clips per chain (default 32:
// one 32-row MFMA tile of clips per chain), at most MAX_GROUPS chains.  Measured at B = 32 on
// MI355X: 1 chain 322 ms, 2 chains 315 ms, 4 chains 666 ms (dispatch-bound) - see DESIGN_HISTORY.md 4.4.
static int plan_groups(m2m_session* s, int rows_env, int rows = -1) {       // rows_env: DecodeSwitches::group_rows; rows: the packed slots to decode (default: the whole encoded batch)
  // Default: TWO chains once there are enough clips to split (B >= 24), one otherwise.  Two graph chains on two
  // streams overlap one chain's latency phases (prologue, merge tail, feed-forward, lm_head / head) with the other's
  // K/V stream: B = 32 -> 2 x 16 clips is +3.7 % over one chain of 32 (tools/chain_sweep.py); more than two chains do
  // not help (the dependent-dispatch rate of the command processor becomes the limit: 4 x 8 = 1 x 32, 8 x 4 is 4x slower).
  const int nrows = rows < 0 ? s->B : rows;
  int G = rows_env > 0 ? ceil_div(nrows, rows_env) : (nrows >= 24 ? 2 : 1);
  if (G < 1) G = 1;
  if (G > MAX_GROUPS) G = MAX_GROUPS;
  // beam search: a clip's beams share a chain (the beam head ranks them together), so chains split at multiples of beam_nb
  const int unit = s->beam_nb > 0 ? s->beam_nb : 1, units = nrows / unit;
  if (G > units) G = units;
  const int base = units / G, extra = units % G;
  int b0 = 0;
  for (int i = 0; i < G; ++i) {
    s->groups[i].view.b0 = b0;
    s->groups[i].view.nb = (base + (i < extra ? 1 : 0)) * unit;
    s->groups[i].view.ord = i; s->groups[i].view.count = G;
    b0 += s->groups[i].view.nb;
  }
  return G;
}

// One graph = `steps` consecutive decode steps of one chain (kernels read the step index from
// device memory, so the same graph replays for every position; steps past the end are no-ops).
static int ensure_graph(m2m_session* s, DecGroup& gr, int steps) {
  const int key[11] = {s->B, s->S, gr.view.b0, gr.view.nb, steps, s->sw.finished_skip ? 1 : 0, s->head_mode, s->beam_nb,
                       gr.view.ord, gr.view.count,        // (ord, count): which cross-K/V layers the chain keeps resident (t5.h)
                       s->sw.token_tables};
  ++gr.graph_clock;
  for (auto& ge : gr.graphs)
    if (memcmp(key, ge.key, sizeof(key)) == 0) { ge.used = gr.graph_clock; gr.graph_exec = ge.exec; return M2M_OK; }
  constexpr size_t MAX_CACHED = 12;
  if (gr.graphs.size() >= MAX_CACHED) {                      // evict the least recently used entry
    size_t lru = 0;
    for (size_t i = 1; i < gr.graphs.size(); ++i) if (gr.graphs[i].used < gr.graphs[lru].used) lru = i;
    (void)hipGraphExecDestroy(gr.graphs[lru].exec);
    (void)hipGraphDestroy(gr.graphs[lru].graph);
    gr.graphs.erase(gr.graphs.begin() + (long)lru);
  }
  gr.graph_exec = nullptr;
  M2M_CHECK_HIP(hipStreamBeginCapture(gr.stream, hipStreamCaptureModeThreadLocal));
  int rc = M2M_OK;
  for (int i = 0; i < steps && rc == M2M_OK; ++i) rc = decode_launch_step(s, gr.view, false, nullptr, 0, gr.stream);
  hipGraph_t gph = nullptr;
  hipError_t e = hipStreamEndCapture(gr.stream, &gph);
  if (rc != M2M_OK) { if (gph) (void)hipGraphDestroy(gph); return rc; }
  if (e != hipSuccess) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return M2M_ERR_HIP; }
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, gph, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(gph); set_error("hipGraphInstantiate: %s", hipGetErrorString(e)); return M2M_ERR_HIP; }
  DecGroup::GraphEntry ge{};
  memcpy(ge.key, key, sizeof(key));
  ge.graph = gph; ge.exec = ex; ge.used = gr.graph_clock;
  gr.graphs.push_back(ge);
  gr.graph_exec = ex;
  return M2M_OK;
}

// Nothing of a failed call may still be running when it returns: the caller owns the workspace and may free or
// regrow it at once.  Errors are rare, so the blanket synchronisation of every chain stream costs nothing.
static void quiesce(m2m_session* s, hipStream_t caller) {
  for (int i = 0; i < MAX_GROUPS; ++i)
    if (s->groups[i].stream) (void)hipStreamSynchronize(s->groups[i].stream);
  (void)hipStreamSynchronize(caller);
  (void)hipGetLastError();
}

// One call of a decode export.  Beam search (HEAD_BEAM) decodes the B encoded clips as B x beam_nb rows and never re-packs them;
// the other heads decode B rows.
namespace {
struct DecodeCall {
  const char* fn;          // the export, for messages
  int head_mode, beam_nb;  // the session's head form for this call
  int64_t* tokens_out;
  float* scores_out;       // beam search: optional sequence scores
  const GrammarParams* gram = nullptr;   // processed and scored heads: the token grammar of this call, nullptr without one
};
}  // namespace

static int decode_call(m2m_session* s, const DecodeCall& c, int max_length, int* out_len_host, hipStream_t caller);

// M2M_ERR_STATE unless the session holds an encode: never encoded, or the last greedy decode re-packed its live rows over it
static int require_encoded(const m2m_session* s, const char* fn) {
  if (s->encoded) return M2M_OK;
  set_error("%s: %s", fn, s->rows_moved > 0 ? "re-encode: the last m2m_generate_greedy re-packed its live rows over the encoded state (it "
                                              "consumes the encode whenever m2m_session_repack_stats reports rows moved)"
                                            : "call m2m_encode first");
  return M2M_ERR_STATE;
}

// the sampling parameters (m2m_generate_sample, m2m_generate_processed), checked and laid out into the SampleParams block on the host
static int fill_sample_params(const m2m_sample_params* p, SampleParams& h, const char* fn) {
  M2M_REQUIRE(isfinite(p->temperature) && p->temperature > 0.f, "%s: temperature must be a strictly positive finite float, got %g", fn,
              (double)p->temperature);
  M2M_REQUIRE(p->top_k >= 0, "%s: top_k must be >= 0 (0 disables the filter), got %d", fn, p->top_k);
  M2M_REQUIRE(p->top_p >= 0.f && p->top_p <= 1.f, "%s: top_p must be a float in [0, 1], got %g", fn, (double)p->top_p);
  h.temperature = p->temperature; h.top_k = p->top_k; h.top_p = p->top_p; h.pad_ = 0; h.seed = (unsigned long long)p->seed;
  return M2M_OK;
}

extern "C" int m2m_generate_greedy(m2m_session* s, int max_length, int64_t* tokens_out_dev, int* out_len_host, void* stream) {
  const char* fn = "m2m_generate_greedy";
  M2M_REQUIRE(s && tokens_out_dev && out_len_host, "m2m_generate_greedy: null argument");
  int rc;
  if ((rc = require_encoded(s, fn))) return rc;
  M2M_REQUIRE(max_length >= 1 && max_length <= s->max_dec, "m2m_generate_greedy: max_length %d outside [1, %d]", max_length, s->max_dec);
  return decode_call(s, {fn, HEAD_GREEDY, 0, tokens_out_dev, nullptr}, max_length, out_len_host, (hipStream_t)stream);
}

extern "C" int m2m_generate_sample(m2m_session* s, int max_length, const m2m_sample_params* p, int64_t* tokens_out_dev,
                                   int* out_len_host, void* stream) {
  const char* fn = "m2m_generate_sample";
  M2M_REQUIRE(s && p && tokens_out_dev && out_len_host, "m2m_generate_sample: null argument");
  int rc;
  if ((rc = fill_sample_params(p, s->call_host->sample, fn))) return rc;
  M2M_REQUIRE(s->m->g.vocab_size <= SAMPLE_MAX_VOCAB, "m2m_generate_sample: vocab_size %d > %d (the sampling head keeps a row in one "
              "wavefront's registers)", s->m->g.vocab_size, SAMPLE_MAX_VOCAB);
  if ((rc = require_encoded(s, fn))) return rc;
  M2M_REQUIRE(max_length >= 1 && max_length <= s->max_dec, "m2m_generate_sample: max_length %d outside [1, %d]", max_length, s->max_dec);
  return decode_call(s, {fn, HEAD_SAMPLE, 0, tokens_out_dev, nullptr}, max_length, out_len_host, (hipStream_t)stream);
}

// Logits processors (include/music2midi_amd.h): the id lists are checked and laid out into the ProcessParams block on the host; the
// decode loop runs the processed head (HEAD_PROCESSED, greedy or sampling select).
static int fill_process_params(const m2m_session* s, int max_length, const m2m_process_params* p, ProcessParams& h,
                               const char* fn = "m2m_generate_processed") {
  const m2m_t5_geometry& g = s->m->g;
  const int V = g.vocab_size;
  M2M_REQUIRE(V <= PROC_MAX_VOCAB, "%s: vocab_size %d > %d (the processed head keeps a row in one wavefront's registers)", fn, V,
              PROC_MAX_VOCAB);
  M2M_REQUIRE(max_length <= PROC_MAX_LEN, "%s: max_length %d > %d (a row's history is staged in LDS)", fn, max_length, PROC_MAX_LEN);
  M2M_REQUIRE(isfinite(p->repetition_penalty) && p->repetition_penalty > 0.f,
              "%s: repetition_penalty must be a strictly positive finite float, got %g", fn, (double)p->repetition_penalty);
  M2M_REQUIRE(p->no_repeat_ngram_size >= 0, "%s: no_repeat_ngram_size must be >= 0, got %d", fn, p->no_repeat_ngram_size);
  M2M_REQUIRE(p->min_length >= 0, "%s: min_length must be >= 0, got %d", fn, p->min_length);
  M2M_REQUIRE(p->min_new_tokens >= 0, "%s: min_new_tokens must be >= 0, got %d", fn, p->min_new_tokens);
  M2M_REQUIRE(p->forced_bos_token_id >= -1 && p->forced_bos_token_id < V, "%s: forced_bos_token_id %d outside [-1, %d)", fn,
              p->forced_bos_token_id, V);
  M2M_REQUIRE(p->forced_eos_token_id >= -1 && p->forced_eos_token_id < V, "%s: forced_eos_token_id %d outside [-1, %d)", fn,
              p->forced_eos_token_id, V);
  M2M_REQUIRE(p->n_suppress_tokens >= 0 && (p->n_suppress_tokens == 0 || p->suppress_tokens), "%s: bad suppress_tokens list", fn);
  M2M_REQUIRE(p->n_begin_suppress_tokens >= 0 && (p->n_begin_suppress_tokens == 0 || p->begin_suppress_tokens),
              "%s: bad begin_suppress_tokens list", fn);
  M2M_REQUIRE(p->n_bad_words >= 0 && (p->n_bad_words == 0 || (p->bad_words_ids && p->bad_words_lengths)), "%s: bad bad_words list", fn);
  h = ProcessParams{};
  h.penalty = p->repetition_penalty; h.ngram = p->no_repeat_ngram_size; h.min_length = p->min_length; h.min_new = p->min_new_tokens;
  h.forced_bos = p->forced_bos_token_id; h.forced_eos = p->forced_eos_token_id;
  h.begin_index = p->forced_bos_token_id >= 0 ? 2 : 1;   // 4.34: input_ids_seq_length (1), + 1 with forced_bos_token_id
  h.max_length = max_length;
  for (int i = 0; i < p->n_suppress_tokens; ++i) {
    const int v = p->suppress_tokens[i];
    M2M_REQUIRE(v >= 0 && v < V, "%s: suppress_tokens id %d outside [0, %d)", fn, v, V);
    h.supp[v >> 5] |= 1u << (v & 31); h.has_supp = 1;
  }
  for (int i = 0; i < p->n_begin_suppress_tokens; ++i) {
    const int v = p->begin_suppress_tokens[i];
    M2M_REQUIRE(v >= 0 && v < V, "%s: begin_suppress_tokens id %d outside [0, %d)", fn, v, V);
    h.begin[v >> 5] |= 1u << (v & 31); h.has_begin = 1;
  }
  int64_t off = 0;
  for (int q = 0; q < p->n_bad_words; ++q) {
    const int L = p->bad_words_lengths[q];
    M2M_REQUIRE(L >= 1 && L <= PROC_MAX_BAD_IDS, "%s: bad_words sequence %d has length %d (1 .. %d)", fn, q, L, PROC_MAX_BAD_IDS);
    const int32_t* ids = p->bad_words_ids + off;
    off += L;
    for (int k = 0; k < L; ++k) M2M_REQUIRE(ids[k] >= 0 && ids[k] < V, "%s: bad_words id %d outside [0, %d)", fn, ids[k], V);
    if (L == 1) {
      if (ids[0] == g.eos_token_id) continue;               // 4.34 filters the sequence [eos] out
      h.bad1[ids[0] >> 5] |= 1u << (ids[0] & 31); h.has_bad1 = 1;
      continue;
    }
    M2M_REQUIRE(h.n_bad < PROC_MAX_BAD, "%s: more than %d bad_words sequences of two or more ids", fn, PROC_MAX_BAD);
    const int o = h.bad_off[h.n_bad];
    M2M_REQUIRE(o + L <= PROC_MAX_BAD_IDS, "%s: bad_words sequences of two or more ids hold more than %d ids", fn, PROC_MAX_BAD_IDS);
    for (int k = 0; k < L; ++k) h.bad_ids[o + k] = ids[k];
    h.bad_off[++h.n_bad] = o + L;
  }
  return M2M_OK;
}

static int generate_processed(m2m_session* s, int max_length, const m2m_process_params* proc, const m2m_sample_params* sample,
                              int64_t* tokens_out_dev, int* out_len_host, void* stream, const GrammarParams* gram, const char* fn) {
  M2M_REQUIRE(s && proc && tokens_out_dev && out_len_host, "%s: null argument", fn);
  int rc;
  if (sample && (rc = fill_sample_params(sample, s->call_host->sample, fn))) return rc;
  M2M_REQUIRE(max_length >= 1 && max_length <= s->max_dec, "%s: max_length %d outside [1, %d]", fn, max_length, s->max_dec);
  if ((rc = fill_process_params(s, max_length, proc, s->call_host->proc, fn))) return rc;
  if ((rc = require_encoded(s, fn))) return rc;
  return decode_call(s, {fn, HEAD_PROCESSED | (sample ? HEAD_SAMPLE : HEAD_GREEDY), 0, tokens_out_dev, nullptr, gram}, max_length,
                     out_len_host, (hipStream_t)stream);
}

extern "C" int m2m_generate_processed(m2m_session* s, int max_length, const m2m_process_params* proc, const m2m_sample_params* sample,
                                      int64_t* tokens_out_dev, int* out_len_host, void* stream) {
  return generate_processed(s, max_length, proc, sample, tokens_out_dev, out_len_host, stream, nullptr, "m2m_generate_processed");
}

// Per-token outputs (include/music2midi_amd.h): the processed head's scored form (HEAD_SCORED, greedy or sampling select), with a
// neutral ProcessParams block when the call has no processor; with no output asked for, the matching unscored export.
static int generate_scored(m2m_session* s, int max_length, const m2m_process_params* proc, const m2m_sample_params* sample,
                           int64_t* tokens_out_dev, float* scores_out_dev, float* logprobs_out_dev, int* out_len_host, void* stream,
                           const GrammarParams* gram, const char* fn) {
  M2M_REQUIRE(s && tokens_out_dev && out_len_host, "%s: null argument", fn);
  if (!scores_out_dev && !logprobs_out_dev) {        // (never with a grammar: m2m_generate_grammar takes the processed head then)
    if (proc) return m2m_generate_processed(s, max_length, proc, sample, tokens_out_dev, out_len_host, stream);
    if (sample) return m2m_generate_sample(s, max_length, sample, tokens_out_dev, out_len_host, stream);
    return m2m_generate_greedy(s, max_length, tokens_out_dev, out_len_host, stream);
  }
  int rc;
  if (sample && (rc = fill_sample_params(sample, s->call_host->sample, fn))) return rc;
  const int V = s->m->g.vocab_size;
  M2M_REQUIRE(V <= PROC_MAX_VOCAB, "%s: vocab_size %d > %d (the scored head keeps a row in one wavefront's registers)", fn, V,
              PROC_MAX_VOCAB);
  M2M_REQUIRE(max_length >= 1 && max_length <= s->max_dec, "%s: max_length %d outside [1, %d]", fn, max_length, s->max_dec);
  if (proc) {
    if ((rc = fill_process_params(s, max_length, proc, s->call_host->proc, fn))) return rc;
  } else {                                   // no processor: the neutral block (nothing banned, nothing forced)
    ProcessParams& h = s->call_host->proc;
    h = ProcessParams{};
    h.penalty = 1.0f; h.forced_bos = -1; h.forced_eos = -1; h.begin_index = 1; h.max_length = max_length;
  }
  if ((rc = require_encoded(s, fn))) return rc;
  ScoreParams& sc = s->call_host->score;
  sc = ScoreParams{};
  sc.scores = scores_out_dev; sc.logprobs = logprobs_out_dev; sc.rows = s->B; sc.steps = max_length - 1;
  sc.vec4 = (V % 4 == 0 && ((uintptr_t)scores_out_dev & 15) == 0) ? 1 : 0;
  return decode_call(s, {fn, HEAD_SCORED | HEAD_PROCESSED | (sample ? HEAD_SAMPLE : HEAD_GREEDY), 0, tokens_out_dev, nullptr, gram},
                     max_length, out_len_host, (hipStream_t)stream);
}

extern "C" int m2m_generate_scored(m2m_session* s, int max_length, const m2m_process_params* proc, const m2m_sample_params* sample,
                                   int64_t* tokens_out_dev, float* scores_out_dev, float* logprobs_out_dev, int* out_len_host,
                                   void* stream) {
  return generate_scored(s, max_length, proc, sample, tokens_out_dev, scores_out_dev, logprobs_out_dev, out_len_host, stream, nullptr,
                         "m2m_generate_scored");
}

// the call's grammar block (m2m_generate_grammar, m2m_generate_beam_processed), checked against the model and laid out for the device
static int fill_grammar_params(const m2m_session* s, int max_length, const m2m_grammar_params* grammar, GrammarParams& gp, const char* fn) {
  const m2m_t5_geometry& g = s->m->g;
  const int V = g.vocab_size;
  M2M_REQUIRE(V <= PROC_MAX_VOCAB, "%s: vocab_size %d > %d (the processed head keeps a row in one wavefront's registers)", fn, V, PROC_MAX_VOCAB);
  M2M_REQUIRE(max_length <= PROC_MAX_LEN, "%s: max_length %d > %d", fn, max_length, PROC_MAX_LEN);
  M2M_REQUIRE(grammar->pitch_offset > GRAM_OFFSET && grammar->pitch_offset <= V, "%s: pitch_offset %d outside [%d, %d]", fn,
              grammar->pitch_offset, GRAM_OFFSET + 1, V);
  M2M_REQUIRE(grammar->n_pitch >= 1 && grammar->n_pitch <= GRAM_MAX_PITCH, "%s: n_pitch %d outside [1, %d]", fn, grammar->n_pitch,
              GRAM_MAX_PITCH);
  M2M_REQUIRE(grammar->n_time >= 1 && grammar->n_time <= V, "%s: n_time %d outside [1, %d]", fn, grammar->n_time, V);
  M2M_REQUIRE(grammar->pitch_offset + grammar->n_pitch + grammar->n_time <= V, "%s: pitch_offset + n_pitch + n_time = %d > vocab_size %d",
              fn, grammar->pitch_offset + grammar->n_pitch + grammar->n_time, V);
  M2M_REQUIRE(g.eos_token_id == GRAM_EOS, "%s: the grammar ends a sequence with id %d, the model's eos_token_id is %d", fn, GRAM_EOS,
              g.eos_token_id);
  gp = GrammarParams{};
  gp.enable = 1; gp.pitch0 = grammar->pitch_offset; gp.time0 = gp.pitch0 + grammar->n_pitch; gp.end = gp.time0 + grammar->n_time;
  return M2M_OK;
}

// The MIDI token grammar (include/music2midi_amd.h): the processed or scored head with the call's GrammarParams block (DecodeCall::gram:
// decode_call uploads it and zeroes the clips' states); without a processor the neutral m2m_process_params.
extern "C" int m2m_generate_grammar(m2m_session* s, int max_length, const m2m_grammar_params* grammar, const m2m_process_params* proc,
                                    const m2m_sample_params* sample, int64_t* tokens_out_dev, float* scores_out_dev,
                                    float* logprobs_out_dev, int* out_len_host, void* stream) {
  const char* fn = "m2m_generate_grammar";
  if (!grammar) return m2m_generate_scored(s, max_length, proc, sample, tokens_out_dev, scores_out_dev, logprobs_out_dev, out_len_host, stream);
  M2M_REQUIRE(s && tokens_out_dev && out_len_host, "m2m_generate_grammar: null argument");
  GrammarParams gp{};
  int rc;
  if ((rc = fill_grammar_params(s, max_length, grammar, gp, fn))) return rc;
  if (scores_out_dev || logprobs_out_dev)
    return generate_scored(s, max_length, proc, sample, tokens_out_dev, scores_out_dev, logprobs_out_dev, out_len_host, stream, &gp, fn);
  m2m_process_params neutral{};
  neutral.repetition_penalty = 1.0f; neutral.forced_bos_token_id = -1; neutral.forced_eos_token_id = -1;
  return generate_processed(s, max_length, proc ? proc : &neutral, sample, tokens_out_dev, out_len_host, stream, &gp, fn);
}

// the decode loop of every head form (s->head_mode, set by decode_call)
static int decode_loop(m2m_session* s, const DecodeCall& c, int max_length, int* out_len_host, hipStream_t caller) {
  const char* fn = c.fn;
  const bool beam = c.head_mode & HEAD_BEAM;
  const int steps = max_length - 1, rows = beam ? s->B * c.beam_nb : s->B;
  const DecodeSwitches sw;
  int G = plan_groups(s, sw.group_rows, rows);        // beam search: chains split at clip boundaries
  const bool graph = sw.graph;
  const int U = sw.graph_steps;
  // Live-row re-packing at the host polls (decode.hip "live-row re-packing"): once a quarter of the packed rows have emitted EOS the
  // live ones are moved into the first slots and smaller chains take over.  M2M_COMPACT=0: rows keep their slots (round 4).  Never in
  // beam search: a clip's beams move through each other's cache slots, so a beam call does not consume the encode.
  const bool compact = !beam && sw.compact;
  int rc;
  // order every chain after whatever the caller enqueued (encode ran on the caller's stream)
  M2M_CHECK_HIP(hipEventRecord(s->ev_in, caller));
  for (int i = 0; i < G; ++i) {
    DecGroup& gr = s->groups[i];
    M2M_CHECK_HIP(hipStreamWaitEvent(gr.stream, s->ev_in, 0));
    if ((rc = decode_init(s, gr.view, steps, false, gr.stream))) return rc;
    if (beam && (rc = decode_beam_init(s, gr.view, gr.stream))) return rc;
    if (graph && (rc = ensure_graph(s, gr, U))) return rc;
    gr.state_host->done = (steps == 0);
  }
  // Launch round-robin over the chains in chunks; after each chunk (a POLL POINT, P steps launched) fetch the loop states so a
  // batch whose rows have all emitted EOS stops early (the kernels themselves turn into no-ops once their chain's state.done is
  // set).  The first polls come sooner (after 16, 32, 64, 96, 128 steps, then every 64): many rows of a real batch end within
  // their first tens of tokens, and every step before a re-packing costs the full batch.
  //
  // Look-ahead (M2M_POLL_LOOKAHEAD, default on): the snapshot of a poll - each chain's DecState and its slice of the finished
  // flags, copied to pinned memory on the chain's own stream, then an event - is followed AT ONCE by the first launch of the next
  // chunk, and only then does the host wait for the events.  The chains therefore never run dry at a poll.  What holds:
  //  (i)   the step counts P at which snapshots are taken are those of the draining poll (=0) for any steps, M2M_GRAPH_STEPS,
  //        M2M_NO_GRAPH and M2M_COMPACT, after a re-packing too: `launched` advances exactly as without the look-ahead, and the
  //        look-ahead is the FIRST launch of the chunk that starts at P (never more than that chunk), counted in `ahead`;
  //  (ii)  every decision - done, re-pack or not, which rows move, the `steps - P >= 64` condition - is a function of P and the
  //        snapshot at P alone, so ids, out_len, the range flag and repack_stats() do not depend on the switch;
  //  (iii) outside a re-packing and the end of the call the host waits for events only: no chain is drained;
  //  (iv)  state_host / fin_host are the targets of a poll's copies only; the next copy into them (the next poll's, or the fresh
  //        states of a re-packing) is enqueued after the host has read them, and `running` (not state_host) says which chains
  //        to launch while a copy is in flight;
  //  (v)   an error return leaves the look-ahead to decode_call's quiesce.
  // The look-ahead is not taken while two chains stream the same cross-K/V layers (decode_chains_may_drift: measured slower).
  // Steps that a look-ahead runs past the end of a chain (every row finished, or max_length reached) are no-ops, as the rest of
  // a graph always was.
  const int CHUNK = 64;
  const int unit = graph ? U : 1;      // decode steps per launch
  auto chunk_at = [&](int p) { return compact ? (p < 32 ? 16 : (p < 128 ? 32 : CHUNK)) : CHUNK; };
  bool running[MAX_GROUPS];            // chain i was not done in the last snapshot the host has read
  for (int i = 0; i < MAX_GROUPS; ++i) running[i] = steps > 0;
  auto launch = [&](int units) -> int {
    for (int k = 0; k < units; ++k)
      for (int i = 0; i < G; ++i) {
        DecGroup& gr = s->groups[i];
        if (!running[i]) continue;
        if (graph) M2M_CHECK_HIP(hipGraphLaunch(gr.graph_exec, gr.stream));
        else if (const int e = decode_launch_step(s, gr.view, false, nullptr, 0, gr.stream)) return e;
      }
    return M2M_OK;
  };
  int launched = 0;                    // steps launched up to the current poll point (the look-ahead not counted)
  int ahead = 0;                       // launches of the chunk that starts at `launched` already enqueued (the last poll's look-ahead)
  int cur_rows = rows;                 // packed slots still being decoded
  s->repacks = 0; s->rows_moved = 0;
  int out_len = 1;                     // longest finished chain so far (chains retired by a re-packing included)
  bool range_error = false;
  bool all_done = steps == 0;
  std::vector<int> mv_src, mv_dst;
  while (!all_done && launched < steps) {
    const int n = std::min(steps - launched, chunk_at(launched));
    const int units = ceil_div(n, unit);
    if ((rc = launch(units - ahead))) return rc;
    launched += units * unit;
    ahead = 0;
    // ---- poll point P = launched: the snapshot ...
    const bool may_repack = compact && steps - launched >= CHUNK && cur_rows >= 2 && cur_rows < 32000;
    for (int i = 0; i < G; ++i) {
      DecGroup& gr = s->groups[i];
      M2M_CHECK_HIP(hipMemcpyAsync(gr.state_host, gr.view.state, sizeof(DecState), hipMemcpyDeviceToHost, gr.stream));
      if (may_repack)
        M2M_CHECK_HIP(hipMemcpyAsync(s->fin_host + gr.view.b0, s->finished + gr.view.b0, (size_t)gr.view.nb * sizeof(int),
                                     hipMemcpyDeviceToHost, gr.stream));
      M2M_CHECK_HIP(hipEventRecord(gr.ev_done, gr.stream));
    }
    // ... the look-ahead: the first launch of the chunk that starts at P (without graphs: as many direct steps, within that chunk) ...
    if (sw.lookahead && launched < steps && decode_chains_may_drift(s, G)) {
      ahead = graph ? 1 : std::min(U, std::min(steps - launched, chunk_at(launched)));
      if ((rc = launch(ahead))) return rc;
    }
    // ... and the wait for the snapshot alone
    all_done = true;
    for (int i = 0; i < G; ++i) {
      DecGroup& gr = s->groups[i];
      M2M_CHECK_HIP(hipEventSynchronize(gr.ev_done));
      running[i] = !gr.state_host->done;
      if (running[i]) all_done = false;
    }
    // ---- re-pack the live rows, decided from the snapshot at P
    if (may_repack && !all_done) {
      const int* fin = s->fin_host;
      int live = 0;
      for (int b = 0; b < cur_rows; ++b) live += fin[b] ? 0 : 1;
      if (live >= 1 && (cur_rows - live) * 4 >= cur_rows) {
        if (ahead) {        // drain the look-ahead: rows move between idle chains, at the step count the chains have reached by now
          for (int i = 0; i < G; ++i) {
            DecGroup& gr = s->groups[i];
            M2M_CHECK_HIP(hipMemcpyAsync(gr.state_host, gr.view.state, sizeof(DecState), hipMemcpyDeviceToHost, gr.stream));
          }
          for (int i = 0; i < G; ++i) M2M_CHECK_HIP(hipStreamSynchronize(s->groups[i].stream));
        }
        int t_cur = -1, t_ended = 0;
        for (int i = 0; i < G; ++i) {                             // retire the current chains: keep what they report
          const DecState& hs = *s->groups[i].state_host;
          range_error |= hs.overflow != 0;
          if (hs.done) { if (hs.out_len > out_len) out_len = hs.out_len; if (hs.t > t_ended) t_ended = hs.t; }
          else t_cur = hs.t;
        }
        // a chain still running has done exactly the launched steps (P, and the look-ahead's); every chain may have ENDED inside
        // the look-ahead: the rows still move (the re-packing was decided at P), and the call ends with the chains as they are
        const bool ended = t_cur < 0;
        M2M_REQUIRE(!ended || ahead, "%s: no running chain at a re-packing point", fn);
        M2M_REQUIRE(ended || t_cur == std::min(launched + ahead * unit, steps), "%s: a chain at step %d, %d launched", fn, t_cur,
                    launched + ahead * unit);
        if (ended) t_cur = t_ended;
        mv_src.clear(); mv_dst.clear();
        for (int hole = 0, tail = live; hole < live; ++hole) {    // finished slots in front take the live rows from behind the packed range
          if (!fin[hole]) continue;
          while (tail < cur_rows && fin[tail]) ++tail;
          mv_src.push_back(tail++); mv_dst.push_back(hole);
        }
        hipStream_t st0 = s->groups[0].stream;
        // A chain that ended inside the look-ahead (at hs.t < t_cur: all its rows finished) stopped appending self K/V there, and its
        // rows go on as finished rows of chains at t_cur: with M2M_FINISHED_SKIP=0 they read those positions, so they are cleared.
        for (int i = 0; i < G && !ended; ++i) {
          const DecState& hs = *s->groups[i].state_host;
          if (hs.done && hs.t < t_cur && (rc = decode_clear_self(s, s->groups[i].view, hs.t, t_cur, st0))) return rc;
        }
        // Moving a row OVERWRITES the finished clip in its destination slot (cross K/V, self K/V, residual row): from here on the
        // session no longer holds the encode of clips 0..B-1 in clip order, so this generate CONSUMES it.  A later
        // m2m_decode_forced / m2m_generate_greedy / m2m_bench_kernel without a new m2m_encode returns M2M_ERR_STATE instead of
        // decoding permuted / duplicated clips.
        if (!mv_src.empty()) s->encoded = false;
        if (!mv_src.empty() && (rc = decode_move_rows(s, mv_src.data(), mv_dst.data(), (int)mv_src.size(), t_cur, st0))) return rc;
        M2M_CHECK_HIP(hipStreamSynchronize(st0));
        s->repacks += 1; s->rows_moved += (int)mv_src.size();
        if (ended) { all_done = true; continue; }
        cur_rows = live;
        G = plan_groups(s, sw.group_rows, cur_rows);
        for (int i = 0; i < G; ++i) {
          DecGroup& gr = s->groups[i];
          DecState hs{};
          hs.t = t_cur; hs.t_copy = t_cur; hs.done = 0; hs.out_len = 1; hs.n_unfinished = 0; hs.max_steps = steps;
          *gr.state_host = hs;
          M2M_CHECK_HIP(hipMemcpyAsync(gr.view.state, gr.state_host, sizeof(DecState), hipMemcpyHostToDevice, gr.stream));
          if (graph && (rc = ensure_graph(s, gr, U))) return rc;
          running[i] = true;
        }
      }
    }
  }
  // headless loop: the last step's arg-max is still a pending key (no later step consumed it)
  if (!beam && steps > 0)
    for (int i = 0; i < G; ++i)
      if ((rc = decode_finalize(s, s->groups[i].view, s->groups[i].stream))) return rc;
  // valid length = the longest chain (one process decoding the whole batch stops when EVERY row has finished)
  for (int i = 0; i < G; ++i) {
    DecGroup& gr = s->groups[i];
    M2M_CHECK_HIP(hipMemcpyAsync(gr.state_host, gr.view.state, sizeof(DecState), hipMemcpyDeviceToHost, gr.stream));
    M2M_CHECK_HIP(hipStreamSynchronize(gr.stream));
    const int l = steps == 0 ? 1 : gr.state_host->out_len;
    if (l > out_len) out_len = l;
    range_error |= gr.state_host->overflow != 0;
  }
  // the output, on the caller's stream (all chains are idle now)
  if (beam) {   // finalize (a clip that is not done stopped at max_length, t = steps); valid length = the longest hypothesis
    if ((rc = decode_beam_finalize(s, rows, steps, c.tokens_out, c.scores_out, max_length, caller))) return rc;
    M2M_CHECK_HIP(hipMemcpyAsync(&s->call_host->beam, s->beam_dev, sizeof(BeamParams), hipMemcpyDeviceToHost, caller));
  } else {      // pack [B, max_dec] -> caller's [B, max_length]
    M2M_CHECK_HIP(hipMemcpy2DAsync(c.tokens_out, (size_t)max_length * 8, s->tokens, (size_t)s->max_dec * 8,
                                   (size_t)max_length * 8, (size_t)s->B, hipMemcpyDeviceToDevice, caller));
  }
  M2M_CHECK_HIP(hipStreamSynchronize(caller));
  if (beam) { const int w = s->call_host->beam.max_hyp_len + 1; out_len = w < max_length ? w : max_length; }
  *out_len_host = out_len;
  if (range_error) {
    set_error("%s: a decoder activation left the fixed-point residual range (|x| >= 2^21) or was not finite; "
              "the fp32 reference would produce Inf/NaN logits here - token ids are not valid (check the checkpoint)", fn);
    return M2M_ERR_RANGE;
  }
  return M2M_OK;
}

// a parameter block filled on the host -> its device block in the workspace, on the caller's stream
static int upload(void* dev, const void* host, size_t bytes, hipStream_t caller, const char* fn) {
  if (hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, caller) == hipSuccess) return M2M_OK;
  set_error("%s: hipMemcpyAsync: %s", fn, hipGetErrorString(hipGetLastError()));
  return M2M_ERR_HIP;
}

// The parameter blocks the head reads reach the captured graphs through the workspace, ordered before the chains by the loop's event.
// The session's head mode holds for this call only, and nothing of a failed call is left running.
static int decode_call(m2m_session* s, const DecodeCall& c, int max_length, int* out_len_host, hipStream_t caller) {
  int rc = M2M_OK;
  if (c.head_mode & HEAD_SAMPLE) rc = upload(s->sample_dev, &s->call_host->sample, sizeof(SampleParams), caller, c.fn);
  if (rc == M2M_OK && (c.head_mode & HEAD_PROCESSED)) rc = upload(s->proc_dev, &s->call_host->proc, sizeof(ProcessParams), caller, c.fn);
  if (rc == M2M_OK && (c.head_mode & HEAD_PROCESSED)) {
    // the grammar block travels with every processed call (enable = 0 without a grammar); with one, the states of the call's rows
    // restart (one per clip; one per beam row in a processed beam call)
    s->call_host->gram = c.gram ? *c.gram : GrammarParams{};
    rc = upload(s->gram_dev, &s->call_host->gram, sizeof(GrammarParams), caller, c.fn);
    const size_t gram_rows = (size_t)s->B * (size_t)((c.head_mode & HEAD_BEAM) ? c.beam_nb : 1);
    if (rc == M2M_OK && c.gram && hipMemsetAsync(s->gram_state, 0, gram_rows * sizeof(GrammarState), caller) != hipSuccess) {
      set_error("%s: hipMemsetAsync: %s", c.fn, hipGetErrorString(hipGetLastError()));
      rc = M2M_ERR_HIP;
    }
  }
  if (rc == M2M_OK && (c.head_mode & HEAD_BEAM)) rc = upload(s->beam_dev, &s->call_host->beam, sizeof(BeamParams), caller, c.fn);
  if (rc == M2M_OK && (c.head_mode & HEAD_SCORED)) {
    // finished rows write nothing: the caller's buffers are zeroed on its stream, before the chains start
    const ScoreParams& sc = s->call_host->score;
    const size_t cells = (size_t)sc.rows * (size_t)sc.steps;
    hipError_t e = hipSuccess;
    if (sc.scores && cells) e = hipMemsetAsync(sc.scores, 0, cells * (size_t)s->m->g.vocab_size * sizeof(float), caller);
    if (e == hipSuccess && sc.logprobs && cells) e = hipMemsetAsync(sc.logprobs, 0, cells * sizeof(float), caller);
    if (e != hipSuccess) { set_error("%s: hipMemsetAsync: %s", c.fn, hipGetErrorString(e)); rc = M2M_ERR_HIP; }
    if (rc == M2M_OK) rc = upload(s->score_dev, &s->call_host->score, sizeof(ScoreParams), caller, c.fn);
  }
  if (rc == M2M_OK) {
    s->head_mode = c.head_mode; s->beam_nb = c.beam_nb;
    rc = decode_loop(s, c, max_length, out_len_host, caller);
    s->head_mode = HEAD_GREEDY; s->beam_nb = 0;
  }
  if (rc != M2M_OK) quiesce(s, caller);
  return rc;
}

// Beam search (hf 4.34 _beam_search / BeamSearchScorer, see include/music2midi_amd.h): the B encoded clips are decoded as B x nb
// rows (clip-major).  The step's head is dec_beam_kernel; dec_beam_final_kernel writes the output.
// the checks of a beam call and its BeamParams block (m2m_generate_beam, m2m_generate_beam_processed); `h` is the caller's: the
// session's staging block is written once every check of the call has passed
static int fill_beam_params(const m2m_session* s, int max_length, const m2m_beam_params* p, BeamParams& h, const char* fn) {
  M2M_REQUIRE(p->num_beams >= 2 && p->num_beams <= BEAM_MAX, "%s: num_beams %d outside [2, %d] (one beam is m2m_generate_greedy)", fn,
              p->num_beams, BEAM_MAX);
  M2M_REQUIRE(p->num_return_sequences >= 1 && p->num_return_sequences <= p->num_beams,
              "%s: num_return_sequences %d has to be in [1, num_beams = %d]", fn, p->num_return_sequences, p->num_beams);
  M2M_REQUIRE(p->early_stopping >= 0 && p->early_stopping <= 2, "%s: early_stopping %d must be 0 (False), 1 (True) or 2 (\"never\")", fn,
              p->early_stopping);
  M2M_REQUIRE(isfinite(p->length_penalty), "%s: length_penalty must be finite, got %g", fn, (double)p->length_penalty);
  const int V = s->m->g.vocab_size;
  M2M_REQUIRE(V <= SAMPLE_MAX_VOCAB && V >= 2 * p->num_beams, "%s: vocab_size %d outside [2 num_beams, %d] (the beam head keeps a row in "
              "one wavefront's registers)", fn, V, SAMPLE_MAX_VOCAB);
  int rc;
  if ((rc = require_encoded(s, fn))) return rc;
  M2M_REQUIRE(max_length >= 1 && max_length <= s->max_dec, "%s: max_length %d outside [1, %d]", fn, max_length, s->max_dec);
  M2M_REQUIRE((int64_t)s->B * p->num_beams <= s->max_batch, "%s: %d clips x %d beams > the session's max_batch %d", fn, s->B, p->num_beams,
              s->max_batch);
  h = BeamParams{};
  h.nb = p->num_beams; h.lp = p->length_penalty; h.early = p->early_stopping; h.n = p->num_return_sequences;
  h.max_length = max_length; h.max_hyp_len = 0;
  return M2M_OK;
}

extern "C" int m2m_generate_beam(m2m_session* s, int max_length, const m2m_beam_params* p, int64_t* tokens_out_dev,
                                 float* scores_out_dev, int* out_len_host, void* stream) {
  const char* fn = "m2m_generate_beam";
  M2M_REQUIRE(s && p && tokens_out_dev && out_len_host, "m2m_generate_beam: null argument");
  int rc;
  BeamParams bp{};
  if ((rc = fill_beam_params(s, max_length, p, bp, fn))) return rc;
  s->call_host->beam = bp;
  return decode_call(s, {fn, HEAD_BEAM, p->num_beams, tokens_out_dev, scores_out_dev}, max_length, out_len_host, (hipStream_t)stream);
}

// Beam search under the token grammar and the logits processors (include/music2midi_amd.h): the processed beam head (HEAD_BEAM |
// HEAD_PROCESSED, dec_beam_kernel<NPL, true>) with the call's ProcessParams block (the neutral one without a processor) and its
// GrammarParams block (enable = 0 without a grammar).  The processors that read a row's history are refused: a beam's history is
// scattered through the ancestry table.
extern "C" int m2m_generate_beam_processed(m2m_session* s, int max_length, const m2m_beam_params* p, const m2m_grammar_params* grammar,
                                           const m2m_process_params* proc, int64_t* tokens_out_dev, float* scores_out_dev,
                                           int* out_len_host, void* stream) {
  const char* fn = "m2m_generate_beam_processed";
  if (!grammar && !proc) return m2m_generate_beam(s, max_length, p, tokens_out_dev, scores_out_dev, out_len_host, stream);
  M2M_REQUIRE(s && p && tokens_out_dev && out_len_host, "m2m_generate_beam_processed: null argument");
  int rc;
  // validate first, then fill: a refused call leaves the session's staging blocks as they were
  BeamParams bp{};
  if ((rc = fill_beam_params(s, max_length, p, bp, fn))) return rc;
  GrammarParams gp{};
  if (grammar && (rc = fill_grammar_params(s, max_length, grammar, gp, fn))) return rc;
  m2m_process_params neutral{};
  neutral.repetition_penalty = 1.0f; neutral.forced_bos_token_id = -1; neutral.forced_eos_token_id = -1;
  static thread_local ProcessParams h;       // (4.4 KB: not on the stack)
  if ((rc = fill_process_params(s, max_length, proc ? proc : &neutral, h, fn))) return rc;   // (max_length <= 2048 too)
  M2M_REQUIRE(h.penalty == 1.0f && h.ngram == 0 && h.n_bad == 0, "%s: repetition_penalty, no_repeat_ngram_size and bad_words sequences of "
              "two or more ids read a row's history and are not applied under beam search", fn);
  s->call_host->beam = bp;
  s->call_host->proc = h;
  return decode_call(s, {fn, HEAD_BEAM | HEAD_PROCESSED, p->num_beams, tokens_out_dev, scores_out_dev, grammar ? &gp : nullptr}, max_length,
                     out_len_host, (hipStream_t)stream);
}

// Teacher-forced decoder pass over all Ld positions at once (hf: modeling_t5.py:448-509 per block, :898-1066 wrapper):
// the encoder's MFMA GEMMs and flash attention applied to the decoder weights, causal + relative-position bias in
// the self-attention, the cached cross K/V (V transposed once per layer) in the cross-attention.  Same arithmetic as
// Ld KV-cached decode steps (M2M_FORWARD=step runs those instead), ~1/50 of the time at Ld = 1024.
static int forward_batched(m2m_session* s, const int64_t* ids, int Ld, float* logits_out, hipStream_t st) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int P = m->precision, d = g.d_model;
  const BatchedPass p{s, P, s->B, Ld, ceil_div(Ld, 64) * 64, st};
  int rc;
  if ((rc = launch_embed_rows(ids, m->shared, s->x_enc, p.M(), d, g.vocab_size, g.pad_token_id, st))) return rc;
  for (int l = 0; l < g.num_decoder_layers; ++l) {
    const DecLayerPacked& L = m->dec[l];
    if ((rc = self_attn_sublayer(p, L.ln0, L.wqkv, L.wo, s->dec_bias_full_tab, s->max_dec, s->dec_bias_far, true))) return rc;
    if ((rc = cross_attn_sublayer(p, L, l))) return rc;
    if ((rc = feed_fwd_sublayer(p, L.ln2, L.wi, L.wo_ff, EPI_GATED16))) return rc;
  }
  GemmArgs a{};
  a.vt_which = -1;
  a.A = s->h_enc; a.W = m->lm_head; a.M = p.M(); a.N = g.vocab_size; a.K = d; a.out = logits_out; a.ldo = g.vocab_size;
  a.nx = s->x_enc; a.nw = m->dec_final_ln; a.neps = g.layer_norm_eps;
  return launch_norm_gemm(P, EPI_STORE_F32, a, st);
}

extern "C" int m2m_session_repack_stats(const m2m_session* s, int* repacks_out, int* rows_moved_out) {
  M2M_REQUIRE(s && repacks_out && rows_moved_out, "m2m_session_repack_stats: null argument");
  *repacks_out = s->repacks; *rows_moved_out = s->rows_moved;
  return M2M_OK;
}

extern "C" int m2m_decode_forced(m2m_session* s, const int64_t* dec_input_ids_dev, int Ld, float* logits_out_dev, void* stream) {
  M2M_REQUIRE(s && dec_input_ids_dev && logits_out_dev, "m2m_decode_forced: null argument");
  if (const int rc = require_encoded(s, "m2m_decode_forced")) return rc;
  M2M_REQUIRE(Ld >= 1 && Ld <= s->max_dec, "m2m_decode_forced: Ld %d outside [1, %d]", Ld, s->max_dec);
  hipStream_t st = (hipStream_t)stream;
  const EncSwitchScope sw_scope(&s->sw.enc);
  M2M_CHECK_HIP(hipMemcpyAsync(s->forced_ids, dec_input_ids_dev, (size_t)s->B * Ld * 8, hipMemcpyDeviceToDevice, st));
  const char* fwd = env_str("M2M_FORWARD");         // "step": Ld KV-cached decode steps instead (read per call, here only: tests toggle it on one session)
  const bool stepwise = fwd && strcmp(fwd, "step") == 0;
  if (!stepwise) return forward_batched(s, s->forced_ids, Ld, logits_out_dev, st);
  const DecView all{0, s->B, s->states};
  int rc;
  if ((rc = decode_init(s, all, Ld, true, st))) return rc;
  for (int t = 0; t < Ld; ++t)
    if ((rc = decode_launch_step(s, all, true, logits_out_dev, Ld, st))) return rc;
  DecState hs{};
  M2M_CHECK_HIP(hipMemcpyAsync(&hs, all.state, sizeof(hs), hipMemcpyDeviceToHost, st));
  M2M_CHECK_HIP(hipStreamSynchronize(st));
  if (hs.overflow) {
    set_error("m2m_decode_forced: a decoder activation left the fixed-point residual range (|x| >= 2^21) or was not finite");
    return M2M_ERR_RANGE;
  }
  return M2M_OK;
}

// ------------------------------------------------------------------ bench ---
extern "C" int m2m_bench_kernel(m2m_session* s, int which, int self_len, int iters, float* avg_us_host,
                                int64_t* bytes_host, void* stream) {
  M2M_REQUIRE(s && avg_us_host && bytes_host && iters >= 1, "m2m_bench_kernel: bad argument");
  if (const int rc = require_encoded(s, "m2m_bench_kernel")) return rc;
  M2M_REQUIRE(self_len >= 1 && self_len <= s->max_dec, "m2m_bench_kernel: self_len out of range");
  M2M_REQUIRE(which == M2M_KERNEL_DEC_CROSS_ATTN || which == M2M_KERNEL_DEC_SELF_ATTN || which == M2M_KERNEL_DEC_STEP,
              "m2m_bench_kernel: unknown kernel id %d", which);
  const m2m_model* m = s->m;
  const int Ld = m->g.num_decoder_layers;
  hipStream_t caller = (hipStream_t)stream;
  const DecodeSwitches sw;
  const int G = plan_groups(s, sw.group_rows);
  M2M_CHECK_HIP(hipEventRecord(s->ev_in, caller));
  for (int i = 0; i < G; ++i) M2M_CHECK_HIP(hipStreamWaitEvent(s->groups[i].stream, s->ev_in, 0));
  int rc;
  // every chain sees a live loop in its (self_len)-th step
  DecState hs{}; hs.t = self_len - 1; hs.t_copy = self_len - 1; hs.done = 0; hs.out_len = 1; hs.n_unfinished = 0; hs.max_steps = s->max_dec;
  {   // slot -> clip table of the greedy loop: identity (a fresh session has none, a re-packed generate leaves a permutation)
    std::vector<int> ident((size_t)s->B);
    for (int b = 0; b < s->B; ++b) ident[(size_t)b] = b;
    M2M_CHECK_HIP(hipMemcpy(s->tok_row, ident.data(), ident.size() * sizeof(int), hipMemcpyHostToDevice));
  }
  for (int i = 0; i < G; ++i) {
    const DecGroup& gr = s->groups[i];
    M2M_CHECK_HIP(hipMemcpyAsync(gr.view.state, &hs, sizeof(hs), hipMemcpyHostToDevice, gr.stream));
    // ... with every row live: after a generate whose rows emitted EOS the finished-row early-out would skip those rows' K/V
    // streams in the timed launches while bytes_host below counts them in full
    M2M_CHECK_HIP(hipMemsetAsync(s->finished + gr.view.b0, 0, (size_t)gr.view.nb * sizeof(int), gr.stream));
  }
  for (int i = 0; i < G; ++i) M2M_CHECK_HIP(hipStreamSynchronize(s->groups[i].stream));
  hipEvent_t e0, e1;
  M2M_CHECK_HIP(hipEventCreate(&e0));
  M2M_CHECK_HIP(hipEventCreate(&e1));
  const int same_layer = env_int("M2M_BENCH_SAME_LAYER", 0);   // diagnostic: K/V working set small enough for the Infinity Cache
  // the kernel exactly as the decode loop launches it: every chain launches ITS clips on ITS stream (the chains run
  // side by side), back to back, cycling through the decoder layers so the K/V working set is the real loop's.
  // One "launch" of the figures below = the co-scheduled launches of all G chains = all B clips.
  auto run = [&](int n) -> int {
    for (int i = 0; i < n; ++i) {
      const int layer = same_layer ? 0 : i % Ld;
      for (int c = 0; c < G; ++c) {
        const DecGroup& gr = s->groups[c];
        if (which == M2M_KERNEL_DEC_CROSS_ATTN) { if ((rc = decode_launch_attn(s, gr.view, false, layer, 0, gr.stream, s->sw.headless))) return rc; }
        else if (which == M2M_KERNEL_DEC_SELF_ATTN) { if ((rc = decode_launch_attn(s, gr.view, true, layer, self_len, gr.stream, s->sw.headless))) return rc; }
      }
    }
    return M2M_OK;
  };
  auto fork = [&](hipEvent_t ev) -> int {
    M2M_CHECK_HIP(hipEventRecord(ev, caller));
    for (int c = 0; c < G; ++c) M2M_CHECK_HIP(hipStreamWaitEvent(s->groups[c].stream, ev, 0));
    return M2M_OK;
  };
  auto join = [&](hipEvent_t ev) -> int {
    for (int c = 0; c < G; ++c) {
      M2M_CHECK_HIP(hipEventRecord(s->groups[c].ev_done, s->groups[c].stream));
      M2M_CHECK_HIP(hipStreamWaitEvent(caller, s->groups[c].ev_done, 0));
    }
    M2M_CHECK_HIP(hipEventRecord(ev, caller));
    return M2M_OK;
  };
  float ms = 0.f;
  if (which != M2M_KERNEL_DEC_STEP) {
    if ((rc = run(Ld))) return rc;  // warm-up
    if ((rc = fork(e0))) return rc;
    if ((rc = run(iters))) return rc;
    if ((rc = join(e1))) return rc;
    M2M_CHECK_HIP(hipEventSynchronize(e1));
    M2M_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  } else {
    // the whole decode step as the loop runs it: all chains concurrently, each replaying its graph
    // (t advances by `iters` from self_len - 1, so self-attention lengths are the real ones)
    M2M_REQUIRE(self_len - 1 + iters < s->max_dec, "m2m_bench_kernel: self_len + iters exceeds max_dec_len");
    const int U = 1;
    for (int i = 0; i < G; ++i) if (sw.graph && (rc = ensure_graph(s, s->groups[i], U))) return rc;
    M2M_CHECK_HIP(hipEventRecord(e0, caller));
    for (int i = 0; i < G; ++i) M2M_CHECK_HIP(hipStreamWaitEvent(s->groups[i].stream, e0, 0));
    for (int k = 0; k < iters; ++k)
      for (int i = 0; i < G; ++i) {
        DecGroup& gr = s->groups[i];
        if (sw.graph) M2M_CHECK_HIP(hipGraphLaunch(gr.graph_exec, gr.stream));
        else if ((rc = decode_launch_step(s, gr.view, false, nullptr, 0, gr.stream))) return rc;
      }
    for (int i = 0; i < G; ++i) {
      M2M_CHECK_HIP(hipEventRecord(s->groups[i].ev_done, s->groups[i].stream));
      M2M_CHECK_HIP(hipStreamWaitEvent(caller, s->groups[i].ev_done, 0));
    }
    M2M_CHECK_HIP(hipEventRecord(e1, caller));
    M2M_CHECK_HIP(hipEventSynchronize(e1));
    M2M_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  *avg_us_host = ms * 1000.0f / (float)iters;
  const int64_t qo = (int64_t)s->B * m->inner * (4 + (int64_t)m->esize);
  const int64_t kv_cross = (int64_t)s->B * m->inner * s->S * 2 * (int64_t)m->esize;
  const int64_t kv_self = (int64_t)s->B * m->inner * self_len * 2 * (int64_t)m->esize;
  if (which == M2M_KERNEL_DEC_CROSS_ATTN) *bytes_host = kv_cross + qo;
  else if (which == M2M_KERNEL_DEC_SELF_ATTN) *bytes_host = kv_self + qo;
  else *bytes_host = (int64_t)Ld * (kv_cross + kv_self + 2 * qo);  // + weights: added by the caller
  for (int i = 0; i < G; ++i) M2M_CHECK_HIP(hipStreamSynchronize(s->groups[i].stream));
  return M2M_OK;
}
