/*
 * music2midi_amd — C ABI of the MI355X (gfx950) Music2MIDI inference hot path.
 *
 * The reference (ytinyui/music2midi) is pure Python with no FFI of its own; its
 * hot path is two Python call sites into third-party libraries:
 *
 *   ref: music2midi/input.py:33-41      LogMelSpectrogram.forward  (torchaudio MelSpectrogram)
 *   ref: music2midi/input.py:50-59      Conditioning.forward       (2 embedding rows prepended)
 *   ref: music2midi/transformer.py:28-39 T5Transformer.forward     (HF T5 teacher-forced forward)
 *   ref: music2midi/transformer.py:41-45 T5Transformer.generate    (HF T5 encoder + greedy generate)
 *
 * Each entry point below names the call site it replaces.  INTEGRATION.md shows
 * the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - Every function returns 0 on success or a negative M2M_ERR_* code; it never
 *    throws or aborts.  m2m_last_error() returns a thread-local message.
 *  - "dev" pointers are device (HBM) addresses, "host" pointers are host
 *    addresses.  The caller owns every input, output and workspace buffer; the
 *    library owns only what *_create() returns (plans, repacked weights,
 *    sessions) until the matching *_destroy().
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *    All work is enqueued asynchronously on it unless stated otherwise.
 *  - No function allocates or frees device memory except the *_create /
 *    *_destroy pairs.
 */
#ifndef MUSIC2MIDI_AMD_H
#define MUSIC2MIDI_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M2M_ABI_VERSION 1

enum {
  M2M_OK = 0,
  M2M_ERR_INVALID = -1,     /* bad argument / unsupported geometry */
  M2M_ERR_HIP = -2,         /* a HIP runtime call failed */
  M2M_ERR_NOMEM = -3,       /* workspace too small / allocation failed */
  M2M_ERR_STATE = -4,       /* call order violated (e.g. generate before encode) */
  M2M_ERR_RANGE = -5        /* the decoder produced a value outside its fixed-point residual range (|x| >= 2^21) or a
                               non-finite one (corrupt checkpoint, diverged fine-tune): the token ids are NOT valid */
};

enum {
  M2M_PREC_FP32 = 0,        /* fp32 weights / KV / GEMM inputs (f32 MFMA): parity mode */
  M2M_PREC_BF16 = 1,        /* bf16 weights / KV / GEMM inputs, fp32 accumulate: throughput mode */
  M2M_PREC_FP8 = 2          /* m2m_trainer_create only: as BF16, but the dense projection products run on block-scaled OCP FP8
                               (MXFP8, e4m3 elements, 32 per E8M0 scale): forward and dX by default, the weight gradients too with
                               M2M_FP8_PARTS=fwd,dx,dw; M2M_FP8_GRAD=e5m2 for e5m2 gradient operands — BASELINE configs[4] */
};

int m2m_abi_version(void);
const char* m2m_last_error(void);

/* Number of visible HIP devices (0 when none; never fails). */
int m2m_device_count(void);

/* ------------------------------------------------------------------------- *
 * Frontend: framed STFT -> |X|^2 -> mel filterbank -> log(clamp(., 1e-6))
 * replaces ref: music2midi/input.py:25-41 (torchaudio MelSpectrogram + log).
 * ------------------------------------------------------------------------- */
typedef struct m2m_frontend m2m_frontend;

typedef struct {
  int n_fft;                /* must be 2048 (ref: config.yaml:12) */
  int hop_length;           /* 1..n_fft/2 (reference: 256) */
  int n_freqs;              /* n_fft/2 + 1 */
  int n_mels;               /* = d_model (ref: music2midi/transformer.py:20) */
  const float* window_host; /* [n_fft] analysis window (Hann, periodic) */
  const float* fb_host;     /* [n_freqs, n_mels] row-major mel filterbank (dense) */
} m2m_frontend_desc;

int  m2m_frontend_create(const m2m_frontend_desc* desc, m2m_frontend** out);
void m2m_frontend_destroy(m2m_frontend* fe);
/* frames = 1 + n_samples / hop (center=True), or a negative error. */
int  m2m_frontend_num_frames(const m2m_frontend* fe, int n_samples);
/* non-zero taps the sparse filterbank keeps (diagnostic). */
int  m2m_frontend_fb_nnz(const m2m_frontend* fe);

/*
 * wav_dev  [B, T] fp32 row-major.
 * out_dev  row f of clip b is written at out_dev + b*out_batch_stride + (row_offset + f)*n_mels
 *          (fp32).  With row_offset = n_cond and out_batch_stride = (n_cond+frames)*n_mels the
 *          kernel writes straight into the encoder input, leaving rows [0, n_cond) for
 *          m2m_cond_rows_f32 — the reference's torch.cat copy (input.py:59) never happens.
 * T >= n_fft/2 + 1 (reflect padding needs it, as torch.stft does).
 */
int m2m_logmel_f32(const m2m_frontend* fe, const float* wav_dev, int B, int T,
                   float* out_dev, int64_t out_batch_stride, int row_offset, void* stream);

/* The kernel form and launch geometry m2m_logmel_f32(fe, B, T, ...) uses (read-only; launches nothing). */
enum {
  M2M_FE_FORM_V2_NJ6 = 0,         /* logmel_v2_kernel<16, 6>: hop <= 272, n_mels <= 384 */
  M2M_FE_FORM_V2_NJ8 = 1,         /* logmel_v2_kernel<16, 8>: hop <= 272, 385 <= n_mels <= 512 */
  M2M_FE_FORM_V1_TAPS_LDS = 2,    /* logmel_kernel<true>: first form, padded tap table in LDS */
  M2M_FE_FORM_V1_TAPS_GLOBAL = 3  /* logmel_kernel<false>: first form, padded tap table read from memory */
};
typedef struct {
  int form;              /* M2M_FE_FORM_* */
  int grid_x, grid_y;    /* workgroups: chunk groups per clip, clips */
  int chunks;            /* chunks each workgroup walks */
  int frames_per_chunk;  /* FR (16 in the second form) */
  int frames;            /* 1 + T / hop */
  int n_wpad;            /* floats in the padded tap table */
  int lds_bytes;         /* dynamic LDS per workgroup */
} m2m_frontend_plan_t;
int m2m_frontend_plan(const m2m_frontend* fe, int B, int T, m2m_frontend_plan_t* out);

/*
 * Conditioning rows, replaces ref: music2midi/input.py:57-59.
 * tables_dev_host: host array of n_tables device pointers, table i is [n_i, n_dim] fp32.
 * table_rows_host: host array with n_i (indices are range-checked on device: an
 *                  out-of-range index writes NaNs into that row rather than faulting).
 * idx_dev [B, n_tables] int64.  Row i of clip b lands at out_dev + b*out_batch_stride + i*n_dim.
 */
int m2m_cond_rows_f32(const float* const* tables_dev_host, const int* table_rows_host, int n_tables,
                      int n_dim, const int64_t* idx_dev, int B, float* out_dev,
                      int64_t out_batch_stride, void* stream);

/* ------------------------------------------------------------------------- *
 * Training augmentation: peak normalisation + pitch shift of a waveform batch, replaces
 * ref: music2midi/dataset.py:131-133,157-160 (librosa.util.normalize, librosa.effects.pitch_shift).
 * The definition is music2midi_amd/audio.py (normalize, pitch_shift): n_fft 2048, hop 512, periodic Hann,
 * zero-padded centred frames; phase-vocoder stretch by rate = 2^(-step/12); polyphase resampling by
 * up/down = rate (denominator <= 1000) through a Kaiser(5.0) windowed sinc of 20 max(up, down) + 1 taps; fix_length.
 * ------------------------------------------------------------------------- */
typedef struct m2m_augment m2m_augment;

#define M2M_AUGMENT_MAX_STEP 12            /* |step| <= 12 semitones */
#define M2M_AUGMENT_MAX_SAMPLES (1 << 22)  /* T <= 2^22 */

/* The handle owns the window, the FFT twiddles and one resampling filter per step in -12..12 (device and host copies). */
int  m2m_augment_create(m2m_augment** out);
void m2m_augment_destroy(m2m_augment* a);

/* What audio.pitch_shift computes on the way for a clip of T samples shifted by `step` semitones.  Host arithmetic only:
 * `a` may be NULL, nothing is launched.  step 0 reports up = down = 1, taps = 0 and the unstretched extents. */
typedef struct {
  int frames;            /* 1 + T / 512 */
  int stretched_frames;  /* len(np.arange(0, frames, rate)) */
  int stretched_len;     /* int(round(T / rate)) */
  int up, down;          /* Fraction(rate).limit_denominator(1000) */
  int taps;              /* 20 max(up, down) + 1 */
  int cap_frames;        /* 2 * frames: rows per clip of the stretched-STFT workspace region (the extent at step +12) */
  int cap_len;           /* 2 * T: floats per clip of the stretched-waveform workspace region */
} m2m_augment_plan_t;
int m2m_augment_plan(const m2m_augment* a, int T, int step, m2m_augment_plan_t* out);
/* The resampling filter of `step` (fp32, as scipy's resample_poly hands it to upfirdn for fp32 input): the first n of its taps to
 * out_host.  Host arithmetic only; returns the number of taps (0 for step 0) or a negative error. */
int m2m_augment_filter(int step, float* out_host, int n);

/* Bytes of workspace_dev for a call with B clips of T samples (any steps), or a negative error. */
int64_t m2m_augment_workspace_bytes(int B, int T);

/* Optional copies of the intermediates, each dense over the batch (device pointers; a NULL member is skipped):
 *   stft            [B][frames][1025] complex fp32 (re, im) of the (normalised) clip
 *   stretched_stft  [B][cap_frames][1025] complex fp32: rows < the clip's stretched_frames are meaningful
 *   stretched_wave  [B][cap_len] fp32: samples < the clip's stretched_len are meaningful
 * The rest of a region, and all of a step-0 clip's part (it is copied, not transformed), is unspecified. */
typedef struct {
  float* stft;
  float* stretched_stft;
  float* stretched_wave;
} m2m_augment_stages;

/*
 * out_dev[b] = pitch_shift(normalize_host[b] ? normalize(wav_dev[b]) : wav_dev[b], steps_host[b]),  wav_dev / out_dev [B, T] fp32.
 * steps_host [B] int semitones, normalize_host [B] bytes (NULL = no clip is normalised): host arrays, read before the call returns.
 * A step-0 clip is copied (bit-equal); normalisation divides by max |y| (bit-equal to the host function, skipped below FLT_MIN).
 * Every clip's result is independent of the other clips of the batch.  Nothing is synchronised and nothing returns to the host.
 * M2M_ERR_INVALID before anything is launched: B outside 1..65535, T outside 1..2^22, a |step| > 12, out_dev overlapping wav_dev.
 */
int m2m_pitch_shift_f32(const m2m_augment* a, const float* wav_dev, int B, int T, const int* steps_host,
                        const unsigned char* normalize_host, float* out_dev, void* workspace_dev,
                        const m2m_augment_stages* stages, void* stream);

/* ------------------------------------------------------------------------- *
 * Scoring of decoded tokens: token ids -> notes -> melody -> the counts of the chroma accuracy, replaces for labelled decodes
 * ref: music2midi/tokenizer.py:169-200 (decode), music2midi/utils.py:5-20 and music2midi/evaluation.py:10-75.
 * The definitions are music2midi_amd/tokenizer.py (_decode_tokens, _decode), utils.py (numpy_to_midi) and evaluation.py; the
 * results are EQUAL to theirs (integers; the frame arithmetic repeats the host's float64 operations).  No handle, no workspace,
 * no environment switch; both calls enqueue on `stream` and return nothing to the host.  Every M2M_ERR_INVALID below is
 * answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_SCORE_MAX_TOKENS 2048          /* ids per row */
#define M2M_SCORE_MAX_ROWS 65535
#define M2M_SCORE_MAX_FRAMES (1 << 22)     /* frames of 10 ms per timeline: 11.6 hours */
#define M2M_SCORE_MAX_LABELS (1 << 24)     /* label notes per call */

/* len(np.arange(0, end_seconds, 1 / 100)) as the kernels compute it: ceil(end_seconds / (1.0 / 100.0)) in double; 0 for an end
 * that is not positive.  Host arithmetic, exported so that the formula can be tested without a GPU. */
int64_t m2m_score_frame_count(double end_seconds);

/*
 * MidiTokenizer.decode without the host: row r of ids_dev [R, L] int64 (row r at ids_dev + r * row_stride) is one state machine
 * over (time index, mode, pitch); ids 0 / 1 are skipped, 2 ends the row, 3 / 4 are ONSET / OFFSET, [pitch_offset, time_offset) are
 * pitches and EVERY id >= time_offset is a time; row r adds r * steps_per_row to its time indices (0: "batched").
 * notes_out_dev [R, L, 3] int32: (onset index, offset index, pitch) of the closed notes of the row in emission order;
 * counts_out_dev [R] int32 their number (L is a true bound: every emission consumes an id), or -1 for a row holding an id outside
 * [0, vocab_size) - nothing is written for it.  Entries beyond a row's count are unspecified.
 * M2M_ERR_INVALID: R outside 1..65535, L outside 1..2048, row_stride < L, vocab_size outside 1..4096, pitch_offset < 5, a pitch
 * range outside 1..128 ids, time_offset > vocab_size, steps_per_row < 0, a time index or an element offset beyond int32.
 */
int m2m_score_detokenize(const int64_t* ids_dev, int R, int L, int64_t row_stride, int64_t steps_per_row, int pitch_offset,
                         int time_offset, int vocab_size, int32_t* notes_out_dev, int32_t* counts_out_dev, void* stream);

/*
 * The same decode with a confidence per note (the definition: music2midi_amd/confidence.py, note_logprobs).  logprobs_dev [R, L]
 * float32 (row r at logprobs_dev + r * lp_row_stride) holds the log-probability of every id, column-aligned with ids_dev.  Every
 * note and every OFFSET event takes (lp[time] + lp[mode]) + lp[pitch] of the three tokens that made it - the latest time token, the
 * latest ONSET / OFFSET token, the latest pitch token - as rounded float32 additions in that order; a closed note carries its own
 * sum (on) and the sum of the event that closed it (off).  A note is dropped iff on + off < min_logprob is true in float32: a NaN
 * total is kept, -inf keeps every note.  notes_dev / counts_dev hold the kept notes only, in m2m_score_detokenize's layout (the
 * one m2m_score_chroma_counts reads); note_lp_dev [R, L, 2] float32 holds (on, off) of note n of row r at [r, n].
 * The limits, the -1 count of a row with an id outside the vocabulary and every M2M_ERR_INVALID are m2m_score_detokenize's; also
 * M2M_ERR_INVALID: lp_row_stride < L, a log-probability offset beyond int32, a null logprobs_dev or note_lp_dev.
 */
int m2m_score_detokenize_scored(const int64_t* ids_dev, int R, int L, int64_t row_stride, int64_t steps_per_row,
                                int pitch_offset, int time_offset, int vocab_size,
                                const float* logprobs_dev, int64_t lp_row_stride, float min_logprob,
                                int32_t* notes_dev, int32_t* counts_dev, float* note_lp_dev, void* stream);

/*
 * evaluation.extract_midi_melody + the integer core of melody_chroma_accuracy, per timeline.  The output notes are
 * m2m_score_detokenize's (seconds = index * time_step); row r belongs to timeline r, or every row to timeline 0 when sequential.
 * labels_dev [3, n_labels] float64: starts, ends, pitches (whole numbers 0..127) of the label notes, those of timeline t at
 * [label_offsets_dev[t], label_offsets_dev[t + 1]) (int32 [n_timelines + 1]); a note with end <= start does not exist.
 * frame_cap: the caller's upper bound on n_frames of any timeline (it sizes the grid).
 * out_dev [n_timelines, 3] int32, zeroed on `stream` first: correct = frames where both melodies sound and differ by a multiple of
 * 12, voiced = frames where the label melody sounds, frames = n_frames - or -1 (and no counts) for a timeline beyond frame_cap.
 * M2M_ERR_INVALID: R, L as above, n_timelines other than R (1 when sequential), time_step outside (0, 3600], n_labels outside
 * 0..2^24, frame_cap outside 1..2^22, a null pointer.
 */
int m2m_score_chroma_counts(const int32_t* notes_dev, const int32_t* counts_dev, int R, int L, int sequential, double time_step,
                            const double* labels_dev, const int32_t* label_offsets_dev, int n_labels, int n_timelines, int frame_cap,
                            int32_t* out_dev, void* stream);

#define M2M_SCORE_MAX_THRESHOLDS 64        /* confidence thresholds per m2m_score_note_counts call */

/* The bytes of workspace m2m_score_note_counts needs for these sizes: 36 per label note + 24 per output slot (R * L) +
 * 8 * n_thresholds * (n_labels + R * L), every array rounded up to 8 bytes.  Host arithmetic; -1 for a size out of range. */
int64_t m2m_score_note_workspace_bytes(int R, int L, int n_labels, int n_thresholds);

/*
 * Note-level matching (the definition: music2midi_amd/note_metrics.py, match_counts - the hit rules of
 * mir_eval.transcription.match_notes and the size of a maximum bipartite matching), per timeline and per confidence threshold.
 * notes_dev, counts_dev, R, L, sequential, time_step, labels_dev, label_offsets_dev, n_labels and n_timelines are
 * m2m_score_chroma_counts' (seconds = double(index) * time_step; a note with end <= start does not exist on either side).
 * A label note r and an output note e hit when their pitches are equal, rint(fabs(r.on - e.on) * 1e6) / 1e6 <= onset_tolerance and,
 * unless offset_ratio < 0 (onsets only), rint(fabs(r.off - e.off) * 1e6) / 1e6 <= fmax(offset_ratio * (r.off - r.on),
 * offset_min_tolerance): float64, one rounded operation each, never contracted.
 * note_lp_dev [R, L, 2] float32 (m2m_score_detokenize_scored's, may be NULL) and min_logprobs_dev [n_thresholds] float32: output
 * note e counts under threshold k unless float32(on + off) < min_logprobs_dev[k] is true in float32 (a NaN total is kept, -inf
 * keeps every note).  With note_lp_dev NULL there is one threshold, it keeps every note and min_logprobs_dev is not read (it may
 * be NULL then, and only then).
 * workspace_dev: at least m2m_score_note_workspace_bytes(R, L, n_labels, n_thresholds) bytes, 8-byte aligned, the caller's; its
 * contents are unspecified before and after.  The library allocates nothing.
 * out_dev [n_timelines, n_thresholds, 3] int32, zeroed on `stream` first: tp = the size of a maximum matching of the hit graph
 * (exact: augmenting paths per pitch, no cap on the candidates of a note), n_est = the output notes kept under the threshold,
 * n_ref = the label notes.  A timeline that contains a row whose count is -1 gets tp = -1 (and no counts).  One launch serves all
 * thresholds.
 * M2M_ERR_INVALID: R, L, sequential, n_timelines, time_step, n_labels as m2m_score_chroma_counts; n_thresholds outside 1..64;
 * onset_tolerance or offset_min_tolerance outside [0, 3600] or NaN; offset_ratio NaN or above 1e6; a null notes / counts /
 * offsets / output pointer; null labels with n_labels > 0; a null note_lp_dev with n_thresholds > 1; a null min_logprobs_dev with
 * note_lp_dev; a null or misaligned workspace, or workspace_bytes below the need.
 */
int m2m_score_note_counts(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, int R, int L, int sequential,
                          double time_step, const double* labels_dev, const int32_t* label_offsets_dev, int n_labels, int n_timelines,
                          double onset_tolerance, double offset_ratio, double offset_min_tolerance, const float* min_logprobs_dev,
                          int n_thresholds, void* workspace_dev, int64_t workspace_bytes, int32_t* out_dev, void* stream);

#define M2M_SCORE_FRAME_TILE 1024          /* frames of one timeline per workgroup of the frame-roll kernels */

/*
 * Frame-level scoring (the definition: music2midi_amd/frame_metrics.py, frame_counts - ref music2midi/plot_midi.py:102-126
 * restated), per timeline and per confidence threshold.  Both note lists become piano rolls at 100 frames per second (a note sounds
 * in [int(start * 100), int(end * 100)), cut at n_frames - 1; n_frames as m2m_score_frame_count of the later end of both sides) and
 * every (pitch, frame) cell is a true positive (ref & est), a false negative (ref & ~est) or a false positive (~ref & est); the
 * melody roll has 12 rows and, in every frame where anything sounds, the row (highest sounding pitch % 12) set.
 * notes_dev .. frame_cap are m2m_score_chroma_counts', note_lp_dev / min_logprobs_dev / n_thresholds m2m_score_note_counts': output
 * note e exists under threshold k unless float32(on + off) < min_logprobs_dev[k] is true (a NaN total is kept); n_frames, and with
 * it the cut, is taken over the labels and the notes kept under k.
 * out_dev [n_timelines, n_thresholds, 6] int32, zeroed on `stream` first: tp, fn, fp of the full roll, tp, fn, fp of the melody roll.
 * frames_dev [n_timelines] int32: n_frames with every output note kept - or -1 (and no counts) for a timeline beyond frame_cap.
 * No workspace; one launch serves all thresholds.
 * M2M_ERR_INVALID: R, L, sequential, n_timelines, time_step, n_labels, frame_cap as m2m_score_chroma_counts; n_thresholds outside
 * 1..64; a null notes / counts / offsets / output / frames pointer; null labels with n_labels > 0; a null note_lp_dev with
 * n_thresholds > 1; a null min_logprobs_dev with note_lp_dev.
 */
int m2m_score_frame_counts(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, int R, int L, int sequential,
                           double time_step, const double* labels_dev, const int32_t* label_offsets_dev, int n_labels, int n_timelines,
                           int frame_cap, const float* min_logprobs_dev, int n_thresholds, int32_t* out_dev, int32_t* frames_dev,
                           void* stream);

/* The note slots per timeline and kind m2m_score_error_notes writes for these sizes: max_timeline_labels + L (sequential: + R * L),
 * twice that for the melody roll - a run of an error roll starts where a run of either side starts or ends, the melody's top pitch
 * changes only where a note starts or ends.  Host arithmetic; -1 for a size out of range. */
int m2m_score_error_notes_capacity(int R, int L, int sequential, int max_timeline_labels, int melody_only);

/* The bytes of workspace m2m_score_error_notes needs: per timeline 4, per timeline and tile (of M2M_SCORE_FRAME_TILE frames up to
 * frame_cap) 12, and the three bit-packed rolls, 128 (melody: 12) rows of 4 * 32 bytes per tile; every array rounded up to 8 bytes.
 * Host arithmetic; -1 for a size out of range. */
int64_t m2m_score_error_notes_workspace_bytes(int n_timelines, int frame_cap, int melody_only);

/*
 * The three error rolls of m2m_score_frame_counts as notes (frame_metrics.error_rolls + roll_to_notes, ref plot_midi.py:19-70),
 * for ONE threshold (min_logprob, -inf: every note; note_lp_dev may be NULL only then) and the full (melody_only 0) or the melody
 * roll (1).  Every maximal run of set cells of a row is one note, also across tiles.
 * notes_out_dev [n_timelines, 3, cap, 3] int32, cap = m2m_score_error_notes_capacity(R, L, sequential, max_timeline_labels,
 * melody_only): (first frame, end frame = last frame + 1, row) of the runs of tp / fn / fp, in the definition's order: ascending
 * end frame, then ascending row.  counts_out_dev [n_timelines, 3] int32: their number - or -1 (and nothing written) for a timeline
 * beyond frame_cap, with more than max_timeline_labels label notes, or (impossible by the bound) more runs than cap.
 * workspace_dev: at least m2m_score_error_notes_workspace_bytes(n_timelines, frame_cap, melody_only) bytes, 8-byte aligned, the
 * caller's; its contents are unspecified before and after.  Two launches on `stream`; the library allocates nothing.
 * M2M_ERR_INVALID: as m2m_score_frame_counts for the shared arguments; melody_only other than 0 / 1; max_timeline_labels outside
 * 0..2^24; a NaN min_logprob, or one above -inf without note_lp_dev; a null or misaligned workspace, or workspace_bytes below the need.
 */
int m2m_score_error_notes(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, int R, int L, int sequential,
                          double time_step, const double* labels_dev, const int32_t* label_offsets_dev, int n_labels, int n_timelines,
                          int frame_cap, float min_logprob, int melody_only, int max_timeline_labels, void* workspace_dev,
                          int64_t workspace_bytes, int32_t* notes_out_dev, int32_t* counts_out_dev, void* stream);

#define M2M_CONSENSUS_MAX_CANDIDATES 16    /* candidate rows per clip of the consensus calls */

/* The bytes of workspace m2m_consensus_pairwise_counts needs: 28 per note slot (R * L: three float64 and one int32 array) +
 * 16 per pair slot (R * (K - 1) * L: match, stamp, stack and interval, int32), every array rounded up to 8 bytes - 28 * R * L +
 * 16 * R * (K - 1) * L, 31 MB of pair slots at R = 128, L = 1024, K = 16.  Host arithmetic; -1 for a size out of range or an R
 * that is no multiple of K. */
int64_t m2m_consensus_workspace_bytes(int R, int L, int K);

/*
 * Pairwise note-level agreement of the K candidate rows of every clip (the definition: music2midi_amd/consensus.py,
 * pairwise_counts).  notes_dev [R, L, 3] / counts_dev [R] are m2m_score_detokenize's, batched (steps_per_row 0); the candidates of
 * clip b are rows b * K .. b * K + K - 1, B = R / K clips.  time_step and the three tolerances are m2m_score_note_counts'
 * (offset_ratio < 0: onsets only), and so are the hit test and the exact maximum matching: tp_out_dev [B, K, K] int32, zeroed on
 * `stream` first, holds at [b, i, j], i != j, the size of a maximum matching of the hit graph with candidate j as the reference
 * (its duration gives the offset tolerance) and candidate i as the estimate, and at [b, i, i] the kept notes (end > start) of
 * candidate i; n_out_dev [B, K] int32 holds those counts too.  A clip that contains a row whose count is -1 gets
 * tp_out_dev[b, 0, 0] = -1 and nothing else.
 * workspace_dev: at least m2m_consensus_workspace_bytes bytes for (R, L, K), 8-byte aligned, the caller's; its contents are
 * unspecified before and after, and nothing read from it was written by an earlier call.  One launch; the library allocates nothing.
 * M2M_ERR_INVALID: R, L, time_step and the tolerances as m2m_score_note_counts; K outside 2..16; R % K != 0; a null notes / counts
 * / output pointer; a null or misaligned workspace, or workspace_bytes below the need.
 */
int m2m_consensus_pairwise_counts(const int32_t* notes_dev, const int32_t* counts_dev, int R, int L, int K, double time_step,
                                  double onset_tolerance, double offset_ratio, double offset_min_tolerance, void* workspace_dev,
                                  int64_t workspace_bytes, int32_t* tp_out_dev, int32_t* n_out_dev, void* stream);

/*
 * The candidate the others agree with most (consensus.py, expected_agreement and select).  tp_dev [B, K, K] and n_dev [B, K] are
 * m2m_consensus_pairwise_counts'.  utility_out_dev [B, K] float64: u[i] = (sum over j != i, in increasing j, of a(i, j)) / (K - 1)
 * with a(i, j) = 1.0 when n[i] + n[j] == 0 and double(2 * tp[i, j]) / double(n[i] + n[j]) otherwise - float64, one rounded
 * operation each, the sum started at 0.0.  chosen_out_dev [B] int32: the first maximum of u.  A clip with tp[b, 0, 0] < 0 gets
 * chosen -1 and utilities 0.  One launch of one wave per clip.
 * M2M_ERR_INVALID: B outside 1..65535, K outside 2..16, a null pointer, a utility pointer that is not 8-byte aligned.
 */
int m2m_consensus_select(const int32_t* tp_dev, const int32_t* n_dev, int B, int K, int32_t* chosen_out_dev, double* utility_out_dev,
                         void* stream);

/* ------------------------------------------------------------------------- *
 * Audio ingest: the sample bytes of a WAVE file -> mono fp32 -> another sample rate, zero-padded; replaces, for the files it
 * takes, the host step of ref: music2midi/model.py:83-84 (librosa.load).  The definitions are music2midi_amd/audio.py (read_wav,
 * load_audio's y.mean(axis=1), resample = scipy.signal.resample_poly); the results are EQUAL to theirs for finite samples.
 * No handle, no workspace, no environment switch; both calls enqueue on `stream` and return nothing to the host.  Every
 * M2M_ERR_INVALID below is answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_INGEST_MAX_FRAMES (1 << 28)    /* frames / samples of one call's input */
#define M2M_INGEST_MAX_CHANNELS 7          /* from 8 channels up numpy's mean sums pairwise: those files stay on the host */
#define M2M_INGEST_MAX_RATIO 1000          /* up, down <= 1000: Fraction.limit_denominator(1000) */
#define M2M_INGEST_MAX_OUT (1 << 30)       /* samples of one call's output buffer */

enum {                                     /* sample formats: read_wav's */
  M2M_PCM_U8 = 0,                          /* (u8 - 128) / 128 */
  M2M_PCM_S16 = 1,                         /* i16 / 32768 */
  M2M_PCM_S24 = 2,                         /* sign-extended 24 bits / 8388608 */
  M2M_PCM_S32 = 3,                         /* (float)((double)i32 / 2147483648) */
  M2M_PCM_F32 = 4,
  M2M_PCM_F64 = 5                          /* (float)f64 */
};

/* ceil(n_in * up / down), the length of resample_poly's output; M2M_ERR_INVALID for n_in outside 0..2^28 or up / down outside
 * 1..1000.  Host arithmetic, exported so that the formula can be tested without a GPU. */
int64_t m2m_ingest_resampled_length(int64_t n_in, int up, int down);
/* J = 20 max(up, down) / up + 1: taps per phase of the phase-major filter below.  Host arithmetic. */
int m2m_ingest_phase_taps(int up, int down);

/*
 * out_dev[f] = mean over the channels of frame f, fp32 [n_frames]: the samples converted as above, summed in channel order in
 * fp32 from +0 and divided by the fp32 channel count - np.mean(axis=1) of read_wav's array for 1..7 channels.
 * bytes_dev: n_frames * channels interleaved little-endian samples; ANY address (a `data` chunk starts at any even offset, 24-bit
 * samples are never aligned): an address that is no multiple of the sample width is read byte by byte.
 * M2M_ERR_INVALID: n_frames outside 1..2^28, channels outside 1..7, an unknown format, a null pointer, out_dev overlapping the input.
 */
int m2m_ingest_pcm(const void* bytes_dev, int64_t n_frames, int channels, int format, float* out_dev, void* stream);

/*
 * out_dev[n] = sum_m x_dev[m] h[n down - m up + half] for n < n_out = ceil(n_in up / down), x zero outside [0, n_in), and 0 for
 * n_out <= n < capacity: scipy.signal.resample_poly(x, up, down) for fp32 x, zero-padded to `capacity` samples.  One fp32
 * accumulator per output, taps in ascending m, a rounded multiply then a rounded add (no FMA): upfirdn's order.
 * h = up * firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)) in fp32 is designed by the caller (the library designs
 * no filter) and handed over phase-major: h_phase_dev [up][J] fp32, J = m2m_ingest_phase_taps(up, down),
 * h_phase_dev[p][J - 1 - j] = h[p + j up], 0 where p + j up > 2 half.  up == down copies (bit-equal); h_phase_dev may be NULL then.
 * M2M_ERR_INVALID: n_in outside 1..2^28, up / down outside 1..1000 or not in lowest terms (unless equal), half other than
 * 10 max(up, down), capacity below n_out or above 2^30, a null pointer, out_dev [capacity] overlapping x_dev [n_in].
 */
int m2m_ingest_resample_f32(const float* x_dev, int64_t n_in, int up, int down, const float* h_phase_dev, int half, float* out_dev,
                            int64_t capacity, void* stream);

/* ------------------------------------------------------------------------- *
 * Training dataset: the segments of a batch, each cut from a different recording whose sample bytes lie in device memory, decoded,
 * downmixed and resampled by ONE launch - what ref: music2midi/dataset.py:124-129 (librosa.load(offset=, duration=)) does per
 * item on the host.  The definition is Music2MIDIDataset.crop_host (music2midi_amd/dataset.py): read_wav, the slice, y.mean(axis=1),
 * resample.  Every sample is EQUAL to what m2m_ingest_pcm followed by m2m_ingest_resample_f32 give for the clip's bytes alone: the
 * clip is resampled on its own, frames outside it do not exist for the filter.
 * No handle, no environment switch; the call enqueues on `stream` and returns nothing to the host.  Every M2M_ERR_INVALID below is
 * answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_DATASET_MAX_CLIPS 65535
#define M2M_DATASET_LDS_WINDOW 4096        /* floats of LDS for the input frames of one tile of 256 outputs (16 KiB) */

typedef struct {
  const void* bytes_dev;                   /* the clip's FIRST frame: n_frames * channels interleaved samples, any address */
  const float* h_phase_dev;                /* the phase-major filter of up / down as m2m_ingest_resample_f32 takes it; NULL when up == down */
  int64_t n_frames;                        /* frames of the clip, not of the recording */
  int32_t channels;                        /* 1..7 */
  int32_t format;                          /* M2M_PCM_* */
  int32_t up, down;                        /* in lowest terms, or equal */
  int32_t half;                            /* 10 max(up, down) */
  int32_t reserved;                        /* 0 */
} m2m_dataset_clip;

/* Input frames one tile of 256 outputs can touch: (up - 1 + 255 down) / up + J, J = m2m_ingest_phase_taps; 0 for up == down (no
 * filter, no window); M2M_ERR_INVALID for up / down outside 1..1000.  A ratio whose window exceeds M2M_DATASET_LDS_WINDOW is not
 * taken by the call below: the caller crops those recordings on the host.  Host arithmetic. */
int m2m_dataset_crop_window(int up, int down);

/*
 * out_dev[c * row_stride + n], c < n_clips, n < T: resample_poly(mean over the channels of clip c, up, down)[n] for
 * n < n_out(c) = ceil(n_frames up / down), exact zero for n_out(c) <= n < T.  Nothing outside these n_clips rows of T floats is written.
 * clips_host [n_clips] is copied to table_dev (device scratch of n_clips * sizeof(m2m_dataset_clip) bytes, 8-byte aligned) on
 * `stream`, then one launch of (ceil(T / 256), n_clips) workgroups follows; clips_host may be reused when the call returns.
 * M2M_ERR_INVALID: n_clips outside 1..65535, T outside 1..2^30, row_stride < T, a null pointer, table_dev misaligned; per clip:
 * n_frames outside 1..2^28, channels outside 1..7, an unknown format, n_frames * channels * width >= 2^31, up / down outside
 * 1..1000 or not in lowest terms (unless equal), half other than 10 max(up, down), a missing filter, n_out > T, a window above
 * M2M_DATASET_LDS_WINDOW, reserved != 0, the rows of out_dev overlapping the clip's bytes, its filter or table_dev.
 */
int m2m_dataset_crop_f32(const m2m_dataset_clip* clips_host, int n_clips, void* table_dev, float* out_dev, int64_t row_stride,
                         int64_t T, void* stream);

/* ------------------------------------------------------------------------- *
 * Rendering notes to audio: the packed notes of a batch of clips -> fp32 samples by ONE launch, a wavetable voice.  Stands in for
 * ref: webui.py:66 (PrettyMIDI.fluidsynth) and PrettyMIDI.synthesize, with a built-in timbre instead of a SoundFont.  The definition
 * is music2midi_amd/render.py (render_host); every sample is EQUAL to its: integer phase and decay arithmetic, then single rounded
 * fp32 operations in its order, nothing contracted, the notes of a sample added in packed order.
 * No handle, no workspace, no environment switch; the call copies nothing, enqueues one kernel on `stream` and returns nothing to
 * the host.  Every M2M_ERR_INVALID below is answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_RENDER_MAX_SAMPLES (1 << 28)
#define M2M_RENDER_MAX_NOTES (1 << 20)     /* packed notes of one call, all clips together */
#define M2M_RENDER_MAX_CLIPS 65535
#define M2M_RENDER_MAX_RAMP (1 << 24)      /* attack, release and decay steps: fp32 holds every integer up to it */

typedef struct {
  int32_t on;                              /* first sample, may be negative (>= -2^30): k = n - on */
  int32_t off;                             /* release begins here; min(off, n_samples) */
  uint32_t inc;                            /* phase step per sample, 2^32 = one period */
  uint32_t dec;                            /* decay steps per sample in units of 2^-16 */
  int32_t table;                           /* row of wave_dev, 0..n_tables - 1 */
  float gain;
} m2m_render_note;

typedef struct {
  const float* wave_dev;                   /* [n_tables][table_size + 1], entry table_size of a row equal to its entry 0 */
  const float* decay_dev;                  /* [decay_steps + 1] */
  int32_t table_size;                      /* a power of two, 256..65536 */
  int32_t n_tables;                        /* 1..64 */
  int32_t decay_steps;                     /* J, 1..2^24 */
  int32_t attack, release;                 /* A, R in samples, 1..2^24 */
  int32_t reserved;                        /* 0 */
} m2m_render_voice;

/* Output samples per workgroup: the tile of the lists below.  Host arithmetic. */
int m2m_render_tile(void);

/*
 * out_dev[c * row_stride + n], c < n_clips, n < n_samples: the sum, from +0 and in list order, over the notes of tile
 * (c, n / tile) with on <= n < min(off + release, n_samples) of (((w e) att) rel) gain, k = n - on:
 *   phase = (uint32)(k inc), s = 32 - log2 table_size, i = phase >> s, fr = (float)(phase & (2^s - 1)) 2^-s, W = row `table`,
 *   w = W[i] + fr (W[i + 1] - W[i]);  u = (uint64)k dec, j = u >> 16, ef = (float)(u & 0xFFFF) 2^-16,
 *   e = E[j] + ef (E[j + 1] - E[j]) for j < decay_steps, else E[decay_steps];
 *   att = (float)min(k + 1, attack) (1.0f / attack);  rel = 1 for n < off, else (float)(release - (n - off)) (1.0f / release).
 * Every sample of the n_clips rows is written (a tile without notes: zeros), nothing outside them.
 * notes_dev [n_notes]; tile_start_dev int32 [n_clips * tiles + 1], tiles = ceil(n_samples / tile), ascending from 0 to n_entries:
 * the notes of tile t of clip c are tile_notes_dev[tile_start_dev[c * tiles + t] .. tile_start_dev[c * tiles + t + 1]), int32
 * indices into notes_dev (an index outside it is clamped, a table outside the voice likewise).  With n_notes = 0, notes_dev and
 * tile_notes_dev may be null.
 * M2M_ERR_INVALID: n_samples outside 1..2^28, n_clips outside 1..65535, n_notes outside 0..2^20, n_entries outside 0..2^31 - 1 or
 * positive without notes, row_stride < n_samples, attack or release outside 1..2^24, a table_size that is not a power of two in
 * 256..65536, n_tables outside 1..64, decay_steps outside 1..2^24, reserved != 0, a null pointer, a pointer that is not 4-byte aligned.
 */
int m2m_render_notes_f32(const m2m_render_note* notes_dev, int n_notes, const int32_t* tile_start_dev, const int32_t* tile_notes_dev,
                         int64_t n_entries, const m2m_render_voice* voice, float* out_dev, int64_t n_samples, int64_t row_stride,
                         int n_clips, void* stream);

/* ------------------------------------------------------------------------- *
 * Aligning note labels to a recording: integer chroma / onset features of log band energies and batched DTW.  Stands in for the
 * feature and DTW stages of ref: data/align_audio_midi.py.  This is the project's own aligner, not synctoolbox's; the definition is
 * music2midi_amd/align.py (features_host, coarse, cost_matrix, dtw_host) and every output below is EQUAL to its: one fp32
 * subtraction before each comparison of the features, integer arithmetic everywhere else.
 * No handle, no environment switch; the calls enqueue on `stream` and return nothing to the host.  Every M2M_ERR_INVALID below is
 * answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_ALIGN_MAX_FRAMES 32768         /* a side of one DTW problem: 10.9 min at 50 frames per second */
#define M2M_ALIGN_MAX_CLIPS 65535
#define M2M_ALIGN_MAX_PROBLEMS 65535
#define M2M_ALIGN_MAX_TOTAL_FRAMES (1 << 26)   /* frames of one features call, all clips together */

/*
 * L_dev fp32 [total_frames, 88]: the log energies of the 88 bands (MIDI 21..108) of all clips, those of clip b at rows
 * [frame_offsets_dev[b], frame_offsets_dev[b + 1]) (int32 [n_clips + 1]; offsets outside 0..total_frames are clamped); finite.
 * max_frames: the longest clip (the launch geometry).  chroma_out_dev, onset_out_dev uint8 [total_frames, 12], per frame t of a clip
 * with d = (float)(ln 2.5, ln 5, ln 10, ln 20), M = max_p L[t][p], silent when M <= -6.0f (all twelve of both are then 0):
 *   chroma[c] = sum over the bands p of class c ((21 + p) % 12 == c) of #{k : L[t][p] >= M - d[k]};
 *   on[t][p] = t >= 2 and L[t][p] - L[t-2][p] >= (float)ln 4 and L[t][p] >= M - d[3] and not silent; first = on[t] and not on[t-1];
 *   onset[c] = max over tau = 0..3 of (4 - tau) * (sum over the bands of class c of first[t - tau]).
 * M2M_ERR_INVALID: n_clips outside 1..65535, total_frames outside 1..2^26, max_frames outside 1..total_frames, a null pointer,
 * L_dev or frame_offsets_dev not 4-byte aligned.
 */
int m2m_align_features(const float* L_dev, const int32_t* frame_offsets_dev, int n_clips, int max_frames, int64_t total_frames,
                       uint8_t* chroma_out_dev, uint8_t* onset_out_dev, void* stream);

/*
 * out_dev int32 [total_coarse, 12]: row j of clip b (rows [coarse_offsets_dev[b], coarse_offsets_dev[b + 1])) is the sum of the W
 * chroma frames centred on frame j * D of the clip (W / 2 before it), zeros outside the clip.  max_coarse: the most rows of a clip.
 * M2M_ERR_INVALID: n_clips outside 1..65535, total_frames outside 1..2^26, total_coarse outside 1..total_frames, max_coarse outside
 * 1..total_coarse, W or D outside 1..255, a null pointer, a table or out_dev not 4-byte aligned.
 */
int m2m_align_coarse(const uint8_t* chroma_dev, const int32_t* frame_offsets_dev, const int32_t* coarse_offsets_dev, int n_clips,
                     int max_coarse, int64_t total_frames, int64_t total_coarse, int W, int D, int32_t* out_dev, void* stream);

typedef struct {
  int32_t a_offset;                        /* first frame of side a (the rows) in the a arrays */
  int32_t n;                               /* frames of side a, 1..32768 */
  int32_t b_offset;                        /* first frame of side b (the columns) in the b arrays */
  int32_t m;                               /* frames of side b, 1..32768 */
  int32_t shift;                           /* 0..11: class c of side b takes class (c - shift) mod 12, np.roll(b, shift, axis=1) */
  int32_t path_offset;                     /* first point of this problem's path in path_out_dev; n + m - 1 points are reserved */
} m2m_align_problem;

/* Columns of a strip of the DTW kernel (its workgroup's threads).  Host arithmetic. */
int m2m_align_dtw_strip(void);
/* Bytes of workspace m2m_align_dtw needs for problems of rows_host[p] x cols_host[p] frames: the problem table, then per problem
 * two direction bits per cell and a scratch path.  M2M_ERR_INVALID (negative) for n_problems outside 1..65535 or a side outside
 * 1..32768.  Host arithmetic. */
int64_t m2m_align_dtw_workspace_bytes(const int32_t* rows_host, const int32_t* cols_host, int n_problems);

/*
 * n_problems DTW problems by ONE launch, one workgroup each.  Cell (i, j) of a problem costs, with S = 256 and
 * cost(u, v) = S - isqrt((S S (u.v)^2) / ((u.u) (v.v))) (S when a vector is zero), u frame a_offset + i of side a and v frame
 * b_offset + j of side b rolled by `shift`:
 *   coarse = 1: cost of a0_dev / b0_dev, int32 [frames, 12] with values 0..672 (a1_dev / b1_dev are not read; pass a0_dev / b0_dev);
 *   coarse = 0: cost of a0_dev / b0_dev (chroma) + cost of a1_dev / b1_dev (onset), uint8 [frames, 12].
 * D[-1][-1] = 0, the other border cells +inf; D[i][j] = min(D[i-1][j-1] + 4 C, D[i-1][j] + 3 C, D[i][j-1] + 3 C), a tie takes the
 * diagonal, then (i-1, j), then (i, j-1).  total_out_dev[p] = D[n-1][m-1]; the path from (0, 0) to (n-1, m-1), front to back, has
 * path_len_out_dev[p] points: its rows at path_out_dev[path_offset + k], its columns at path_out_dev[path_capacity + path_offset + k].
 * problems_host is copied to the head of workspace_dev on `stream`; it must stay valid until that copy has run.
 * M2M_ERR_INVALID: n_problems outside 1..65535, coarse other than 0 or 1, a side outside 1..32768, frames outside the arrays
 * (a_frames, b_frames), a shift outside 0..11, path regions that are not ascending and disjoint or exceed path_capacity
 * (1..2^31 - 1), a null pointer, feature arrays not 16-byte (coarse) / 4-byte aligned, a workspace not 256-byte aligned.
 * M2M_ERR_NOMEM: workspace_bytes below m2m_align_dtw_workspace_bytes.
 */
int m2m_align_dtw(const void* a0_dev, const void* a1_dev, int a_frames, const void* b0_dev, const void* b1_dev, int b_frames, int coarse,
                  const m2m_align_problem* problems_host, int n_problems, void* workspace_dev, int64_t workspace_bytes,
                  int32_t* total_out_dev, int32_t* path_out_dev, int64_t path_capacity, int32_t* path_len_out_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * Beat tracking: an onset envelope of log band energies, a tempo from its autocorrelation, the beats by a dynamic program.  This is
 * the project's own tracker in the family of Ellis (2007), not librosa's or madmom's; the definition is music2midi_amd/beats.py
 * (onset_envelope_host, track_envelope_host) and every output below is EQUAL to its: one fp32 subtraction, one scaling by 16 and one
 * truncation per band of the envelope, integer arithmetic everywhere else.  Every transcendental number is a table the caller passes.
 * No handle, no environment switch; the calls enqueue on `stream` and return nothing to the host.  Every M2M_ERR_INVALID below is
 * answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_BEAT_MAX_FRAMES 32768          /* frames of one clip: 10.9 min at 50 frames per second */
#define M2M_BEAT_MAX_CLIPS 65535
#define M2M_BEAT_MAX_TOTAL_FRAMES (1 << 26) /* frames of one call, all clips together */
#define M2M_BEAT_LAG_MIN 15                /* periods in frames: 200 BPM .. */
#define M2M_BEAT_LAG_MAX 100               /* .. 30 BPM */
#define M2M_BEAT_HALF 12                   /* the novelty's local sum reaches this many frames to either side */
#define M2M_BEAT_ENV_MAX 22440             /* the largest envelope value: 88 bands of 255 */

/*
 * L_dev fp32 [total_frames, 88] and frame_offsets_dev as in m2m_align_features.  env_out_dev int32 [total_frames]; frame t of a clip,
 * with M = max_p L[t][p]: 0 when t = 0 or M <= -6.0f, otherwise the sum over the bands with L[t][p] >= M - (float)ln 20 of
 * (int)min(max(L[t][p] - L[t-1][p], 0.0f) * 16.0f, 255.0f).
 * M2M_ERR_INVALID: n_clips outside 1..65535, total_frames outside 1..2^26, max_frames outside 1..total_frames, a null pointer, a
 * pointer that is not 4-byte aligned.
 */
int m2m_beat_envelope(const float* L_dev, const int32_t* frame_offsets_dev, int n_clips, int max_frames, int64_t total_frames,
                      int32_t* env_out_dev, void* stream);

typedef struct {
  int32_t env_offset;                      /* first frame of the clip in env_dev */
  int32_t frames;                          /* 1..32768 */
  int32_t period;                          /* 0: estimate the period; 15..100: use this one */
  int32_t beat_offset;                     /* first beat of the clip in beats_out_dev; frames / 8 + 2 entries are reserved */
} m2m_beat_clip;

/* Bytes of workspace m2m_beat_track needs for clips of frames_host[b] frames: the clip table, then the novelty of every frame.
 * M2M_ERR_INVALID (negative) for n_clips outside 1..65535 or a clip outside 1..32768 frames.  Host arithmetic. */
int64_t m2m_beat_track_workspace_bytes(const int32_t* frames_host, int n_clips);

/*
 * n_clips envelopes (env_dev int32 [env_frames], values 0..22440) by ONE launch, one workgroup each.  With e zero outside the clip
 * and F its frames:
 *   o[t] = max(0, 25 e[t] - sum_{|k| <= 12} e[t + k]);
 *   a[k] = (sum_{t >= k} o[t] o[t - k]) / (F - k) for k = 15..min(200, F - 1), 0 for every other lag; 64-bit integers;
 *   score[l] = (a[l] + a[2 l] / 2) * prior_dev[l] for l = 15..100 (prior_dev int32 [101]), 0 below 15;
 *   P = the clip's period when that is not 0; otherwise the first maximum of score, default_period when that maximum is 0;
 *   s = (sum of o) / max(1, #{o > 0});  pen[tau] = (penalty_dev[P * 201 + tau] * s) >> 8 (penalty_dev int32 [101, 201], not negative);
 *   lo = (P + 1) / 2, hi = 2 P;  C[t] = o[t] for t < lo, else o[t] + max over tau = lo..min(hi, t) of (C[t - tau] - pen[tau]), the
 *   smallest tau on a tie, back[t] = t - tau;  the last beat is the first maximum of C over [max(0, F - P), F), the beats the chain
 *   of back from there in ascending order; no beats when every o is 0.
 * period_out_dev int32 [n_clips]: P.  score_out_dev int64 [n_clips, 101], may be null.  beats_out_dev int32 [beat_capacity]: the
 * beats of clip b from beat_offset on, n_beats_out_dev[b] of them (at most frames / 8 + 1).
 * clips_host is copied to the head of workspace_dev on `stream`; it must stay valid until that copy has run.
 * M2M_ERR_INVALID: n_clips outside 1..65535, a clip outside 1..32768 frames or outside env_frames (1..2^26), a period that is neither
 * 0 nor in 15..100, default_period outside 15..100, beat regions that are not ascending and disjoint or exceed beat_capacity
 * (1..2^31 - 1), a null pointer other than score_out_dev, a table or output not 4-byte (score_out_dev: 8-byte) aligned, a workspace
 * not 256-byte aligned.  M2M_ERR_NOMEM: workspace_bytes below m2m_beat_track_workspace_bytes.
 */
int m2m_beat_track(const int32_t* env_dev, int64_t env_frames, const m2m_beat_clip* clips_host, int n_clips, const int32_t* prior_dev,
                   const int32_t* penalty_dev, int default_period, void* workspace_dev, int64_t workspace_bytes, int32_t* period_out_dev,
                   int64_t* score_out_dev, int32_t* beats_out_dev, int64_t beat_capacity, int32_t* n_beats_out_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * Tokenising of note labels: the note arrays of a batch -> token ids, replaces for the batches it takes
 * ref: music2midi/tokenizer.py:86-141 (MidiTokenizer.__call__, _tokenize).  The definition is music2midi_amd/tokenizer.py
 * (_quantize, _tokenize); the ids are EQUAL to its (integer placement; the quantisation repeats the host's float64 operations).
 * No handle, no workspace, no environment switch; the call enqueues on `stream` and returns nothing to the host.  Every
 * M2M_ERR_INVALID below is answered on the arguments alone, before the first HIP call.
 * ------------------------------------------------------------------------- */
#define M2M_TOKENIZE_MAX_NOTES 1024        /* notes per clip */
#define M2M_TOKENIZE_MAX_TIME 4096         /* time ids of the vocabulary */
#define M2M_TOKENIZE_MAX_ROWS 65535

/* MidiTokenizer._quantize: min(rint(nextafter(seconds / time_step, +inf)), n_time - 1) in double, the function the kernel calls;
 * -1 for seconds that are negative or NaN, a time_step outside (0, 3600] or n_time outside 1..4096.  Host arithmetic, exported so
 * that the formula can be tested without a GPU. */
int m2m_tokenize_quantize(double seconds, double time_step, int n_time);
/* 1 + 2k + min(2k, T) + 2 min(k, T): the longest row k = n_notes notes can give over T = n_time time ids (6k + 1 when every onset
 * and offset has an index of its own); -1 for k < 0 or T < 1.  Host arithmetic. */
int64_t m2m_tokenize_row_bound(int n_notes, int n_time);

/*
 * MidiTokenizer.__call__(notes_batch, cutoff_time) without the host loop, one workgroup per clip.
 * notes_dev [3, n_notes] float64: onsets (s), offsets (s), pitches of all clips, those of clip r at
 * [offsets_dev[r], offsets_dev[r + 1]) (int32 [B + 1]) in array order; the velocity is not part of the vocabulary.
 * Per clip: notes with onset < cutoff_time are kept (has_cutoff = 0: all); offset = max(offset, onset + time_step); both times go
 * through m2m_tokenize_quantize; for every distinct index in increasing order the row takes time_offset + index, then ONSET (3) and
 * the pitch ids of the notes starting there, then OFFSET (4) and those of the notes ending there, both in array order; EOS (2) ends
 * the row.  A pitch id is (int64)(float)(pitch + pitch_offset), a time id (int64)(float)(index + time_offset): the host builds a
 * float32 tensor and truncates it.  labels = 1 writes -100 for every id equal to pad_id (Music2MIDI._labels).
 * ids_out_dev [B, row_stride] int64: row r holds its lengths_out_dev[r] ids, then `fill` up to `width`; columns from `width` on are
 * not touched.  A row longer than `width` is cut at `width` and keeps its true length in lengths_out_dev [B] int32, so the caller
 * can tell.  lengths_out_dev[r] = -1, and the row all `fill`, for a clip with a value that cannot be placed - an onset, offset or
 * pitch that is not finite, a negative onset, |pitch| > 32768 - or with offsets outside 0..n_notes or more than 1024 notes apart.
 * M2M_ERR_INVALID: B outside 1..65535, n_notes outside 0..1024 B, time_step outside (0, 3600], n_time outside 1..4096,
 * pitch_offset < 5, time_offset outside pitch_offset..2^30, has_cutoff / labels other than 0 or 1, width < 1, row_stride < width,
 * a null pointer.
 */
int m2m_tokenize_notes(const double* notes_dev, const int32_t* offsets_dev, int n_notes, int B, double time_step, int pitch_offset,
                       int time_offset, int n_time, int has_cutoff, double cutoff_time, int64_t fill, int labels, int64_t pad_id,
                       int64_t* ids_out_dev, int width, int64_t row_stride, int32_t* lengths_out_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * T5 encoder-decoder weights, replaces what ref: music2midi/transformer.py:14-16
 * builds (T5Config + T5ForConditionalGeneration) once a state dict is loaded.
 * ------------------------------------------------------------------------- */
typedef struct {
  int d_model, d_ff, num_layers, num_decoder_layers, num_heads, d_kv;
  int vocab_size, num_buckets, max_distance;
  int pad_token_id, eos_token_id, decoder_start_token_id;
  float layer_norm_eps;
} m2m_t5_geometry;

/* All pointers: DEVICE, fp32, HuggingFace layout ([out_features, in_features]). */
typedef struct {
  const float *ln0, *q, *k, *v, *o;             /* layer.0.layer_norm, SelfAttention.{q,k,v,o} */
  const float *ln1, *wi0, *wi1, *wo;            /* layer.1.layer_norm, DenseReluDense.{wi_0,wi_1,wo} */
} m2m_enc_layer_weights;

typedef struct {
  const float *ln0, *q, *k, *v, *o;             /* layer.0: self attention */
  const float *ln1, *cq, *ck, *cv, *co;         /* layer.1: EncDecAttention.{q,k,v,o} */
  const float *ln2, *wi0, *wi1, *wo;            /* layer.2: DenseReluDense */
} m2m_dec_layer_weights;

typedef struct {
  const float* shared;            /* [V, d_model] token embedding */
  const float* lm_head;           /* [V, d_model] separate tensor (transformers 4.34 untied head) */
  const float* enc_rel_bias;      /* [num_buckets, H] encoder.block.0 relative_attention_bias */
  const float* dec_rel_bias;      /* [num_buckets, H] decoder.block.0 relative_attention_bias */
  const float* enc_final_ln;      /* [d_model] */
  const float* dec_final_ln;      /* [d_model] */
  const m2m_enc_layer_weights* enc;  /* host array [num_layers] */
  const m2m_dec_layer_weights* dec;  /* host array [num_decoder_layers] */
} m2m_t5_weights;

typedef struct m2m_model m2m_model;

/* Repacks the weights into kernel layouts (device-side kernels on `stream`,
 * synchronised before returning); the source tensors may be freed afterwards.
 * Creation also writes the decoder's layer-0 token tables into the same blob: the
 * layer-0 self-attention's q (fp32) and k, v (storage type) of every (head, token),
 * [num_heads][vocab_size][64] each, which the greedy decode step reads instead of
 * projecting (M2M_DEC_TOKEN_TABLES, read when a session is
 * created: 0 off, 1 this step's q / k / v, 2 the cached K/V rows as well; default 2).  A model whose tables
 * would exceed 16 MB, or whose vocabulary is above 65 535, has none and decodes as
 * with 0.  m2m_model_param_bytes and m2m_model_checksum include them. */
int  m2m_model_create(const m2m_t5_geometry* geom, const m2m_t5_weights* w, int precision,
                      void* stream, m2m_model** out);
void m2m_model_destroy(m2m_model* m);
int  m2m_model_precision(const m2m_model* m);
int64_t m2m_model_param_bytes(const m2m_model* m);   /* bytes of repacked weights held */
/* 64-bit position-weighted checksum of the repacked device weights (sum of word_i * (2 i + 1) mod 2^64 over the
 * whole packed blob), synchronised before returning.  After the one-time weight broadcast of a multi-GPU run
 * (ref: train.py:40-41 strategy="ddp") every rank's value must be equal: the ranks all-reduce MIN and
 * MAX of it and fail loudly on a difference instead of decoding from diverged replicas. */
int  m2m_model_checksum(const m2m_model* m, uint64_t* out_host, void* stream);

/* T5 relative-position bucket (hf: models/t5/modeling_t5.py:217-262), host-side,
 * exported so the integer table can be tested without a GPU. rel = key_pos - query_pos. */
int m2m_rel_bucket(int rel, int bidirectional, int num_buckets, int max_distance);

/* ------------------------------------------------------------------------- *
 * Session: workspace + captured decode-step graph for up to (max_batch,
 * max_enc_len, max_dec_len).  One session per concurrent call; a session is
 * not re-entrant.  The workspace is caller-owned device memory.
 * ------------------------------------------------------------------------- */
typedef struct m2m_session m2m_session;

int64_t m2m_session_workspace_bytes(const m2m_model* m, int max_batch, int max_enc_len, int max_dec_len);
int  m2m_session_create(const m2m_model* m, int max_batch, int max_enc_len, int max_dec_len,
                        void* workspace_dev, int64_t workspace_bytes, m2m_session** out);
void m2m_session_destroy(m2m_session* s);

/*
 * Encoder stack + cross-attention K/V projection for every decoder layer,
 * replaces the encoder half of ref: music2midi/transformer.py:44 (HF generate
 * runs the encoder once, hf: generation/utils.py:809-848) and of :35-37.
 * inputs_embeds_dev [B, S, d_model] fp32 (cond rows + log-mel rows).
 * enc_out_dev: optional [B, S, d_model] fp32 copy of the final encoder states (NULL to skip).
 */
int m2m_encode(m2m_session* s, const float* inputs_embeds_dev, int B, int S, float* enc_out_dev, void* stream);

/*
 * KV-cached greedy decode, replaces the decode half of
 * ref: music2midi/transformer.py:44 (hf: generation/utils.py:2783-2973, do_sample=False):
 * start token decoder_start_token_id, argmax, rows that emitted EOS keep emitting
 * pad, stop when every row has finished or the length reaches max_length.
 * tokens_out_dev [B, max_length] int64 (columns >= *out_len_host are pad).
 * *out_len_host: number of valid columns L <= max_length.  This call synchronises `stream`.
 * Returns M2M_ERR_RANGE (tokens are still written) when an activation left the decoder's fixed-point range or
 * was not finite - where the fp32 reference would have produced Inf/NaN logits.  On every error return all
 * library-owned streams have been synchronised, so the caller may free or reuse the workspace at once.
 *
 * Session state afterwards: m2m_encode -> any number of m2m_decode_forced / m2m_generate_greedy / m2m_bench_kernel calls on the same
 * encode is legal (HF's forward and generate share one encoder pass the same way, ref: music2midi/transformer.py:28-45) - EXCEPT
 * that a greedy decode which re-packed its live rows (m2m_session_repack_stats reports rows_moved > 0, see below) has overwritten
 * finished clips' cross K/V with live ones and thereby CONSUMED the encode: the next call that needs it returns M2M_ERR_STATE
 * ("re-encode: ...") until m2m_encode runs again.  The token ids of the call itself are unaffected.
 */
int m2m_generate_greedy(m2m_session* s, int max_length, int64_t* tokens_out_dev, int* out_len_host, void* stream);

/*
 * KV-cached sampled decode (hf: generation/utils.py sample(), do_sample=True): the greedy loop above with the arg-max replaced by
 * transformers 4.34's logits warpers in their order - temperature (logits / T, skipped for T == 1), top-k (every logit strictly
 * below the k-th largest is removed, k = min(top_k, V); top_k = 0 disables it), top-p (sorted ascending, the entries whose
 * cumulative softmax is <= 1 - top_p are removed, the largest always stays; top_p = 1 disables it) - and a draw from the softmax
 * of what is left.  The uniform of clip row r at position t hashes (seed, r, t), so the same seed gives the same ids whatever the
 * chain split, the live-row re-packing or the kernel forms; the ids are not HF's samples (another random generator).
 * Invalid parameters return M2M_ERR_INVALID: temperature <= 0 or not finite, top_k < 0, top_p outside [0, 1]; so does a vocabulary
 * larger than 4096.  Everything else - arguments, out_len, M2M_ERR_RANGE, the re-packing and the session state afterwards - is as
 * for m2m_generate_greedy.
 */
typedef struct {
  float temperature;
  int top_k;
  float top_p;
  uint64_t seed;
} m2m_sample_params;

int m2m_generate_sample(m2m_session* s, int max_length, const m2m_sample_params* p, int64_t* tokens_out_dev, int* out_len_host,
                        void* stream);

/*
 * KV-cached beam search (hf: generation/utils.py _beam_search, generation/beam_search.py BeamSearchScorer / BeamHypotheses,
 * transformers 4.34 read for an encoder-decoder; this export applies no logits processor - the token grammar and the processors
 * that do not read a row's history come with m2m_generate_beam_processed below): each of the B encoded clips is decoded as
 * num_beams rows.  Every step scores log_softmax(logits) + the running beam score (fp32), takes the clip's top 2 num_beams over
 * num_beams x V (ties to the lower beam-major index) and walks them in rank order: an EOS of rank < num_beams becomes a hypothesis
 * (score sum_logprobs / len ** length_penalty, len = the start token plus the generated tokens, EOS not counted; at most
 * num_beams kept per clip), an EOS of rank >= num_beams is dropped, any other candidate is the next running beam until there are
 * num_beams.  A clip is done once it holds num_beams hypotheses and early_stopping is 1 (True), or the worst of them reaches the best
 * running score of the step divided by cur_len ** length_penalty (0, False) - by max_length ** length_penalty instead when
 * length_penalty > 0 (2, "never").  The loop ends when every clip is done or at max_length; a clip that is not done then adds its
 * running beams at length max_length.
 * Output (finalize): the best num_return_sequences = n hypotheses of clip c, best first (the later-added first among equal
 * scores), in rows c * n .. c * n + n - 1 of tokens_out_dev [B * n, max_length] (row pitch max_length): the hypothesis, EOS at
 * column len when len < max_length, pad_token_id after.  *out_len_host = min(longest returned hypothesis + 1, max_length): the
 * columns HF returns.  scores_out_dev (optional, may be NULL) [B * n] receives the hypotheses' scores (HF sequences_scores).
 * The session needs max_batch >= B * num_beams.  The self-attention reads a beam's K/V through its ancestry (the slot of every
 * cached position) instead of copying caches; the beams of a clip share its cross K/V; live rows are NOT re-packed, so the encode
 * stays valid for a later m2m_generate_greedy / m2m_decode_forced.  Invalid parameters return M2M_ERR_INVALID without launching
 * anything: num_beams outside [2, 32], num_return_sequences outside [1, num_beams], early_stopping outside {0, 1, 2}, a
 * non-finite length_penalty, a vocabulary larger than 4096 or smaller than 2 num_beams, B * num_beams > max_batch.  Non-finite
 * logits return M2M_ERR_RANGE as m2m_generate_greedy does.
 */
typedef struct {
  int num_beams;
  float length_penalty;
  int early_stopping;       /* 0 False, 1 True, 2 "never" */
  int num_return_sequences;
} m2m_beam_params;

int m2m_generate_beam(m2m_session* s, int max_length, const m2m_beam_params* p, int64_t* tokens_out_dev, float* scores_out_dev,
                      int* out_len_host, void* stream);

/*
 * KV-cached greedy or sampled decode with transformers 4.34's logits processors (hf: generation/utils.py _get_logits_processor for
 * an encoder-decoder, generation/logits_process.py).  input_ids are the decoder ids so far: the start token and the t generated
 * ids at step t, cur_len = t + 1.  The processors change the raw logits of every row at every step, in this order:
 *   repetition_penalty != 1   every id present in input_ids (the start token included): logit < 0 -> logit * p, else logit / p
 *   no_repeat_ngram_size n>0  -inf for every id that would complete an n-gram already in input_ids
 *   bad_words                 a sequence equal to [eos_token_id] is dropped; a one-id sequence -> -inf at every step; a longer one
 *                             -> -inf on its last id when input_ids end with the others (skipped while it is longer than input_ids)
 *   min_length                EOS -> -inf while cur_len < min_length
 *   min_new_tokens            EOS -> -inf while cur_len - 1 < min_new_tokens
 *   forced_bos_token_id       at cur_len == 1 every id but it -> -inf, it -> 0
 *   forced_eos_token_id       at cur_len == max_length - 1 every id but it -> -inf, it -> 0
 *   suppress_tokens           -> -inf at every step
 *   begin_suppress_tokens     -> -inf at cur_len == 2 with forced_bos_token_id set, at cur_len == 1 without
 * then select: sample == NULL takes the arg-max (ties to the lower id), otherwise m2m_generate_sample's warpers and draw follow
 * (same seed semantics).  1.0 / 0 / -1 / an empty list leave a processor out; the history of a row is the clip's own token row, so
 * ids do not depend on the live-row re-packing or the chain split.  Non-finite RAW logits return M2M_ERR_RANGE (the -inf of the
 * processors is legal).
 * Invalid parameters return M2M_ERR_INVALID without launching anything: repetition_penalty <= 0 or not finite, a negative
 * no_repeat_ngram_size / min_length / min_new_tokens / count, a forced id outside [-1, V), a listed id outside [0, V), a null list
 * with a non-zero count, a bad-words sequence of length < 1, invalid sample parameters (as m2m_generate_sample), and the device
 * limits: a vocabulary larger than 4096, max_length > 2048, more than 64 bad-words sequences of two or more ids or more than 512
 * ids in them.  bad_words_ids holds the n_bad_words sequences concatenated, bad_words_lengths their lengths.  Everything else -
 * arguments, out_len, M2M_ERR_RANGE, the re-packing and the session state afterwards - is as for m2m_generate_greedy.
 */
typedef struct {
  float repetition_penalty;               /* > 0; 1 = off */
  int no_repeat_ngram_size;               /* >= 0; 0 = off */
  int min_length;                         /* >= 0; 0 = off */
  int min_new_tokens;                     /* >= 0; 0 = off */
  int forced_bos_token_id;                /* -1 = off */
  int forced_eos_token_id;                /* -1 = off */
  const int32_t* suppress_tokens;
  int n_suppress_tokens;
  const int32_t* begin_suppress_tokens;
  int n_begin_suppress_tokens;
  const int32_t* bad_words_ids;           /* the sequences concatenated */
  const int32_t* bad_words_lengths;       /* [n_bad_words] */
  int n_bad_words;
} m2m_process_params;

int m2m_generate_processed(m2m_session* s, int max_length, const m2m_process_params* proc, const m2m_sample_params* sample,
                           int64_t* tokens_out_dev, int* out_len_host, void* stream);

/*
 * The same decode with per-token outputs (hf: generate(return_dict_in_generate=True, output_scores=True) and
 * compute_transition_scores(normalize_logits=True)).  proc == NULL: no logits processor; sample == NULL: the arg-max (ids equal to
 * m2m_generate_greedy's); both follow m2m_generate_processed / m2m_generate_sample otherwise.  For the token clip c selects at
 * step t (column t + 1 of its token row), written while the row is in registers for the select:
 *   scores_out_dev   (optional) [max_length - 1, B, V] fp32: the row the token was selected from, as HF appends it to `scores` -
 *                    the raw logits (greedy), the logits after the processors, or after processors, temperature, top-k and top-p
 *                    with the removed entries at -inf (sampling);
 *   logprobs_out_dev (optional) [B, max_length - 1] fp32: log_softmax(that row)[token].  Asked for alone, no V-wide row is written.
 * Both are zeroed on `stream` first; a row that finished before step t (it emits pad) writes nothing and stays 0 - HF runs the
 * model on finished rows and returns their logits.  The outputs follow the clip, not its slot: the live-row re-packing and the
 * chain split do not change them.  With both outputs NULL this is the matching unscored export.  Checks and error codes are those
 * of m2m_generate_processed (when proc is given) and m2m_generate_sample (when sample is given); a vocabulary larger than 4096
 * returns M2M_ERR_INVALID.  Everything else - out_len, M2M_ERR_RANGE, the re-packing and the session state afterwards - is as for
 * m2m_generate_greedy.
 */
int m2m_generate_scored(m2m_session* s, int max_length, const m2m_process_params* proc, const m2m_sample_params* sample,
                        int64_t* tokens_out_dev, float* scores_out_dev, float* logprobs_out_dev, int* out_len_host, void* stream);

/*
 * The same decode constrained to the MIDI token grammar (music2midi_amd/grammar.py; hf: generate(prefix_allowed_tokens_fn=...),
 * PrefixConstrainedLogitsProcessor): at every step the ids that may not follow the row's prefix go to -inf, after the min_length /
 * min_new_tokens bans and before forced_bos_token_id (4.34's place for the processor).  Pitch ids are [pitch_offset, pitch_offset +
 * n_pitch), time ids the n_time ids after them; EOS = 2, ONSET = 3 and OFFSET = 4 as the tokenizer writes them.  The state of a row
 * (phase, last time index, the sounding pitches of earlier groups and of the current one: 48 bytes per clip in the workspace) is
 * advanced by the id actually emitted, so a step costs O(1) whatever its position.  grammar == NULL is m2m_generate_scored.
 * proc, sample and the two outputs are as there (all optional; with both outputs NULL the unscored processed head runs).
 * M2M_ERR_INVALID: pitch_offset < 5, n_pitch outside [1, 128], n_time < 1, pitch_offset + n_pitch + n_time > vocab_size, vocab_size
 * > 4096, max_length > 2048, eos_token_id != 2.
 */
typedef struct { int pitch_offset, n_pitch, n_time; } m2m_grammar_params;
int m2m_generate_grammar(m2m_session* s, int max_length, const m2m_grammar_params* grammar, const m2m_process_params* proc,
                         const m2m_sample_params* sample, int64_t* tokens_out_dev, float* scores_out_dev, float* logprobs_out_dev,
                         int* out_len_host, void* stream);

/*
 * Beam search under the MIDI token grammar and the logits processors (hf 4.34: generate(num_beams=..., prefix_allowed_tokens_fn=...,
 * min_length=..., forced_eos_token_id=...), _beam_search with a non-empty logits_processor).  The step is m2m_generate_beam's with
 * one change: the fp32 log_softmax of a row is processed against its own beam's prefix (cur_len = t + 1) BEFORE the running beam
 * score is added, in _get_logits_processor's order: one-id bad_words, min_length, min_new_tokens, the grammar's mask (as
 * m2m_generate_grammar: PrefixConstrainedLogitsProcessor's place), forced_bos_token_id, forced_eos_token_id (every other id -inf,
 * the forced one 0: it wins over the grammar), suppress_tokens, begin_suppress_tokens.  The grammar state is kept per ROW (48 bytes
 * each, max_batch of them in the workspace): new beam i takes its parent's state advanced by the id it carries.  A clip may have
 * fewer than num_beams finite candidates that are not EOS (the forced_eos_token_id step): as in HF its beams are then filled from
 * candidates at -inf, ties to the lower beam-major flat index, and carry the score -inf from there on; a returned hypothesis may
 * have the score -inf.  No NaN arises: raw logits are finite or the call returns M2M_ERR_RANGE.
 * grammar == NULL: no grammar; proc == NULL: no processor; both NULL: this IS m2m_generate_beam.  With a neutral block and no grammar
 * the ids and scores are m2m_generate_beam's.  M2M_ERR_INVALID without launching anything: every invalid case of m2m_generate_beam
 * and of m2m_generate_grammar's block, an invalid processor block (as m2m_generate_processed), a processor that reads a row's history
 * (repetition_penalty != 1, no_repeat_ngram_size > 0, a bad_words sequence of two or more ids: a beam's history is scattered through
 * the ancestry table), max_length > 2048.  Everything else is as for m2m_generate_beam.
 */
int m2m_generate_beam_processed(m2m_session* s, int max_length, const m2m_beam_params* p, const m2m_grammar_params* grammar,
                                const m2m_process_params* proc, int64_t* tokens_out_dev, float* scores_out_dev, int* out_len_host,
                                void* stream);

/*
 * Rows end at different steps (ref: music2midi/model.py:115-135 decodes chunks of inference.batch_size = 128 three-second
 * segments to max_length 1024; a trained checkpoint ends a segment after tens to hundreds of tokens).  Once a quarter of the
 * rows still being decoded have emitted EOS, m2m_generate_greedy (and m2m_generate_sample, m2m_generate_processed) re-packs the live rows into the first slots of the batch at its
 * next host poll and goes on with smaller launches; ids do not depend on it.  The host polls after 16, 32, 64, 96 and 128 steps and
 * then every 64 (without the re-packing: every 64).  A poll copies every chain's loop state - and, where a re-packing is possible
 * (>= 64 steps left, >= 2 rows), its finished flags - to pinned memory on the chain's own stream, launches the first graph of the
 * next chunk, and only then waits for the copies: the chains do not run dry at a poll, and the host decides from the snapshot alone,
 * so ids, lengths and these statistics do not depend on it.  Only a poll that does re-pack drains the chains (rows move between
 * idle chains, one graph later than they were counted).  One case keeps the draining poll because it measured faster with it: two
 * chains that stream the same cross-K/V layers from HBM (more layers streamed than the two chains' resident windows hold between
 * them, e.g. 32 clips x 864 positions in fp32).  M2M_POLL_LOOKAHEAD=0 restores the draining poll everywhere (every chain idle from
 * its last kernel until the host has read the snapshot and launched again, at every poll - M2M_COMPACT=1 adds four early polls
 * even to a batch that never emits EOS).  This returns how often rows were re-packed in the
 * last call and how many were moved; rows_moved > 0 means that call consumed the session's encode (see m2m_generate_greedy).
 * M2M_COMPACT=0 in the environment disables the re-packing.
 */
int m2m_session_repack_stats(const m2m_session* s, int* repacks_out, int* rows_moved_out);

/*
 * Teacher-forced decoder pass, replaces the decoder half of
 * ref: music2midi/transformer.py:35-37 (logits only; the loss is a host-side reduction).
 * dec_input_ids_dev [B, Ld] int64 (= shift_right(labels)), logits_out_dev [B, Ld, V] fp32.
 */
int m2m_decode_forced(m2m_session* s, const int64_t* dec_input_ids_dev, int Ld, float* logits_out_dev, void* stream);

/* ------------------------------------------------------------------------- *
 * Training step: what ref: music2midi/model.py:27-43 drives through Lightning —
 * `self.model(inputs).loss` (ref: music2midi/transformer.py:28-39: HF T5 forward with labels),
 * `loss.backward()`, and `Adafactor(self.parameters(), warmup_init=True).step()` with
 * `AdafactorSchedule` (relative step, no external learning rate).
 *
 * Parameters and gradients live in two caller-owned flat fp32 device buffers of
 * m2m_trainer_num_params() floats; m2m_trainer_tensor_info() gives every tensor's state-dict key
 * (relative to the LightningModule's `model.` prefix), shape and offset, so the host framework can
 * expose views of the same memory as its parameters.  q/k/v (and wi_0/wi_1, cross k/v) of a layer
 * are adjacent so that each fused projection is one matrix.  The library owns the activations,
 * the bf16 copy of the weights (throughput mode) and the optimizer state.
 * ------------------------------------------------------------------------- */
typedef struct m2m_trainer m2m_trainer;

typedef struct {
  char name[160];           /* e.g. "transformer.encoder.block.0.layer.0.SelfAttention.q.weight" */
  int64_t offset;           /* floats into the flat buffers */
  int rows, cols;           /* 1-D tensors: rows = length, cols = 0 */
} m2m_tensor_info;

/* n_cond / cond_rows_host: the conditioning embedding tables (ref: music2midi/input.py:45-55), trainable.
 * max_*: largest batch, encoder length (cond rows + frames) and label length of a step.
 * A trainer is used from one host thread at a time; it owns its activations (m2m_trainer_workspace_bytes: 2.3 GB at 16 clips of
 * 3 s — every sub-layer keeps its operands until the grouped weight-gradient launch), two streams and a captured graph. */
int  m2m_trainer_create(const m2m_t5_geometry* geom, int n_cond, const int* cond_rows_host, int precision,
                        int max_batch, int max_enc_len, int max_dec_len, m2m_trainer** out);
void m2m_trainer_destroy(m2m_trainer* t);
int64_t m2m_trainer_num_params(const m2m_trainer* t);
int  m2m_trainer_num_tensors(const m2m_trainer* t);
int  m2m_trainer_tensor_info(const m2m_trainer* t, int index, m2m_tensor_info* out);
int64_t m2m_trainer_workspace_bytes(const m2m_trainer* t);   /* device bytes the trainer holds (activations etc.) */

/*
 * Teacher-forced forward + backward.
 * enc_inputs_dev [B, S, d_model] fp32: log-mel rows at [n_cond, S) as m2m_logmel_f32 writes them; rows
 *                [0, n_cond) are overwritten from the CURRENT conditioning tables (they are trainable).
 * cond_idx_dev   [B, n_cond] int64.        labels_dev [B, Ld] int64, -100 = ignored
 *                (decoder inputs = shift_right(labels), hf: modeling_t5.py:618-637).
 * loss_out_dev   fp32[1]: mean cross entropy over the non-ignored labels.
 * grads_dev      flat fp32, OVERWRITTEN with d loss / d params; NULL = forward only.
 * logits_out_dev optional [B, Ld, V] fp32.
 * Deterministic: every reduction has a fixed order, two calls give bit-identical results.
 * Streams: with gradients the pass runs on the trainer's own streams — stream-ordered behind everything already on `stream`
 * (the inputs are copied into trainer-owned buffers first) and `stream` waits for its end, so for the caller it behaves like
 * work on `stream`.  From the second call with the same (params_dev, grads_dev, B, S, Ld, dropout) on, the pass is replayed as
 * one captured HIP graph (M2M_TRAIN_GRAPH=0 disables that), one graph PER SHAPE: up to 8 keys are kept, least recently used
 * first out, so batches whose label length changes and comes back replay their own graph; params_dev / grads_dev must stay
 * valid while the trainer lives.  A batch without any scored label (all -100) gives loss = NaN and zero gradients, as torch's
 * CrossEntropyLoss does.
 */
int m2m_train_forward_backward(m2m_trainer* t, const float* params_dev, const float* enc_inputs_dev,
                               const int64_t* cond_idx_dev, const int64_t* labels_dev, int B, int S, int Ld,
                               float* loss_out_dev, float* grads_dev, float* logits_out_dev, void* stream);

/* Gradient accumulation (pytorch-lightning's Trainer(accumulate_grad_batches=N): each micro-batch's backward sees loss / N and the
 * gradients add up until the optimizer steps).  The same pass as m2m_train_forward_backward, except:
 * grads_dev      required; d (loss * grad_scale) / d params is ADDED to it when accumulate = 1, and OVERWRITES it when
 *                accumulate = 0 (the first micro-batch of a window).  Every writer of the buffer adds in its own epilogue:
 *                no separate pass over the buffer.  The alignment padding between tensors is zeroed as before.
 * grad_scale     finite, > 0 (1 / N); it multiplies the gradient of the logits only.  loss_out_dev stays the UNSCALED mean.
 * The mode (scaled, accumulate) is part of the per-shape graph key; the factor is not: it is read from a device word written
 * before every replay, so one graph per shape and mode serves any N.  With a sync stream set, the early ranges are released
 * once their accumulated values are final.  m2m_train_forward_backward keeps its contract (grads OVERWRITTEN, factor 1). */
int m2m_train_forward_backward_acc(m2m_trainer* t, const float* params_dev, const float* enc_inputs_dev,
                                   const int64_t* cond_idx_dev, const int64_t* labels_dev, int B, int S, int Ld,
                                   float* loss_out_dev, float* grads_dev, float* logits_out_dev, float grad_scale, int accumulate,
                                   void* stream);

/* Dropout of the teacher-forced pass (hf T5Config.dropout_rate, 0.1 in the reference's config; active because
 * ref: train.py:33 puts the module in train() mode): on the embeddings, the attention probabilities, every
 * residual branch, the gated activation and the final norms, as hf: modeling_t5.py places them.  Masks come from a
 * counter-based hash of (seed, forward_backward call index since this call, site, element) and are regenerated in the
 * backward pass.  p = 0 (the default after create) switches it off. */
int m2m_trainer_set_dropout(m2m_trainer* t, float p, uint64_t seed);

/* Data-parallel training (ref: train.py:40-41 — pl.Trainer(strategy="ddp"): the gradient all-reduce overlapped with backward).
 * With a sync stream set, m2m_train_forward_backward issues the backward pass in two parts — decoder side, then encoder side —
 * and makes `sync_stream` wait (a device-side event, no host synchronisation) for the point where the gradients of the two
 * "early" ranges are final and will not be written again in this call: the shared embedding + lm_head at the front of the flat
 * buffer, and the decoder blocks.  The all-reduce of those ranges, enqueued on `sync_stream` right after the call returns, runs
 * beside the encoder-side backward; the rest of the buffer is final when the caller's own stream continues.  The gradients are
 * bit-identical to the unsplit pass.  nullptr switches the split off.
 * m2m_trainer_early_grad_ranges: out[0..3] = {offset, count, offset, count} in floats of the flat gradient buffer. */
int m2m_trainer_set_sync_stream(m2m_trainer* t, void* sync_stream);
int m2m_trainer_early_grad_ranges(const m2m_trainer* t, int64_t* out);
/* Measurement hook (bench.py train_configs4.roofline): nodes (kernel launches + copies) of the captured graph(s) of the shape
 * most recently passed to m2m_train_forward_backward = launches per training step; 0 while that shape has not been captured. */
int m2m_trainer_graph_nodes(const m2m_trainer* t);

/* One transformers.optimization.Adafactor step with the reference's settings (lr=None, eps=(1e-30, 1e-3),
 * clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0, scale_parameter, relative_step,
 * warmup_init): params_dev is updated in place from grads_dev.  The step counter and the factored second
 * moments are library-owned; export/import them to checkpoint a run. */
int m2m_adafactor_step(m2m_trainer* t, float* params_dev, const float* grads_dev, void* stream);
int m2m_adafactor_get_step(const m2m_trainer* t);
int64_t m2m_adafactor_state_floats(const m2m_trainer* t);
int m2m_adafactor_state_export(const m2m_trainer* t, float* state_out_dev, void* stream);
int m2m_adafactor_state_import(m2m_trainer* t, const float* state_in_dev, int step, void* stream);

/* Gradient clipping as pytorch-lightning's Trainer(gradient_clip_val=, gradient_clip_algorithm=) applies it where the optimizer
 * steps (the rules: music2midi_amd/clipping.py).  algorithm 0: off (the default after create; `value` is ignored), 1: norm —
 * torch.nn.utils.clip_grad_norm_(params, value): total = the 2-norm of the per-tensor 2-norms, every gradient times
 * coef = min(1, value / (total + 1e-6)); 2: value — torch.nn.utils.clip_grad_value_: every element clamped to [-value, value], a NaN
 * stays a NaN.  M2M_ERR_INVALID for another algorithm, and for a value that is NaN or <= 0 while the algorithm is not 0.
 * Every m2m_adafactor_step that follows applies the setting: in norm mode it first runs the two norm launches on grads_dev (a full
 * read of the gradient; no atomics, every sum in a fixed order) and leaves the two words readable; the clip itself costs no
 * further pass: the step's kernels read g * coef (or the clamped g) on the fly, so the second moments see the clipped gradient.
 * grads_dev is NOT written: it holds the unclipped gradient after the step (Lightning's .grad is clipped in place).
 * With algorithm 0 the step is the unclipped one, bit for bit. */
int m2m_trainer_set_grad_clip(m2m_trainer* t, int algorithm /* 0 off, 1 norm, 2 value */, float value);

/* The global gradient norm of any gradient buffer laid out as the trainer's: out_dev[0] = total norm as above, out_dev[1] = coef
 * against the trainer's max_norm (clipping off or in value mode: against +inf, i.e. 1).  Two launches and one device-to-device copy
 * of the two fp32 words on `stream`; never synchronises the host; two calls on the same buffer give bit-identical words.  A
 * non-finite gradient is not special-cased: one +inf element gives (inf, 0).  grads_dev NULL: nothing is launched, out_dev receives
 * the two words the last norm-mode m2m_adafactor_step left (zeros before the first). */
int m2m_trainer_grad_norm(m2m_trainer* t, const float* grads_dev, float* out_dev /* [2] */, void* stream);

/* One MXFP8 product, C[M,N] = A[M,K] . B[N,K]^T (fp32 in and out, device pointers, row-major): both operands are quantised
 * to OCP block-scaled FP8 — 32 elements along K per power-of-two E8M0 scale, e4m3 elements (e5m2 for A when a_is_e5m2, the
 * gradient format) — and multiplied on gfx950's scaled MFMA (v_mfma_scale_f32_32x32x64_f8f6f4).  This is the arithmetic of
 * the fp8 training mode (M2M_PREC_FP8 of m2m_trainer_create), exposed so it can be checked on its own.  A test utility:
 * unlike the hot-path entry points it allocates and frees its own device scratch, and it synchronises `stream`. */
int m2m_mx8_matmul_f32(const float* a_dev, const float* b_dev, int M, int N, int K, int a_is_e5m2, float* c_dev, void* stream);
/* The same with A in bf16, as the training step feeds it (K a multiple of 8): fused != 0 quantises A inside the product's operand
 * staging (one launch per product, what the fp8 mode runs), 0 through the separate row quantiser; bit-identical by construction
 * and by test.  Test utility like the above. */
int m2m_mx8_matmul_bf16a(const uint16_t* a_bf16_dev, const float* b_dev, int M, int N, int K, int a_is_e5m2, int fused, float* c_dev,
                         void* stream);
/* The fp8 training step's own routes, one at a time (test utilities like the above: own scratch, `stream` synchronised; bad
 * arguments answer M2M_ERR_INVALID).  The quantiser hooks return the RAW images; what the kernel does not write stays 0xFF.
 * m2m_mx8_quantize_cols: the transposing quantiser of the fp8 weight gradient on src [R][C] (fp32, or bf16 when src_is_bf16; row
 *   stride ld_s >= C elements): qt [C][Rp] FP8 bytes + scales [C][Rp/32] E8M0 bytes, blocks of 32 along the R rows,
 *   Rp = R rounded up to 128, rows >= R zero.
 * m2m_mx8_quantize_rows: the row quantiser (what m2m_mx8_matmul_* and the unfused step products run) on the same kind of source:
 *   q [R][Cp] + scales [R][Cp/32], blocks along the C columns, Cp = C rounded up to 128, columns >= C zero.
 * m2m_mx8_quantize_weight: the step's weight quantiser on one fp32 matrix W [N][K] (N, K multiples of 128, as the fp8 mode requires):
 *   q [N][K] + qs [N][K/32] with blocks along K, qt [K][N] + qts [K][N/32] with blocks along N; e4m3. */
int m2m_mx8_quantize_cols(const void* src_dev, int src_is_bf16, int R, int C, int64_t ld_s, int is_e5m2, uint8_t* qt_dev, uint8_t* scales_dev,
                          void* stream);
int m2m_mx8_quantize_rows(const void* src_dev, int src_is_bf16, int R, int C, int64_t ld_s, int is_e5m2, uint8_t* q_dev, uint8_t* scales_dev,
                          void* stream);
int m2m_mx8_quantize_weight(const float* w_dev, int N, int K, uint8_t* q_dev, uint8_t* qs_dev, uint8_t* qt_dev, uint8_t* qts_dev, void* stream);
/* One projection product as the fp8 step issues it, for a weight W [N][K] and M rows (all row-major, dense):
 *   kind 0, forward:  c [M][N] = x [M][K] . W^T     a = x (bf16), b = W (fp32, through the step's weight quantiser, row image)
 *   kind 1, dX:       c [M][K] = dy [M][N] . W      a = dy (bf16, e5m2 when grad_is_e5m2), b = W (fp32, transposed image)
 *   kind 2, dW:       c [N][K] = dy^T . x           a = dy [M][N], b = x [M][K] (both bf16): two transposing quantiser launches, then
 *                                                    the product over the M rows under the step's split-K policy
 * fused (kinds 0, 1): a is quantised in the product's operand staging (1) or by the row quantiser (0).  epilogue: 0 = c bf16,
 * 1 = c fp32, 2 = c fp32 += product, 3 = c fp32 = r + dropout(product) with the step's counter-based hash (drop_p; element index
 * row * width of c + column, key = splitmix64(step_key + site_salt)); kind 2 takes 1 or 2 only, N and K of kinds 0 and 1 are
 * multiples of 128.  ksplit_out / kchunk_out (optional, host): the k-split and k-chunk the route used (1 and the whole depth when unsplit). */
int m2m_mx8_step_product(int kind, const uint16_t* a_bf16_dev, const void* b_dev, int M, int N, int K, int grad_is_e5m2, int fused, int epilogue,
                         void* c_dev, const float* r_dev, float drop_p, uint64_t step_key, uint64_t site_salt, int* ksplit_out, int* kchunk_out,
                         void* stream);

/* The training step's whole-head attention kernels on their own (csrc/attn_train.hip; hf: modeling_t5.py:159-170 T5Attention and its
 * autograd backward): q [B, Sq, H*64], k / v [B, Sk, H*64] bf16, row-major; bias_tab [H][Sq + Sk - 1] fp32 by (key - query + Sq - 1)
 * or NULL; no 1/sqrt(d) scaling; dropout on the probabilities with the step's counter-based hash (element index
 * ((b*H + h)*Sq + query) * round_up_8(Sk) + key, key = splitmix64(step_key + site_salt)).  Forward: out [B, Sq, H*64] bf16 and the
 * row log-sum-exp lse [B*H][Sq] fp32.  Backward: from q, k, v, out, lse and d_out the gradients dq / dk / dv (layouts of q / k / v) and,
 * with a bias, diag_part [B*H][ceil(Sq/32)][Sk + 31] = per-query-block sums of dS along the diagonals key - local row = x - 31.
 * keep_bits [B*H][ceil(Sk/32)][round_up_32(Sq)] uint32 (needed when drop_p > 0): the forward pass writes one word per (key block, query) —
 * bit k = probability (query, 32 * block + k) is kept — and the backward pass reads them instead of hashing again.
 * Test utilities like m2m_mx8_matmul_f32 (they own one device word for the step key and synchronise `stream` to set it). */
int m2m_attn_head_fwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, const float* bias_tab, int B, int H, int Sq, int Sk,
                           int causal, float drop_p, uint64_t step_key, uint64_t site_salt, uint16_t* out, float* lse, uint32_t* keep_bits,
                           void* stream);
int m2m_attn_head_bwd_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* out, const float* lse, const uint16_t* d_out,
                           const float* bias_tab, int B, int H, int Sq, int Sk, int causal, float drop_p, uint64_t step_key, uint64_t site_salt,
                           const uint32_t* keep_bits, uint16_t* dq, uint16_t* dk, uint16_t* dv, float* diag_part, void* stream);

/* ------------------------------------------------------------------------- *
 * Measurement hooks (bench.py): time one kernel of the decode step in isolation
 * with hipEvents on `stream`, cycling through all decoder layers so the working
 * set matches the real loop.  Requires a prior m2m_encode on the session.
 * ------------------------------------------------------------------------- */
enum {
  M2M_KERNEL_DEC_CROSS_ATTN = 0,
  M2M_KERNEL_DEC_SELF_ATTN = 1,
  M2M_KERNEL_DEC_STEP = 2        /* the whole captured step graph */
};
/* self_len: number of cached self-attention keys to assume (1..max_dec_len).
 * avg_us_host: mean duration of one launch in microseconds.
 * bytes_host: algorithmic HBM bytes one launch moves (K/V streamed + q read + o written). */
int m2m_bench_kernel(m2m_session* s, int which, int self_len, int iters, float* avg_us_host,
                     int64_t* bytes_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSIC2MIDI_AMD_H */
