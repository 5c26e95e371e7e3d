/*
 * sad.h -- C ABI of libsad.so, the MI355X (gfx950) hot path of the
 * synthetic-audio-detection pipeline:
 *
 *   int16 PCM (4 s @ 32 kHz) -> STFT -> mel -> dB -> standardise      [frontend]
 *   -> bilinear 512x512 -> ResNet-18 backbone -> global avg pool        [backbone]
 *   -> N binary heads -> real-logit-averaging ensemble merge            [heads]
 *
 * The reference (TtesseractT/Synthetic-Audio-Detection @ 2025-05-23) has no
 * FFI: its hot path is Python calling torchaudio / torchvision / timm.  Each
 * entry point below names the reference interface (file:line) it replaces; the
 * Python host layer (synthetic-audio-detection_amd/sad/_lib.py) binds them with
 * ctypes, exactly as INTEGRATION.md shows.
 *
 * Conventions:
 *   - every call returns 0 on success, a negative sad_status otherwise;
 *     sad_last_error() returns a thread-local message for the last failure;
 *   - all tensors are caller-owned device pointers (PyTorch caching allocator);
 *     the library never frees caller memory;
 *   - plans are opaque, immutable after creation, freed by *_destroy (one
 *     exception: the experimental fused front end's counters, see
 *     sad_frontend_run);
 *   - *_run calls are asynchronous on the given hipStream_t (passed as void*),
 *     never allocate, never synchronise (graph-capturable; one exception: the
 *     FIRST sad_heads_grad_run on a plan builds its transposed weights);
 *   - distinct plans / streams may be used from different threads;
 *   - cross-stream hand-offs need only the usual event: an output written on
 *     one stream (a libsad call, or a collective on the NCCL/RCCL stream) may
 *     be consumed by a *_run on another stream after hipStreamWaitEvent (or a
 *     host wait) on an event recorded after the producer.  Kernels of
 *     different streams may run concurrently and co-reside on a CU; the
 *     outputs do not depend on it (tests/test_gpu_handoff.py: the front end
 *     beside the stem, and heads / AdamW / backbone fed from a side stream).
 *     The device code holds no packed-FP32 VALU instructions: on MI355X they
 *     returned wrong values while another kernel's MFMAs ran on the same CU
 *     (csrc/Makefile NOPK, tests/test_isa_scan.py).
 */
#ifndef SAD_H_
#define SAD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum sad_status {
  SAD_OK = 0,
  SAD_ERR_ARG = -1,      /* bad argument / shape */
  SAD_ERR_HIP = -2,      /* HIP runtime error */
  SAD_ERR_STATE = -3,    /* not initialised / wrong plan */
  SAD_ERR_NOMEM = -4,    /* workspace too small or device allocation failed */
};

enum sad_dtype {
  SAD_F32 = 0,   /* fp32 activations, f32 MFMA (v_mfma_f32_16x16x4_f32): parity mode */
  SAD_BF16 = 1,  /* bf16 activations, bf16 MFMA (v_mfma_f32_16x16x32_bf16), f32 accumulate */
  SAD_BF16X3 = 2, /* split-bf16 parity mode: every value v stored as hi = bf16(v), lo = bf16(v - hi)
                    (channels interleaved [hi 32 | lo 32] per group of 32, 4 B per value like fp32);
                    each product = W_hi.X_hi + W_lo.X_hi + W_hi.X_lo on bf16 MFMA, f32 accumulate:
                    ~2^-17 relative operands, 3x the bf16 MFMA work, 16/3 x the f32 MFMA rate */
  SAD_F16 = 3    /* IEEE binary16 activations and weights, f16 MFMA (v_mfma_f32_16x16x32_f16), f32
                    accumulate: SAD_BF16's layouts (NHWC, the same weight packs, 2 B per value), kernels,
                    variants and grids with 11 significant bits instead of 8.  Inference only: the
                    backbone / ResNet plans and their runs, sad_conv2d_run, sad_block_conv_run,
                    sad_l1_block_run, sad_pack_conv_weight_run, sad_avgpool_run.
                    RANGE: a plan whose folded weights exceed 65,504 in magnitude, or whose folded
                    weights or biases are not finite, is refused (SAD_ERR_ARG, the message names the
                    conv).  Every fp16 activation store SATURATES a finite value to +-65,504 instead of
                    writing inf, and it does so SILENTLY: no error, no flag.  PRECONDITION: finite
                    inputs (maps, images, activations, biases).  The saturation is the hardware's
                    fp16-overflow clamp, which keeps a value that already is inf or NaN in fp32. */
};

/* ---------------------------------------------------------------- runtime */
/* Select the device for this thread's subsequent plan creation. */
int sad_init(int device);
/* Wait for the device, then release the launch-timing events of an
 * unfinished sad_profile_begin.  The small per-device constant buffers the
 * library allocates once (zero biases; stamp buffers of diagnostic builds) stay
 * allocated until the process exits.  Plans are caller-owned: destroy them
 * first.  sad_init may be called again after it. */
int sad_shutdown(void);
const char* sad_last_error(void);
/* Library / kernel build identification (for provenance in bench output). */
const char* sad_version(void);

/* --------------------------------------------------------------- frontend */
/* Replaces torchaudio.transforms.MelSpectrogram + AmplitudeToDB + the
 * standardisation at inference_runner.py:157-171 (and the norm=None trainer
 * variant at submodel_trainer.py:97-105,191-199). */
typedef struct sad_frontend_cfg {
  int32_t sample_rate;   /* 32000 */
  int32_t n_fft;         /* 2048 (only value supported) */
  int32_t hop_length;    /* 512 */
  int32_t n_mels;        /* 128 */
  float f_min;           /* 20 */
  float f_max;           /* 12000 */
  int32_t norm_slaney;   /* 1 = 'slaney' (inference), 0 = None (trainer) */
  float top_db;          /* 80; <0 disables the clamp */
  int32_t n_samples;     /* samples per segment, 128000 */
} sad_frontend_cfg;

typedef struct sad_frontend_plan sad_frontend_plan;

/* The mel filterbank built on the host in float64 from cfg (htk triangles,
 * optional slaney area norm), rounded once to fp32:
 *   pts[i] = mel2hz(hz2mel(f_min) + (hz2mel(f_max) - hz2mel(f_min)) i / (n_mels + 1)), i <= n_mels + 1,
 *   hz2mel(f) = 2595 log10(1 + f / 700); bin k sits at f = (sample_rate / 2) k / (n_fft / 2);
 *   fb[k][m] = max(0, min((f - pts[m]) / (pts[m+1] - pts[m]), (pts[m+2] - f) / (pts[m+2] - pts[m+1]))),
 *   times 2 / (pts[m+2] - pts[m]) with norm_slaney.
 * Limits (SAD_ERR_ARG otherwise, checked on the host before any device call or
 * allocation; *out is left untouched): n_fft = 2048, hop_length > 0,
 * 0 < n_mels <= 1024, n_samples > n_fft / 2, and the bank's non-zero weights
 * must lie within 792 consecutive FFT bins: bin_hi - bin_lo <= 791, bin_lo /
 * bin_hi the lowest / highest bin with a non-zero weight in any filter (an
 * all-zero filter counts as bin 0).  The kernels keep the power of bins
 * bin_lo..bin_hi in an 800-float buffer per wave, 8 of them padding.  The
 * reference's 20 Hz .. 12 kHz bank spans bins 2..768; a 0 Hz .. Nyquist bank
 * (torchaudio's default f_max) spans 1..1023 and is refused. */
int sad_frontend_plan_create(const sad_frontend_cfg* cfg, sad_frontend_plan** out);
/* The same with the caller's filterbank: fbank = HOST fp32 [n_fft/2 + 1][n_mels]
 * (finite, >= 0; copied).  torchaudio builds its bank in fp32 arithmetic
 * (melscale_fbanks, called by MelSpectrogram at inference_runner.py:158-166);
 * the host layer passes that exact bank, so the device projects on the
 * reference's weights, not on a more accurate rounding of the same triangles
 * (which moves a mel bin next to a strong tone at a triangle's edge by up to
 * 6e-3 dB).  The same limits as sad_frontend_plan_create, the 791-bin span of
 * the non-zero weights included. */
int sad_frontend_plan_create_fb(const sad_frontend_cfg* cfg, const float* fbank, sad_frontend_plan** out);
int sad_frontend_plan_destroy(sad_frontend_plan* plan);
/* Number of STFT frames per segment (1 + n_samples / hop = 251). */
int sad_frontend_frames(const sad_frontend_plan* plan, int32_t* n_frames);

/* Two kernels: fe_mel_db writes the dB map, fe_normalize standardises it.
 * (SAD_FE_FUSED=1/2 selects an experimental one-kernel form in which the last
 * workgroup of a segment standardises it, counting arrivals in the plan's
 * per-segment counters; it measured 1.7-2.2x slower, DESIGN.md 5c.  With it,
 * runs of ONE plan must not execute concurrently.)
 *
 * pcm: int16 mono segments, segment i at pcm + i*seg_stride (elements),
 *      n_samples each.  There is no n_ch argument: multi-channel audio goes
 *      through sad_pcm_mono_run first, once per file, as the reference
 *      averages the whole waveform before slicing it (inference_runner.py:145-146);
 *      averaging per segment would redo it for every overlapping window;
 * out_db:  optional [n_seg, n_mels, n_frames] fp32 dB map after the top-db
 *          clamp (NULL to skip);
 * out_map: [n_seg, n_mels, n_frames] fp32 standardised map
 *          (x - mean) / (std_unbiased + 1e-6), per segment. */
int sad_frontend_run(const sad_frontend_plan* plan, const int16_t* pcm, int64_t n_seg,
                     int64_t seg_stride, float* out_db, float* out_map, void* stream);
/* Same on fp32 waveforms already in [-1, 1) (the reference's tensor after
 * mono averaging / resampling, preprocess_waveform at inference_runner.py:144-155). */
int sad_frontend_run_f32(const sad_frontend_plan* plan, const float* wav, int64_t n_seg,
                         int64_t seg_stride, float* out_db, float* out_map, void* stream);
/* Windows of ONE long fp32 waveform wav[wav_len], read in place: segment i
 * starts at sample offsets[i] (DEVICE int64 array; each clamped to
 * [0, wav_len - n_samples]).  Replaces the per-window tensors of slice_waveform
 * (inference_runner.py:176-190) + torch.cat(specs) (:276-289): overlapping
 * windows are never copied. */
int sad_frontend_run_windows(const sad_frontend_plan* plan, const float* wav, int64_t wav_len,
                             const int64_t* offsets, int64_t n_seg, float* out_db, float* out_map,
                             void* stream);

/* -------------------------------------------------------------- ingestion */
/* preprocess_waveform (inference_runner.py:144-155) on the device: the WAV's
 * samples go to HBM as stored (int16) or host-decoded fp32, interleaved
 * [frames][channels]. */
enum sad_pcm_format {
  SAD_PCM_I16 = 0, /* int16, scaled by 1/32768 (torchaudio.load normalize=True) */
  SAD_PCM_F32 = 1  /* fp32 (other WAV encodings, decoded on the host) */
};
/* out[i] = mean_c pcm[i][c] (waveform.mean(dim=0): channels summed in order, / C) for
 * i < frames, 0 for frames <= i < out_len (the zero pad to one window, :151-154). */
int sad_pcm_mono_run(const void* pcm, int32_t format, int64_t frames, int32_t channels, float* out,
                     int64_t out_len, void* stream);

/* Replaces torchaudio.transforms.Resample(orig_freq, new_freq) with its
 * defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), as built
 * at inference_runner.py:148 (and submodel_trainer.py:150-153): the plan holds
 * the polyphase kernel table (float64 on the host, rounded once to fp32). */
typedef struct sad_resample_plan sad_resample_plan;
int sad_resample_plan_create(int32_t orig_freq, int32_t new_freq, sad_resample_plan** out);
int sad_resample_plan_destroy(sad_resample_plan* plan);
/* ceil(new * n_in / orig) with the rates reduced by their gcd (torchaudio's target_length) */
int sad_resample_out_len(const sad_resample_plan* plan, int64_t n_in, int64_t* n_out);
/* x [n_in] fp32 -> y [y_len] fp32: the resampled signal, then zeros up to
 * y_len (>= sad_resample_out_len) */
int sad_resample_run(const sad_resample_plan* plan, const float* x, int64_t n_in, float* y, int64_t y_len,
                     void* stream);

/* out[w] = max |wav[w*hop, w*hop + window)| (window clipped at n; NaN
 * propagates as in torch.max), w < n_windows: the silence test of
 * slice_waveform (inference_runner.py:182-184) without moving windows to the host. */
int sad_window_absmax_run(const float* wav, int64_t n, int64_t window, int64_t hop, int64_t n_windows,
                          float* out, void* stream);

/* ------------------------------------------------------ trainer ingestion */
/* SpectrogramDataset.__getitem__'s load, resample and 2-segment rule
 * (submodel_trainer.py:143-187) for a whole batch of files in ONE launch.  The
 * files' samples sit as stored (interleaved int16, or host-decoded fp32) in one
 * byte arena on the device; only the head of a file that the two segments read
 * has to be there.
 *
 * sad_train_ingest_need_frames: the frames of a file at orig_freq that the
 * first 2 seg_len samples at new_freq read:
 *   2 seg_len                                      orig_freq == new_freq
 *   ((2 seg_len - 1) / new) orig + orig + width    otherwise (orig, new reduced by
 *                                                  their gcd; width as in the plan)
 * A host reads min(total frames, need) frames of each file.
 *
 * file_table [n_files][6] int64, one row per file:
 *   0 byte offset of the file's first sample in the arena (a multiple of 16)
 *   1 frames present in the arena (<= total frames)
 *   2 total frames of the file (sets its resampled length n_out =
 *     sad_resample_out_len, or the frame count at the target rate)
 *   3 channels (1..64)          4 sad_pcm_format          5 index into rate_plans
 * rate_plans [n_rates <= 8]: the resample plan of each source rate to the
 * target rate, NULL for the target rate itself.
 *
 * out [2 n_files][seg_len] fp32.  Row 2f + s, sample i, with m = s seg_len + i:
 * 0 for m >= n_out, else the mono mix of sad_pcm_mono_run fed to the polyphase
 * sum of sad_resample_run (same operations in the same order: the bits that
 * the two calls give on the whole file); samples past the frames present count
 * as 0.  A file with n_out < 2 seg_len gives its first segment (zero-padded when
 * n_out < seg_len) in both rows.  The caller drops files shorter than the
 * reference's 0.9 seg_len rule beforehand.
 *
 * Workgroups are (file, tile) pairs: tiles [n_tiles][2] int32 lists, per file
 * in any order, tile = 0 .. sad_train_ingest_file_tiles(...) - 1.  file_table
 * is read on the HOST for the argument checks; d_file_table (the same values)
 * and d_tiles are DEVICE copies, normally uploaded with the arena in one copy.
 * A rate with fewer than 64 phases whose 1024-output input span exceeds 8192
 * samples (beyond 192 kHz -> 32 kHz) is refused.  Asynchronous on `stream`:
 * one launch, no allocation, no atomics, no host synchronisation. */
int sad_train_ingest_need_frames(int32_t orig_freq, int32_t new_freq, int64_t seg_len, int64_t* need);
int sad_train_ingest_file_tiles(int32_t orig_freq, int32_t new_freq, int64_t total_frames, int64_t seg_len,
                                int64_t* n_tiles);
int sad_train_ingest_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                         const int64_t* d_file_table, int64_t n_files, const int32_t* d_tiles, int64_t n_tiles,
                         const sad_resample_plan* const* rate_plans, int32_t n_rates, int64_t seg_len, float* out,
                         void* stream);

/* -------------------------------------------------- waveform augmentation */
/* Six of the eleven kinds of the reference's audio_augmneter.py (:79-137, the
 * clip of :190), one kind per file, applied to a batch that already sits in
 * sad_train_ingest_run's byte arena (submodel_trainer.py --wave-augment).  The
 * float64 contract is tests/waveaug_ref.py.  y is the file's mono mix
 * (sad_pcm_mono_run's value, operation for operation; 0 past the frames
 * present), sr its stored rate, L its total frames:
 *   0 original                    y
 *   1 dynamic_range_compression   sign(y) |y|^p0                       p0 > 0
 *   2 add_white_noise             y_i + p0 rms n_i; rms over the frames written,
 *                                 n_i a standard normal of (key, i) alone: the
 *                                 splitmix64 finaliser of key + 0x9E3779B97F4A7C15 (i + 1),
 *                                 u1 = (top 24 bits + 1) / 2^24, u2 = bits 16..39 / 2^24,
 *                                 n = sqrt(-2 ln u1) cos(2 pi u2)
 *   3 tremolo                     y ((1 - p1) + p1 sin(2 pi p0 t_i)), t = linspace(0, L / sr, L)
 *   4 phaser                      lfo_i = p1 sin(2 pi p0 i / sr); for f0 = 500, 1500, 2500 Hz:
 *                                 y <- y + lfo lfilter([al, 0, -al], [1 + al, -2 cos w, 1 - al], y),
 *                                 w = 2 pi f0 / sr, al = sin(w) / 2; refused for sr <= 5000
 *   5 time_shift                  out_i = y_{i - s} if s != 0 and 0 <= i - s < L, else 0;
 *                                 s = p0, a whole number of frames (s = 0: all zeros, as
 *                                 the reference gives)
 * then clip(., -1, 1).  speed_up, slow_down, pitch_up, pitch_down and
 * time_pitch_shift are kinds 6-10 of sad_wave_stretch_run ("time and pitch"
 * below), not of these entries.  Deviations
 * from the reference's tool: no resample to 44.1 kHz before augmenting, no round
 * trip through a 16-bit stereo file after it, the rms over the frames written
 * instead of the whole file, and this generator instead of numpy's.
 *
 * file_table [n_files][6] int64 and the arena: as for sad_train_ingest_run
 * (column 5 is not read).  aug_table [n_files][8] int64, one row per file:
 *   0 kind   1 sample rate (Hz)   2 frames to write, n_out <= total frames
 *   3 byte offset of the file's output in mono_out (a multiple of 16, ascending)
 *   4 p0 | p1: two fp32 values, p0 in the low 32 bits   5 the noise key
 *   6 the sum of ceil(n_out / chunk) over the earlier files   7 reserved
 * mono_out holds per file its first n_out frames, fp32, augmented and clipped;
 * sad_train_ingest_run then reads it through a second file table (SAD_PCM_F32, one
 * channel, n_out frames present, the same total), for which its mono mix is the
 * identity: a file of kind 0 gives the rows it gives without this call, bit for
 * bit (int16 files; fp32 files within [-1, 1]).
 *
 * Both tables are read on the HOST for the argument checks; d_file_table and
 * d_aug_table are DEVICE copies (uploaded with the arena).  ws: caller-owned,
 * 16-byte aligned, sad_wave_augment_workspace_size bytes.  At most seven
 * launches for any batch (csrc/waveaug.hip says which), no allocation, no
 * atomics, no host synchronisation; asynchronous on `stream`.  A file's output
 * does not depend on the other files.  sad_wave_augment_geometry: the phaser
 * scan's chunk (frames per workgroup) and the frames a lane walks serially. */
int sad_wave_augment_geometry(int32_t* chunk, int32_t* sub);
int sad_wave_augment_workspace_size(const int64_t* aug_table, int64_t n_files, size_t* bytes);
int sad_wave_augment_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                         const int64_t* d_file_table, int64_t n_files, const int64_t* aug_table,
                         const int64_t* d_aug_table, void* mono_out, int64_t mono_bytes, void* ws, size_t ws_bytes,
                         void* stream);
/* The phaser files of the same batch as ONE THREAD PER FILE walking the three
 * stages serially (the other kinds are left alone): the yardstick that
 * tools/bench_wave_augment.py times the chunked scan against.  Same tables,
 * same checks, one launch, no workspace. */
int sad_wave_phaser_serial_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                               const int64_t* d_file_table, int64_t n_files, const int64_t* aug_table,
                               const int64_t* d_aug_table, void* mono_out, int64_t mono_bytes, void* stream);

/* ---------------------------------------------------------- time and pitch */
/* The other five kinds of audio_augmneter.py (:55-76, :140-145, the clip of
 * :190), the ones that go through librosa (submodel_trainer.py --wave-stretch,
 * csrc/stretch.hip).  The float64 contract is tests/stretch_ref.py: librosa's
 * documented time_stretch and pitch_shift restated (n_fft 2048, hop 512,
 * periodic Hann, center = True with zero padding), NOT pinned to librosa:
 *   time_stretch(y, r) = istft(phase_vocoder(stft(y), r), round(len(y) / r))
 *   pitch_shift(y, n)  = resample_ratio(time_stretch(y, q), q, len(y)), q = 2^(-n / 12)
 *   6 speed_up, 7 slow_down     time_stretch(y, rate)
 *   8 pitch_up, 9 pitch_down    pitch_shift(y, steps)
 *   10 time_pitch_shift         pitch_shift(time_stretch(y, rate), steps)
 * then clip(., -1, 1).  Deviations from the reference's tool: no resample to
 * 44.1 kHz first, no 16-bit file round trip, and resample_ratio, the
 * ingestion's Hann-windowed sinc (width 6, rolloff 0.99) at an arbitrary ratio
 *   out[i] = sum_j x[j] h(i / rho - j), h(u) = c sinc(c u) cos^2(pi u c / 12), |u| < 6 / c,
 *   c = 0.99 min(1, rho)
 * in the place of librosa's soxr_hq.
 *
 * Four stage entries, each batched over files through a stage table
 * [n_files][8] int64 (read on the HOST for the checks; d_table is its DEVICE copy):
 *   0 byte offset of the file's input in `in`     1 input count
 *   2 byte offset of its output in `out`          3 output count
 *   4 the rate, a float64's bits (vocoder, resample; within [0.25, 4])
 *   5 flags: 1 = clip the output to [-1, 1] (istft, resample)
 *   6 byte offset of the file's workspace in `ws` (vocoder, istft)   7 reserved
 * Offsets are multiples of 16 and ascend without overlap.  Counts:
 *   stft      in: fp32 samples present (0 past them); out: frames [T][1025] complex
 *             fp32, frame f = samples [512 f - 1024, 512 f + 1024); the caller
 *             gives T = 1 + length / 512 or fewer
 *   vocoder   in: frames present (0 past them); out: the steps t < count, step t at
 *             s = t rate (float64) reads frames int(s), int(s) + 1; the phase is a
 *             Q0.32 fraction of a turn, summed over the steps by a chunked scan
 *             of 32-bit integers (sad_wave_stretch_geometry's chunk)
 *   istft     in: frames available, of which the first ceil((length + 2048) / 512)
 *             are read; out: `length` fp32 samples (count), zero past the frames
 *   resample  in: fp32 samples; out: count samples at ratio rho = column 4
 * Asynchronous on `stream`, caller-owned workspace (the *_workspace_size entries),
 * no atomics, no allocation. */
int sad_wave_stretch_geometry(int32_t* n_fft, int32_t* hop, int32_t* chunk, int32_t* max_launches);
int sad_stft2048_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                     int64_t n_files, void* out, int64_t out_bytes, void* stream);
int sad_phase_vocoder_workspace_size(const int64_t* table, int64_t n_files, size_t* bytes);
int sad_phase_vocoder_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                          int64_t n_files, void* out, int64_t out_bytes, void* ws, size_t ws_bytes, void* stream);
int sad_istft2048_workspace_size(const int64_t* table, int64_t n_files, size_t* bytes);
int sad_istft2048_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                      int64_t n_files, void* out, int64_t out_bytes, void* ws, size_t ws_bytes, void* stream);
int sad_resample_ratio_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                           int64_t n_files, void* out, int64_t out_bytes, void* stream);
/* The batch entry.  arena and file_table [n_files][6]: as for sad_train_ingest_run
 * (column 1 = frames present, column 2 = total frames L; column 5 is not read).
 * stretch_table [n_files][8] int64, one row per file:
 *   0 kind: 6..10 above; 0..5 = a file of sad_wave_augment_run, left alone here
 *   1 rate, a float64's bits (kinds 6, 7, 10), within [0.25, 4]
 *   2 steps, a float64's bits (kinds 8, 9, 10), |steps| <= 12
 *   3 frames to write, n_out <= the kind's output length (round(L / rate); L for 8, 9)
 *   4 byte offset of the file's output in mono_out (a multiple of 16, ascending)
 *   5 the pitch rate 2^(-steps / 12), a float64's bits (kinds 8, 9, 10): every
 *     length on the host and on the device derives from these bits
 *   6, 7 reserved
 * The file is mono-mixed as sad_pcm_mono_run does (0 past the frames present),
 * goes through its kind's chain and is clipped; mono_out receives its first
 * n_out frames in the layout sad_wave_augment_run writes, so both entries fill one
 * arena that sad_train_ingest_run reads through its second file table.  Only
 * what the first n_out frames depend on is computed (tests/stretch_ref.py
 * need_frames says how much of the file that is).  For every file the result is,
 * bit for bit, what sad_pcm_mono_run and the stage entries give one after
 * another on that file alone: the entry runs the same kernels on stage tables
 * that one more kernel derives on the device.  At most 17 launches for any batch
 * (plan, mono mix, 7 per stretch x 2, resample); ws: 16-byte aligned,
 * sad_wave_stretch_workspace_size bytes.  Everything else is refused with
 * SAD_ERR_ARG before any launch. */
int sad_wave_stretch_workspace_size(const int64_t* file_table, const int64_t* stretch_table, int64_t n_files,
                                    size_t* bytes);
int sad_wave_stretch_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                         const int64_t* d_file_table, int64_t n_files, const int64_t* stretch_table,
                         const int64_t* d_stretch_table, void* mono_out, int64_t mono_bytes, void* ws,
                         size_t ws_bytes, void* stream);

/* --------------------------------------------------------------- streaming */
/* Live feeds (sad/stream.py, stream_runner.py): the ingestion above, formed
 * chunk by chunk for many feeds in ONE launch per push, with the resampler's
 * state carried across chunk boundaries.  For any way of cutting a recording
 * into chunks the samples are the bits sad_pcm_mono_run + sad_resample_run give
 * on the whole recording.
 *
 * A stream bank of `slots` slots is caller-owned device memory (like every
 * workspace of this library), sized by sad_stream_bank_size:
 *   arena [slots][2 CAP] fp32  per slot a mirrored ring of mono samples at the
 *         target rate: global sample g sits at g mod CAP and at CAP + g mod CAP,
 *         so up to CAP consecutive samples are contiguous from g mod CAP on and
 *         sad_scan_select_run / sad_frontend_run_windows read windows in place
 *         (wav = arena, wav_len = arena_len).  CAP = window + room, room =
 *         max(4 max_chunk_frames, 4096), rounded up to a multiple of 4.
 *   carry [slots][2][8192] fp32  the resampler's state: the mono-mixed input
 *         samples the next push's taps reach back to (fewer than K), double-
 *         buffered by push parity, because within one launch some workgroups of
 *         a slot read the old carry while another writes the new one.
 * Neither needs initialising: only what a push has written is ever read.
 *
 * Emission rule (rates reduced by their gcd to orig -> new; width, K as in the
 * resample plan).  With F frames of a feed present, the outputs whose taps are
 * all present are those of polyphase frames j < J(F) = (F - width) / orig (0
 * for F < width): a push from F0 to F1 frames stores global samples
 * [J(F0) new, J(F1) new); at the target rate it stores [F0, F1).  A final push
 * stores the rest up to n_out = ceil(new F1 / orig) (missing inputs are zeros)
 * and then zeros up to one window (preprocess_waveform's pad).  A feed opened
 * at start_frame = J0 orig counts everything before it as digital silence and
 * stores nothing below g0 = J0 new.
 *
 * sad_stream_open_check: may a feed of this rate and channel count, starting at
 * start_frame, use a bank of this geometry?  Refuses channels outside 1..64, a
 * rate the batched kernel cannot take (the rule of sad_train_ingest_file_tiles,
 * or more than 8192 taps), a rate whose single polyphase frame plus end-of-feed
 * tail exceed CAP - window, window > CAP, a start_frame that is no multiple of
 * orig, and one whose first sample g0 (returned in *first_sample) is no
 * multiple of hop.
 *
 * sad_stream_push_tiles: the workgroups of one table row, and (optionally) the
 * global sample range [*first_out, *end_out) the row stores.
 *
 * sad_stream_push_run: one launch for all rows.  The chunks sit as stored
 * (interleaved int16 / fp32) in one byte arena.  table [n_rows][10] int64:
 *   0 slot (each slot at most once per launch)
 *   1 byte offset of the chunk (a multiple of 16)    2 its frames (may be 0)
 *   3 absolute frames of the feed before this chunk (>= start frame)
 *   4 final (0 / 1)      5 index into rate_plans     6 channels (1..64)
 *   7 sad_pcm_format     8 the feed's start frame    9 push parity (0 / 1: the
 *     carry buffer to READ; the other one is written; the host flips it after
 *     every launch that names the slot)
 * tiles [n_tiles][2] int32: (row, tile), tile = 0 .. sad_stream_push_tiles - 1,
 * in any order.  rate_plans as for sad_train_ingest_run (NULL = target rate).
 * The host is the authority on every counter: the device mutates only arena
 * and carry.  A row may add at most CAP - window samples (the caller splits a
 * longer chunk).  table is read on the HOST for the argument checks; d_table
 * and d_tiles are DEVICE copies.  Asynchronous on `stream`: one launch, no
 * allocation, no atomics, no host synchronisation. */
int sad_stream_bank_size(int64_t slots, int64_t window, int64_t hop, int64_t max_chunk_frames,
                         int32_t target_rate, int64_t* cap, int64_t* arena_len, int64_t* carry_len);
int sad_stream_open_check(int32_t rate, int32_t target_rate, int32_t channels, int64_t window, int64_t hop,
                          int64_t cap, int64_t start_frame, int64_t* first_sample);
int sad_stream_push_tiles(int32_t rate, int32_t target_rate, int64_t start_frame, int64_t frames_before,
                          int64_t n_frames, int32_t final, int64_t window, int64_t* first_out, int64_t* end_out,
                          int64_t* n_tiles);
int sad_stream_push_run(const void* chunks, int64_t chunk_bytes, const int64_t* table, const int64_t* d_table,
                        int64_t n_rows, const int32_t* d_tiles, int64_t n_tiles,
                        const sad_resample_plan* const* rate_plans, int32_t n_rates, float* arena, float* carry,
                        int64_t slots, int64_t cap, int64_t window, void* stream);

/* --------------------------------------------------------- catalogue scan */
/* Many files in one run (sad/scan.py, catalog_runner.py): the files' mono
 * 32 kHz waveforms sit back to back in ONE fp32 arena; the device picks the
 * windows to keep (slice_waveform, inference_runner.py:176-190) and, after the
 * ensemble, does the per-file decisions of main (:292-349).  Both *_run calls
 * are asynchronous, allocate nothing and use no float atomics: the same inputs
 * give the same bytes on every run.
 *
 * Selection.  File f is wav[file_start[f], file_start[f] + file_len[f])
 * (DEVICE int64 arrays; a file that does not lie inside [0, wav_len) has no
 * candidates).  Its candidate windows start at range(0, file_len[f] - window + 1,
 * hop); a candidate is kept unless max |x| < silence_threshold (fp32 compare;
 * NaN propagates into the maximum as in sad_window_absmax_run, so it is kept).
 *   offsets   [max_candidates] int64: the kept windows' ABSOLUTE arena offsets,
 *             compacted in file order, then time order (an order-preserving
 *             prefix scan), ready for sad_frontend_run_windows(wav, wav_len, ..);
 *             entries past the kept count are not written;
 *   row_start [n_files + 1] int64: file f's kept windows are rows
 *             [row_start[f], row_start[f+1]) of offsets; row_start[n_files] is
 *             the kept count.
 * max_candidates bounds the candidates examined (the caller knows the file
 * lengths; candidates past it are dropped).  ws: sad_scan_select_workspace_size. */
int sad_scan_select_workspace_size(int64_t n_files, int64_t max_candidates, size_t* bytes);
int sad_scan_select_run(const float* wav, int64_t wav_len, const int64_t* file_start, const int64_t* file_len,
                        int64_t n_files, int64_t window, int64_t hop, float silence_threshold,
                        int64_t max_candidates, int64_t* offsets, int64_t* row_start, void* ws, size_t ws_bytes,
                        void* stream);
/* Per-file post-processing of merged logits [B, C] fp32 (C = N + 1 <= 128, last
 * column Real), file f owning rows [row_start[f], row_start[f+1]) (DEVICE int64
 * [n_files + 1], as sad_scan_select_run writes it; clamped to [0, B]):
 *   probs [B, C] fp32 = sigmoid(logits); with smooth != 0 each column is then
 *         filtered along its file's rows as scipy gaussian_filter1d(sigma=2)
 *         does (17 float64 taps, mode reflect, float64 accumulation rounded to
 *         fp32; never across a file boundary) and each row is divided by its
 *         fp32 sum when that is > 0;
 *   label [B] int32: -1 = Real (p_real >= threshold and every synthetic p <
 *         threshold), else the first argmax of the synthetic columns;
 *   mean  [n_files, C] float64: column means of a file's final probs, summed in
 *         a fixed order; zeros for a file without rows.
 * ws: sad_scan_post_workspace_size bytes. */
int sad_scan_post_workspace_size(int64_t B, int32_t C, int32_t smooth, size_t* bytes);
int sad_scan_post_run(const float* logits, int64_t B, int32_t C, const int64_t* row_start, int64_t n_files,
                      float threshold, int32_t smooth, float* probs, int32_t* label, double* mean, void* ws,
                      size_t ws_bytes, void* stream);

/* Replaces torchvision.transforms.Resize((512,512)) + repeat(3,1,1)
 * (inference_runner.py:172-174) for callers that want the image itself:
 * map [n, h, w] fp32 -> img [n, out_h, out_w] in `dtype` (one channel: the
 * reference's three channels are identical and are folded into conv1). */
int sad_resize_run(const float* map, int64_t n, int32_t h, int32_t w, int32_t out_h,
                   int32_t out_w, int32_t dtype, void* img, void* stream);

/* --------------------------------------------------------------- backbone */
/* Replaces timm.create_model('resnet18', num_classes=0).forward_features +
 * head[0:2] (AdaptiveAvgPool2d + Flatten) at inference_runner.py:35,49-51:
 * standardised map -> (fused) resize -> ResNet-18 -> pooled [B, 512] fp32. */
typedef struct sad_backbone_plan sad_backbone_plan;

/* params: host fp32 arrays in timm state-dict order, for each conv:
 *   conv weight [Cout, Cin, KH, KW], then its BN: weight, bias, running_mean,
 *   running_var  (5 pointers per conv+BN; conv1 has Cin = 3).
 * Order: conv1/bn1, then for layer1..4, block 0..1: conv1/bn1, conv2/bn2,
 * [downsample.0/downsample.1 for block 0 of layer2..4].  n_params must be
 * 5 * 20 = 100.  BN is folded (eps 1e-5) and weights are re-laid out
 * [Cout][KH][KW][Cin] in `dtype` on the current device.
 * map_h, map_w: 1..512 each.  The stem's in-kernel resize is the plain bilinear
 * filter (UPSAMPLING ONLY: what torchvision's antialiased Resize((512,512))
 * reduces to when it enlarges); a side above 512 would be point-sampled, so it
 * is refused with SAD_ERR_ARG before any allocation (*out untouched). */
int sad_backbone_plan_create(const float* const* params, int32_t n_params, int32_t dtype,
                             int32_t map_h, int32_t map_w, sad_backbone_plan** out);
int sad_backbone_plan_destroy(sad_backbone_plan* plan);
/* Device workspace bytes needed by sad_backbone_run for a micro-batch of
 * `micro_batch` segments (the run processes B in chunks of micro_batch). */
int sad_backbone_workspace_size(const sad_backbone_plan* plan, int64_t micro_batch, size_t* bytes);
/* map: [B, map_h, map_w] fp32 standardised maps; feats: [B, 512] fp32. */
int sad_backbone_run(const sad_backbone_plan* plan, const float* map, int64_t B,
                     int64_t micro_batch, float* feats, void* workspace, size_t ws_bytes,
                     void* stream);
/* Same from already-resized images: img [B, 512, 512] fp32 = ONE channel of
 * the reference's [B, 3, 512, 512] input (its 3 channels are identical,
 * inference_runner.py:173; the caller checks that). */
int sad_backbone_run_img(const sad_backbone_plan* plan, const float* img, int64_t B,
                         int64_t micro_batch, float* feats, void* workspace, size_t ws_bytes,
                         void* stream);
/* Same from images whose 3 channels may DIFFER: img3 [B, 3, 512, 512] fp32, the
 * reference's general model input (its load-time check feeds
 * torch.randn(2,3,512,512), inference_runner.py:119-122 / model_merger.py:
 * 148-151); conv1 runs per channel in fp32 (not folded), the rest as above. */
int sad_backbone_run_img3(const sad_backbone_plan* plan, const float* img3, int64_t B,
                          int64_t micro_batch, float* feats, void* workspace, size_t ws_bytes,
                          void* stream);
/* Debug/parity entry: run only the fused resize+stem (conv1+bn1+relu+maxpool)
 * on B maps, writing NHWC [B,128,128,64] in the plan's dtype (SAD_BF16X3: 128
 * bf16 per pixel, [hi 32 | lo 32] per 32 channels).  The maps are the plan's
 * map_h x map_w, both <= 512: the resize is upsampling only, no antialias.
 * B <= 65535; B = 0 launches nothing. */
int sad_backbone_stem_run(const sad_backbone_plan* plan, const float* map, int64_t B,
                          void* out, void* stream);
/* Debug/parity entry: the same fused stem on already resized images, exactly
 * one of img [B,512,512] (the folded stems of sad_backbone_run_img) and img3
 * [B,3,512,512] (the distinct-channel stem of sad_backbone_run_img3) non-null;
 * out as above. */
int sad_backbone_stem_run_img(const sad_backbone_plan* plan, const float* img, const float* img3,
                              int64_t B, void* out, void* stream);
/* Debug/parity entry: layer4 output NHWC [B,16,16,512] (plan dtype) for B <=
 * micro_batch, in addition to the pooled features. */
int sad_backbone_run_debug(const sad_backbone_plan* plan, const float* map, int64_t B,
                           float* feats, void* layer4_out, void* workspace, size_t ws_bytes,
                           void* stream);

/* One chunk with the layer4 activation kept (evidence maps, below): exactly one
 * of map [B, map_h, map_w] and img [B, 512, 512] non-null; B <= the micro-batch
 * the workspace was sized for (sad_backbone_workspace_size(B) bytes at least;
 * SAD_ERR_NOMEM otherwise).  feats [B, 512] fp32; l4_out: caller-owned
 * [B, 16, 16, 512] in the plan's activation layout (SAD_BF16 / SAD_F16: 2 B per
 * value; SAD_F32: 4 B; SAD_BF16X3: 1024 bf16 per pixel, [hi 32 | lo 32] per 32
 * channels).  It runs the un-pooled path of sad_backbone_run_debug.
 * NOTE: this entry pools the STORED, rounded activation, while
 * sad_backbone_run fuses the pool into the last conv (fp32 accumulators).  Its
 * features can therefore differ from the ordinary run's by the activation
 * rounding; they are exactly the mean of l4_out. */
int sad_backbone_run_keep(const sad_backbone_plan* plan, const float* map, const float* img, int64_t B,
                          float* feats, void* l4_out, void* workspace, size_t ws_bytes, void* stream);

/* Shared-trunk ensembles: the ResNet-18 plan split after layer3.  Reference
 * training only ever changes layer4 and the head, so sub-models trained on one
 * frozen trunk differ in layer4 alone: the trunk (stem, layer1-3; 13.83 of the
 * 18.13 GFLOP per segment) runs once and each sub-model's tail (layer4 +
 * average pool) runs on its output.  Every sub-model keeps a full
 * sad_backbone_plan; an entry uses the part of the plan it names.  Trunk and
 * tail issue exactly the launches sad_backbone_run* issues for their part on
 * the same micro-batch, so trunk_run followed by tail_run equals
 * sad_backbone_run / sad_backbone_run_img bit for bit.
 *
 * l3: layer3's output, NHWC [B, 32, 32, 256] in the plan's activation layout:
 *   SAD_BF16    bf16, 256 values per pixel (512 B)
 *   SAD_F16     fp16 (IEEE binary16), 256 values per pixel (512 B)
 *   SAD_F32     fp32, 256 values per pixel (1 KiB)
 *   SAD_BF16X3  split-bf16, 512 bf16 per pixel (1 KiB): per group of 32
 *               channels [hi(32) | lo(32)], hi = bf16(x), lo = bf16(x - hi)
 * Exactly one of map ([B, map_h, map_w] fp32) and img ([B, 512, 512] fp32, as
 * sad_backbone_run_img) is non-null.  trunk_run and tail_run take a workspace
 * of sad_backbone_workspace_size(micro_batch) bytes. */
int sad_backbone_trunk_run(const sad_backbone_plan* plan, const float* map, const float* img,
                           int64_t B, int64_t micro_batch, void* l3_out, void* workspace,
                           size_t ws_bytes, void* stream);
/* layer4 + average pool of `plan` on l3 -> feats [B, 512] fp32; l3 is only read. */
int sad_backbone_tail_run(const sad_backbone_plan* plan, const void* l3, int64_t B,
                          int64_t micro_batch, float* feats, void* workspace, size_t ws_bytes,
                          void* stream);
/* Per micro-batch chunk: the trunk of trunk_plan once, then the tail of each
 * of tail_plans[0..n_tails) on it -> feats[t] [B, 512] fp32.  Tails must have
 * the trunk's dtype and map size (SAD_ERR_ARG otherwise).  The workspace holds
 * the chunk's layer3 activation beside the run's buffers. */
int sad_backbone_shared_workspace_size(const sad_backbone_plan* trunk_plan, int64_t micro_batch,
                                       size_t* bytes);
int sad_backbone_shared_run(const sad_backbone_plan* trunk_plan,
                            const sad_backbone_plan* const* tail_plans, int32_t n_tails,
                            const float* map, const float* img, int64_t B, int64_t micro_batch,
                            float* const* feats, void* workspace, size_t ws_bytes, void* stream);

/* Deeper timm ResNets (resnet34/50/101/152, the
 * `--model-name` choices of submodel_trainer.py:51 / model_merger.py:24 /
 * inference_runner.py:77 backbone_name), on the same kernels: fused
 * resize+stem, block-conv GEMMs (downsample folded into the block's last GEMM
 * as extra K columns), the implicit-GEMM conv for Bottleneck identity adds,
 * then the average pool.  Replaces timm.create_model(name, num_classes=0)
 * .forward_features + global pool:  map -> pooled [B, num_features] fp32.
 * block: SAD_BASIC_BLOCK (resnet18/34: conv1/bn1, conv2/bn2 per block) or
 * SAD_BOTTLENECK (resnet50/101/152: conv1/bn1, conv2/bn2, conv3/bn3, width =
 * planes, expansion 4, stride on conv2 as timm).  layers: blocks per stage
 * ([3,4,6,3] for resnet34/50).  params: 5 pointers per conv+BN in timm
 * state-dict order (conv1/bn1 first; per block its convs, then
 * downsample.0/downsample.1 where present).  dtype SAD_BF16X3 with
 * SAD_BOTTLENECK runs every conv with the fourth split product W_lo.X_lo too
 * (|dlogit| <= 1e-3 on resnet50; environment SAD_DEEP_X4=0: three products).
 * map_h, map_w: 1..512 each, as sad_backbone_plan_create (the stem's resize is
 * upsampling only, no antialias; a larger side is refused with SAD_ERR_ARG
 * before any allocation, *out untouched). */
#define SAD_BASIC_BLOCK 0
#define SAD_BOTTLENECK 1
typedef struct sad_resnet_plan sad_resnet_plan;
int sad_resnet_plan_create(const float* const* params, int32_t n_params, int32_t block,
                           const int32_t* layers, int32_t dtype, int32_t map_h, int32_t map_w,
                           sad_resnet_plan** out);
int sad_resnet_plan_destroy(sad_resnet_plan* plan);
/* pooled feature width: 512 (BasicBlock) or 2048 (Bottleneck) */
int sad_resnet_num_features(const sad_resnet_plan* plan, int32_t* n);
int sad_resnet_workspace_size(const sad_resnet_plan* plan, int64_t micro_batch, size_t* bytes);
/* map: [B, map_h, map_w] fp32; feats: [B, num_features] fp32 */
int sad_resnet_run(const sad_resnet_plan* plan, const float* map, int64_t B, int64_t micro_batch,
                   float* feats, void* workspace, size_t ws_bytes, void* stream);
/* same from resized images img [B, 512, 512] fp32 (one of the 3 identical channels) */
int sad_resnet_run_img(const sad_resnet_plan* plan, const float* img, int64_t B, int64_t micro_batch,
                       float* feats, void* workspace, size_t ws_bytes, void* stream);

/* same from [B, 3, 512, 512] fp32 images with possibly distinct channels */
int sad_resnet_run_img3(const sad_resnet_plan* plan, const float* img3, int64_t B, int64_t micro_batch,
                        float* feats, void* workspace, size_t ws_bytes, void* stream);
/* Debug/parity entry: only this plan's stem (with its fourth split product
 * where the plan carries it), exactly one of map [B,map_h,map_w], img
 * [B,512,512] and img3 [B,3,512,512] non-null; out: NHWC [B,128,128,64] in the
 * plan's dtype, laid out as sad_backbone_stem_run's. */
int sad_resnet_stem_run(const sad_resnet_plan* plan, const float* map, const float* img,
                        const float* img3, int64_t B, void* out, void* stream);

/* sad_backbone_run_keep for the deep plans: one chunk (B <= the micro-batch the
 * workspace was sized for), exactly one of map and img non-null, feats
 * [B, num_features] fp32, l4_out caller-owned [B, 16, 16, num_features] in the
 * plan's activation layout (as above; SAD_BF16X3: 2 num_features bf16 per
 * pixel).  The same note applies: the features are the pool of the stored,
 * rounded activation (here the ordinary run pools it too). */
int sad_resnet_run_keep(const sad_resnet_plan* plan, const float* map, const float* img, int64_t B,
                        float* feats, void* l4_out, void* workspace, size_t ws_bytes, void* stream);

/* Kernel-level timing of the backbone's block-conv launches (bench.py's
 * roofline of the dominant kernel): between begin and end, every block-conv
 * launch of sad_backbone_run* is bracketed by HIP events on its stream.  end()
 * synchronises those events and returns, for the launches of tile `variant`
 * (0 = all), the summed kernel time, the number of KERNEL launches (a conv
 * whose operands pass the 2 GiB buffer range runs as several image-range
 * launches inside one bracket; each counts, so total_ms / launches is the
 * average kernel duration rocprofv3 reports) and their algorithmic FLOPs
 * (2*M*Cout*K with K the conv taps [+ the downsample], never the identity
 * shortcut's columns). */
int sad_profile_begin(void);
int sad_profile_end(int32_t variant, double* total_ms, int64_t* launches, double* flops);

/* ------------------------------------------------------------------ heads */
/* Replaces BinaryClassifier.head (inference_runner.py:36-48) for N sub-models
 * and ModularMultiHeadClassifier.forward (inference_runner.py:62-73).
 * params: per head, host fp32, in nn.Sequential index order:
 *   2.weight [512,512], 2.bias, 3.{weight,bias,running_mean,running_var},
 *   6.weight [256,512], 6.bias, 7.{weight,bias,running_mean,running_var},
 *   10.weight [2,256], 10.bias            (14 pointers per head)
 * feat_index[h]: which backbone's pooled features head h reads (0..n_feat-1). */
typedef struct sad_heads_plan sad_heads_plan;

int sad_heads_plan_create(const float* const* params, int32_t n_heads, const int32_t* feat_index,
                          int32_t n_feat, sad_heads_plan** out);
/* Same with the backbone feature width feat_dim (2.weight is [512, feat_dim];
 * 2048 for Bottleneck ResNets, whose head is Linear(2048, 512),
 * inference_runner.py:39 with base.num_features); feats are [B, feat_dim]. */
int sad_heads_plan_create_dim(const float* const* params, int32_t n_heads, const int32_t* feat_index,
                              int32_t n_feat, int32_t feat_dim, sad_heads_plan** out);
int sad_heads_plan_destroy(sad_heads_plan* plan);
int sad_heads_workspace_size(const sad_heads_plan* plan, int64_t B, size_t* bytes);
/* What sad_heads_merge_run will do with this plan: grouped = 1 when the second
 * Linear of all heads runs as one grouped launch (the hidden columns are in
 * head order: rank(h) == h below), 0 for one launch per head; row_range = the
 * rows per GEMM launch (a larger B runs as several ranges). */
int sad_heads_plan_info(const sad_heads_plan* plan, int32_t* grouped, int64_t* row_range);
/* feats: n_feat pointers to [B, feat_dim] fp32 (the pointer of a feature group
 * no head reads may be NULL); logits: [B, N, 2] fp32 (per head [Real,
 * Synthetic]) or NULL; merged: [B, N+1] fp32 = [syn_1..syn_N, mean_i real_i].
 * A short workspace or a NULL pointer of a used group is refused before any
 * launch; a bad feat_dim or feat_index is refused by plan_create (a failed
 * plan_create leaves nothing allocated).  Any B the workspace admits runs: the
 * GEMMs take B as row ranges that keep their operands inside the 2 GiB buffer
 * range (N = 6: 174,592 rows per range), and a row's value does not depend on
 * its position in the batch.
 *
 * Workspace layout after a run, stable for tests (tests/test_gpu_heads.py
 * reads the intermediate activations from it):
 *   y1  [B][N*512] fp32 at the start: relu(bn1(Linear1(feats))).  Head h's 512
 *       columns sit at 512 * rank(h), rank ordering the heads by
 *       (feat_index[h], h): the heads of one backbone are neighbours, because
 *       one GEMM per backbone writes them.
 *   y2  [B][N*256] fp32 at float offset B*N*512: relu(bn2(Linear2(y1))), head h
 *       at column 256 * h.
 * The row ranges write into this one layout. */
int sad_heads_merge_run(const sad_heads_plan* plan, const float* const* feats, int64_t B,
                        float* logits, float* merged, void* workspace, size_t ws_bytes,
                        void* stream);

/* --------------------------------------------------------------- evidence */
/* Evidence maps: Grad-CAM of one head's target logit on its backbone's layer4
 * activation, exact and without a backward pass through any conv (DESIGN.md
 * 5e).  The reference has no counterpart; the model is the reference's
 * (BinaryClassifier, inference_runner.py:36-51, eval mode).
 *
 * For window b and head h:  j = feat_index[h];  A = backbone j's layer4 output
 * [16, 16, C] as sad_*_run_keep stores it (C = 512 or 2048, HW = 256);  f = the
 * pooled features of the same run;  cls = 0 (Real) or 1 (Synthetic).
 *   1. masks  m1 = (y1 > 0), m2 = (y2 > 0) from the head's own forward on f (a
 *      unit at exactly 0 is off, as in torch's ReLU gradient);
 *   2. g[b, h, :] = W1^T (m1 * (W2^T (m2 * W3[cls, :]))), fp32, W1 / W2 the
 *      BN-folded weights as the heads plan holds them:  g = d logit[cls] / d f;
 *   3. E[b, h, y, x] = (1 / HW) sum_c g[b, h, c] A[b, y, x, c]: signed, fp32,
 *      unnormalised.  Positive E is evidence for the target; ReLU and scaling to
 *      [0, 1] are display steps on the host.
 * By construction sum_yx E[b, h] = g . f, and logit[cls] = g . f + beta(masks).
 *
 * sad_heads_grad_run: step 2 for every head, after sad_heads_merge_run on the
 * same B rows.  workspace: merge_run's, untouched since (y1 / y2 in the layout
 * above; only read).  g_out [n_heads][B][feat_dim] fp32.  Two GEMMs per head,
 * (B x 256)(256 x 512) then (B x 512)(512 x feat_dim), on the f32 implicit-GEMM
 * kernel, in row ranges as merge_run: a row's result does not depend on its
 * position in the batch.  The transposed folded weights and one row range of
 * scratch are allocated by the FIRST call on a plan (which also waits for
 * `stream` once, so it cannot be graph-captured); a plan that never explains
 * allocates nothing.  Calls on ONE plan share that scratch: they must not run
 * concurrently on different streams. */
int sad_heads_grad_run(const sad_heads_plan* plan, const void* workspace, int64_t B, int32_t cls, float* g_out,
                       void* stream);
/* Step 3 for the n_maps heads that read one backbone, in ONE pass over its
 * activation.  l4 [B, hw, C] in the layout of `dtype` (sad_dtype; SAD_BF16X3:
 * 2 C bf16 per pixel, value = hi + lo in fp32); g: n_maps HOST-array pointers
 * to DEVICE [B][C] fp32 (g_out + h B feat_dim of sad_heads_grad_run);
 * out [B][n_maps][hw] fp32.  fp32 accumulation in a fixed order, no atomics:
 * the output is bit-reproducible and independent of B, of a window's position
 * in the batch and of n_maps.  SAD_ERR_ARG before any launch for a null
 * pointer (l4, g, any g[m], out), C not a positive multiple of 64, hw < 1,
 * n_maps outside 1..16, or n_maps * C > 32768 (the gradients stay in LDS). */
int sad_evidence_run(const void* l4, int32_t dtype, int64_t B, int32_t hw, int32_t C, const float* const* g,
                     int32_t n_maps, float* out, void* stream);

/* ------------------------------------------------------------- operators */
/* One NHWC convolution (+ folded-BN bias, optional residual add, optional
 * ReLU) on the implicit-GEMM MFMA kernel the backbone uses: the building block
 * of timm's BasicBlock (conv -> bn -> [+ shortcut] -> act).  Exposed for op-level
 * parity tests and tile tuning.
 * in [N,H,W,Cin], wt [Cout,k,k,Cin] (dtype), bias [Cout] fp32, res/out
 * [N,Ho,Wo,Cout] (dtype; res may be NULL), Ho = (H + 2 pad - k)/stride + 1.
 * variant: 0 = the backbone's choice, 1..8 = tile variants (csrc/conv.hip). */
int sad_conv2d_run(const void* in, int64_t N, int32_t H, int32_t W, int32_t Cin, const void* wt,
                   const float* bias, const void* res, void* out, int32_t Cout, int32_t k,
                   int32_t stride, int32_t pad, int32_t relu, int32_t dtype, int32_t variant,
                   void* stream);

/* One GEMM = conv(in0) + 1x1 shortcut(in1) (+ bias [+ res], optional ReLU) on
 * the block-conv kernels the backbone uses for timm's BasicBlock (conv2 -> bn2
 * -> + shortcut -> act2, the shortcut being the identity or downsample.0/1).
 * wt: [Cout][wt_ld] with wt_ld >= k*k*Cin + Cin1 (0 = exactly that): the conv
 * taps, then the shortcut's weights (identity matrix or folded 1x1 conv) as the
 * next Cin1 K columns; in1 may be NULL (plain conv).  Shortcut pixel =
 * (oy*ss1, ox*ss1) of in1 [N,H1,W1,Cin1].  res (NULL or NHWC [N,Ho,Wo,Cout],
 * same dtype) is an identity shortcut added in the epilogue instead; it needs
 * the halo kernel (bf16, 3x3/s1/p1, H and W multiples of 16).
 * variant: 0 = default, 9..18 = implicit-GEMM tiles, 20 = halo (block.hip, halo.hip);
 * | SAD_CONV_FOUR_PRODUCTS with dtype SAD_BF16X3: also W_lo.X_lo (the deep
 * Bottleneck plans' form, on variants 9 / 13 / 15; 0 picks among them). */
#define SAD_CONV_FOUR_PRODUCTS 0x10000
int sad_block_conv_run(const void* in0, int64_t N, int32_t H, int32_t W, int32_t Cin, const void* in1,
                       int32_t H1, int32_t W1, int32_t Cin1, int32_t ss1, const void* wt, int32_t wt_ld,
                       const float* bias, const void* res, void* out, int32_t Cout, int32_t k,
                       int32_t stride, int32_t pad, int32_t relu, int32_t dtype, int32_t variant,
                       void* stream);

/* One whole layer1 BasicBlock (timm resnet18 layer1.{0,1} with BN folded:
 * out = relu(conv3x3(relu(conv3x3(x; w1) + b1); w2) + b2 + x), 64 channels,
 * stride 1) as ONE fused kernel (csrc/l1block.hip, variant 40): the
 * intermediate stays in LDS and the identity comes from the input patch.
 * Replaces the two sad_block_conv_run launches (conv1; conv2 + res) of a
 * layer1 block -- reference inference_runner.py:49-51 (timm forward_features).
 * bf16, or fp16 with SAD_L1_BLOCK_F16.  x, out: NHWC [N,H,W,64] bf16 (must
 * not overlap), H and W multiples of 16; w1, w2: [64][w_ld] bf16, k = tap * 64
 * + ci; b1, b2: [64] fp32.  ablate: reserved, pass 0, or SAD_L1_BLOCK_F16:
 * every tensor is fp16 (SAD_F16) instead of bf16.  Async on `stream`. */
#define SAD_L1_BLOCK_F16 0x10000
int sad_l1_block_run(const void* x, int64_t N, int32_t H, int32_t W, const void* w1, int32_t w1_ld,
                     const float* b1, const void* w2, int32_t w2_ld, const float* b2, void* out,
                     int32_t ablate, void* stream);

/* --------------------------------------------------------------- training */
/* The submodel_trainer.py hot path: the train-mode
 * front end of SpectrogramDataset.__getitem__ (:139-214, transforms :463-471),
 * and the train-mode ResNet-18 forward (BatchNorm with batch statistics) plus
 * the backward / clip / AdamW of train() (:250-302, setup :606-660).  These are
 * op-level entries; sad/train.py composes them into the step.  Activations are
 * NHWC in `dtype`; statistics, gradients and master weights are fp32. */

/* FrequencyMasking(15) + TimeMasking(35) (fill 0.0) on the top-db clamped dB
 * map, then (x - mean) / (std_unbiased + 1e-6)  (:107-114,191-199).
 * masks: device int32 [n,4] = {f0, f1, t0, t1} (rows [f0,f1), columns [t0,t1)
 * zeroed; f0 == f1 = no mask) or NULL.  db, out_map: [n, n_mels, n_frames]. */
int sad_specaug_norm_run(const float* db, int64_t n, int32_t n_mels, int32_t n_frames, const int32_t* masks,
                         float* out_map, void* stream);
/* transforms.Resize((512,512)) (:200) then RandomResizedCrop's
 * resized_crop(i, j, h, w, (out_hw, out_hw)) (:466), one plane of the three
 * identical channels (:203).  boxes: device int32 [n,4] = {i, j, h, w} in the
 * 512x512 image, or NULL (= the val transform Resize((512,512)), :470).
 * UPSAMPLING ONLY: both stages are the plain bilinear filter, which is what
 * torchvision's antialiased resize reduces to when it enlarges.  So the map
 * sides must be <= 512 and out_hw >= the box sides (the trainer: 128 x 251 maps,
 * out_hw = 512); a downsampling call does NOT apply torchvision's antialias
 * filter.  Boxes must lie inside the 512x512 image (not checked).  n <= 65535. */
int sad_crop_resize_run(const float* map, int64_t n, int32_t h, int32_t w, const int32_t* boxes, int32_t out_hw,
                        int32_t dtype, void* img, void* stream);
/* fp32 OIHW conv weight -> compute layout in dtype.  mode 0: [Cout][k][k][Cin]
 * (forward); 1: [Cin][k][k][Cout] with flipped taps (stride-1 dgrad as a conv of
 * dy); 2: [Cout][64], k = ky*7+kx, input channels summed (fp32 stem); 3: OIHW
 * copy; 4: [Cout][64], k = ky*8+kx (7x7 in an 8x8 grid), channels summed (bf16
 * training stem). */
int sad_pack_conv_weight_run(const float* w, int32_t cout, int32_t cin, int32_t k, int32_t mode, int32_t dtype,
                             void* out, void* stream);
/* timm conv1 7x7/2/p3 WITHOUT bn1 (train-mode BN needs the raw output):
 * img [n, ih, iw] (dtype) -> out NHWC [n, oh, ow, 64]; col_ws >= n*oh*ow*64
 * elements of dtype; w_packed from mode 2. */
int sad_stem_conv_run(const void* img, int64_t n, int32_t ih, int32_t iw, const void* w_packed, void* col_ws,
                      size_t ws_bytes, void* out, int32_t dtype, void* stream);
/* bf16 training stem in one pass (conv.hip stem_bf16_kernel<false, true>):
 * conv1 7x7/2 of the bf16 image with w_packed (pack mode 4), bn1 in train mode
 * (batch statistics -> stats, running stats updated as sad_bn_stats_run), ReLU,
 * maxpool 3x3/2 -> out NHWC [n, 128, 128, 64] bf16.  The raw 256x256 conv map
 * is never stored: the kernel pools sign(gamma) * conv and sums conv, conv^2
 * per channel.  ws: sad_stem_train_workspace_size bytes. */
int sad_stem_train_workspace_size(int64_t n, size_t* bytes);
int sad_stem_train_run(const void* img, int64_t n, const void* w_packed, const float* gamma, const float* beta,
                       float eps, float momentum, float* running_mean, float* running_var, float* stats, void* out,
                       void* ws, size_t ws_bytes, void* stream);
/* Train-mode conv + BatchNorm statistics: out NHWC [N, Ho, Wo, Cout] = raw conv
 * (no bias) of x with w_packed (pack mode 0), and stats / running stats as
 * sad_bn_stats_run computes them on out.  bf16 on the block-conv variants 13,
 * 15, 20 and 25 sums the statistics in the conv epilogue from the fp32
 * accumulators (out is not re-read; *fused_out = 1); otherwise (fp32, other
 * shapes) the conv is followed by the bn_reduce pass over out (*fused_out = 0).
 * ws: sad_conv_bn_train_workspace_size bytes. */
int sad_conv_bn_train_workspace_size(int64_t N, int32_t H, int32_t W, int32_t Cout, int32_t k, int32_t stride,
                                     int32_t pad, size_t* bytes);
int sad_conv_bn_train_run(const void* x, int64_t N, int32_t H, int32_t W, int32_t Cin, const void* w_packed,
                          int32_t Cout, int32_t k, int32_t stride, int32_t pad, int32_t dtype, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean, float* running_var,
                          float* stats, void* out, float* ws, size_t ws_bytes, int32_t* fused_out, void* stream);
/* Workspace (bytes) of the BN entries for a [P, C] tensor. */
int sad_bn_workspace_size(int64_t P, int32_t C, size_t* bytes);
/* BatchNorm2d train-mode statistics of x NHWC [P, C]: stats = [mean | invstd |
 * scale = gamma*invstd | shift = beta - mean*scale] (4*C floats); running
 * stats (optional, both or neither) updated with momentum and the unbiased var. */
int sad_bn_stats_run(const void* x, int64_t P, int32_t C, int32_t dtype, const float* gamma, const float* beta,
                     float eps, float momentum, float* running_mean, float* running_var, float* stats, float* ws,
                     size_t ws_bytes, void* stream);
/* out = act(x*scale + shift [+ res] ) where res is added as-is (identity
 * shortcut) or, with res_stats, as res*rscale + rshift (downsample BN). */
int sad_bn_apply_run(const void* x, int64_t P, int32_t C, int32_t dtype, const float* stats, const void* res,
                     const float* res_stats, int32_t relu, void* out, void* stream);
/* bn1 + ReLU + maxpool 3x3/2/p1: x NHWC [n, H, W, C] raw conv1 -> out [n, Ho, Wo, C]. */
int sad_bn_relu_maxpool_run(const void* x, int64_t n, int32_t H, int32_t W, int32_t C, int32_t dtype,
                            const float* stats, void* out, void* stream);
/* CrossEntropyLoss on logits [B, C] fp32 (the trainer's pooled features, quirk
 * C1): dlogits = (softmax - onehot(target)) * scale; out[0] = sum of row
 * losses, out[1] = count of rows with argmax == target; pred (optional) [B] =
 * argmax (first maximum, outputs.max(1) at :281,346). */
int sad_ce_loss_run(const float* logits, const int64_t* target, int64_t B, int32_t C, float scale, float* dlogits,
                    float* out, int32_t* pred, void* stream);
/* The BinaryClassifier head in train mode (optional --head-loss of
 * submodel_trainer.py; the reference builds it at :613-625 and never calls it,
 * quirk C1): Linear(nf,512) -> BatchNorm1d(512) -> ReLU -> Dropout(p1) ->
 * Linear(512,256) -> BatchNorm1d(256) -> ReLU -> Dropout(p2) -> Linear(256,2).
 * Parameters are the head.* tensors (nn.Sequential indices 2, 3, 6, 7, 10),
 * fp32, device.  Dropout keeps element i of layer L (1, 2) when
 * u(seed, L, i) >= p, u from a splitmix64 hash (headtrain.hip hkeep), so the
 * backward regenerates the forward's masks from the same seed. */
typedef struct {
  const float *w2, *b2, *g3, *be3, *w6, *b6, *g7, *be7, *w10, *b10;
  float *rm3, *rv3, *rm7, *rv7; /* BN running statistics (updated in train mode) */
  int32_t in_features;          /* the backbone's num_features (512 / 2048) */
  float eps, momentum, p1, p2;  /* 1e-5, 0.1, 0.5, 0.3 in the reference */
} sad_head_params;
int sad_head_workspace_size(int64_t B, int32_t in_features, size_t* bytes);
/* feats [B, nf] -> logits [B, 2].  train: batch statistics (running stats
 * updated) and dropout; 0: eval (running stats, no dropout).  ws keeps the
 * activations the backward needs. */
int sad_head_train_forward_run(const sad_head_params* h, const float* feats, int64_t B, int32_t train, uint64_t seed,
                               float* logits, void* ws, size_t ws_bytes, void* stream);
/* After a train-mode forward with the same feats / seed / ws: dlogits [B, 2]
 * -> dfeats [B, nf] and grads = the head's parameter gradients, flat fp32 in
 * parameters() order (2.w, 2.b, 3.w, 3.b, 6.w, 6.b, 7.w, 7.b, 10.w, 10.b). */
int sad_head_train_backward_run(const sad_head_params* h, const float* feats, int64_t B, uint64_t seed,
                                const float* dlogits, float* dfeats, float* grads, void* ws, size_t ws_bytes,
                                void* stream);
/* BatchNorm2d train-mode backward through an optional ReLU:
 * dz = (dy | dpool[n][c]/pool_hw broadcast) * [y > 0 if y];  dbeta = sum dz,
 * dgamma = sum dz*xhat (written, or added if accumulate);  dx = gamma*invstd*
 * (dz - mean dz - xhat * mean(dz*xhat)).  x is the raw (pre-BN) tensor, stats
 * from sad_bn_stats_run; dz_out (optional) receives dz. */
int sad_bn_backward_run(const void* x, int64_t P, int32_t C, int32_t dtype, const float* stats, const float* gamma,
                        const void* dy, const float* dpool, int32_t pool_hw, const void* y, float* dgamma,
                        float* dbeta, int32_t accumulate, void* dz_out, void* dx, float* ws, size_t ws_bytes,
                        void* stream);
/* Conv weight gradient (wgrad.hip, hand-written MFMA, no im2col): dw
 * [Cout][Cin][k][k] fp32 = beta*dw + sum_p dy[p] (x) x[src(p, tap)], the
 * activation gathered per tap straight from NHWC x; split-K partials in ws
 * (sad_conv_wgrad_workspace_size bytes), reduced in a fixed order
 * (deterministic).  Cin, Cout multiples of 8 (bf16) / 4 (fp32). */
int sad_conv_wgrad_workspace_size(int64_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t k,
                                  int32_t stride, int32_t pad, int32_t dtype, size_t* bytes);
int sad_conv_wgrad_run(const void* x, int64_t N, int32_t H, int32_t W, int32_t Cin, const void* dy, int32_t Cout,
                       int32_t k, int32_t stride, int32_t pad, int32_t dtype, float beta, float* dw, void* ws,
                       size_t ws_bytes, void* stream);
/* Conv input gradient for any stride (wgrad.hip): dcol[p][j] = sum_co dy[p][co]
 * W[co][j] on the same MFMA kernel (w_oihw from pack mode 3, dy transposed
 * into ws), then the col2im gather into dx NHWC [N, H, W, Cin] (added to dx
 * if accumulate).  ws: sad_conv_dgrad_workspace_size bytes.  (Stride-1 3x3
 * dgrad runs as a block conv over dy with pack mode 1 weights instead.) */
int sad_conv_dgrad_workspace_size(int64_t N, int32_t Ho, int32_t Wo, int32_t Cout, int32_t Cin, int32_t k,
                                  int32_t dtype, size_t* bytes);
int sad_conv_dgrad_run(const void* dy, int64_t N, int32_t Ho, int32_t Wo, int32_t Cout, const void* w_oihw,
                       int32_t Cin, int32_t H, int32_t W, int32_t k, int32_t stride, int32_t pad, int32_t dtype,
                       int32_t accumulate, void* dx, void* ws, size_t ws_bytes, void* stream);
/* torch.nn.utils.clip_grad_norm_(params, max_norm) over one flat fp32 gradient
 * buffer (:276): norm_coef[0] = ||g||, norm_coef[1] = min(max_norm/(||g||+1e-6), 1);
 * g *= norm_coef[1].  ws >= 1024 doubles. */
int sad_clip_grad_norm_run(float* g, int64_t n, float max_norm, float* norm_coef, void* ws, size_t ws_bytes,
                           void* stream);
/* One conv weight inside the flat parameter buffer and its cached compute
 * copies (pack modes 0 / 1, either may be NULL) for sad_adamw_pack_run. */
typedef struct {
  int64_t offset; /* element offset of the OIHW weight in p */
  int32_t cout, cin, k, reserved;
  void* mode0;    /* [Cout][k][k][Cin] in dtype, or NULL */
  void* mode1;    /* [Cin][k][k][Cout], taps flipped, or NULL */
} sad_pack_seg;
/* sad_adamw_run + the updated conv weights written into their packed copies
 * (<= 16 segments): the trainer's next step needs no pack launches. */
int sad_adamw_pack_run(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                       float eps, float weight_decay, int64_t step, const sad_pack_seg* segs, int32_t nseg,
                       int32_t dtype, void* stream);
/* torch.optim.AdamW step `step` (1-based) over flat fp32 buffers (:648-652,278). */
int sad_adamw_run(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int64_t step, void* stream);
/* y += alpha * x (fp32): folds a step's layer3 gradient into its never-zeroed
 * .grad (quirk C4: layer3 is unfrozen at epochs//3 but not in the optimizer). */
int sad_axpy_run(float* y, const float* x, int64_t n, float alpha, void* stream);
/* Element-wise dtype conversion fp32 <-> bf16 (RNE) of n values: the mixed
 * trainer's hand-over between its fp32 frozen prefix (stem, layers 1-3) and
 * its bf16 layer4 (sad/train.py, submodel_trainer.py --precision mixed). */
int sad_cast_run(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream);
/* timm global average pool: x NHWC [B, hw, C] (dtype) -> out [B, C] fp32 (the
 * trainer's model(inputs), quirk C1). */
int sad_avgpool_run(const void* x, int64_t B, int32_t hw, int32_t C, int32_t dtype, float* out, void* stream);

/* -------------------------------------------------------------- synthetic */
/* Deterministic synthetic segments; bit-identical to
 * sad/synth.py up to rare 1-LSB float64 libm differences in the tone term.
 * pcm: [count, n_samples] int16, segments first_seg .. first_seg+count-1. */
int sad_synth_pcm(uint64_t seed, int64_t first_seg, int64_t count, int32_t n_samples,
                  int16_t* pcm, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAD_H_ */
