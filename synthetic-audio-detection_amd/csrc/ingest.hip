// ingest.hip -- the ingestion edge of the inference path on the device
// (SURVEY 8(f) row 1): a long file's PCM goes to HBM once, compact (int16 as
// it sits in the WAV), and everything from there on runs on the GPU:
//
//   interleaved PCM -> fp32 mono (+ zero pad)        sad_pcm_mono_run
//     preprocess_waveform, inference_runner.py:144-155 (torchaudio.load
//     normalize=True scaling, waveform.mean(dim=0), the pad to one window)
//   -> 32 kHz, torchaudio sinc_interp_hann           sad_resample_run
//     torchaudio.transforms.Resample(sr, 32000) at inference_runner.py:148
//     (lowpass_filter_width 6, rolloff 0.99; the polyphase kernel table is
//     built on the host in float64 and rounded once to fp32, as torchaudio does)
//   -> per-window max |x| for the silence skip       sad_window_absmax_run
//     slice_waveform, inference_runner.py:176-190 (piece.abs().max() < thr)
//   -> the front end reads the kept windows in place by sample offset
//     (sad_frontend_run_windows, frontend.hip): overlapping windows are never
//     copied, and nothing goes back to the host but one float per window.
//
// The mono / window kernels are HBM streaming work; the resampler is fp32-FMA
// work (K = 2 width + orig taps per output, 459 for 44.1 kHz): register-blocked
// over frames with the inputs staged in LDS (resample_wide_kernel).  No MFMA:
// a polyphase FIR is not GEMM-shaped enough to pay for one at fp32.
#include <math.h>

#include <vector>

#include "common.hpp"
#include "ingest.hpp"

namespace sad {

// ---- interleaved PCM [frames][channels] -> mono fp32 [out_len] -------------
// out[i] = (sum_c x[i][c]) / C for i < frames, 0 for frames <= i < out_len.
// The reference's waveform.mean(dim=0) runs on the CPU, where ATen's mean is
// sum(dim).div_(C): channels summed in order, then a true fp32 division (not a
// multiply by 1/C, which differs by an ulp for C = 3, 5, 6, ...); int16 is
// scaled by 1/32768 first (torchaudio.load normalize=True).  Bit-exact with
// the host for every channel count.
template <typename IT>
__global__ __launch_bounds__(256) void pcm_mono_kernel(const IT* __restrict__ x, int64_t frames, int channels,
                                                       float fc, float* __restrict__ out, int64_t out_len) {
  const float scale = sizeof(IT) == 2 ? (1.0f / 32768.0f) : 1.0f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < out_len;
       i += (int64_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    if (i < frames) {
      const IT* p = x + i * channels;
      float s = (float)p[0] * scale;
      for (int c = 1; c < channels; ++c) s += (float)p[c] * scale;
      v = channels == 1 ? s : s / fc;
    }
    out[i] = v;
  }
}

// ---- polyphase windowed-sinc resampler --------------------------------------
// torchaudio.functional.resample with orig/new reduced by their gcd:
//   xp = pad(x, (width, width + orig));  y = conv1d(xp, kernel[new][K], stride orig)
// so output m = j*new + p is  sum_k x[j*orig + k - width] * kernel[p][k]
// (x = 0 outside [0, n_in)), truncated to ceil(new * n_in / orig) samples.
// The table is stored transposed, kt[k][p], so the lanes of a wave (consecutive
// p of one j) read consecutive words, and x[j*orig + k - width] is one
// broadcast address per j.
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, int64_t n_in,
                                                       const float* __restrict__ kt, int orig, int nw, int width,
                                                       int K, float* __restrict__ y, int64_t n_out, int64_t y_len) {
  for (int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; m < y_len; m += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    if (m < n_out) {
      const int64_t j = m / nw;
      const int p = (int)(m - j * nw);
      const int64_t base = j * orig - width;  // x index of tap k = 0
      const int k0 = base < 0 ? (int)-base : 0;
      const int64_t kend = n_in - base;
      const int k1 = kend < K ? (int)kend : K;
      const float* xp = x + base;
      const float* kp = kt + p;
      for (int k = k0; k < k1; ++k) acc = fmaf(xp[k], kp[(int64_t)k * nw], acc);
    }
    y[m] = acc;
  }
}

// Many phases (nw >= 64: 44.1 / 22.05 kHz -> 32 kHz, nw = 320 / 640, K = 459 /
// 455): lanes own 64 consecutive phases p, a wave owns RS_R consecutive frames
// j (RS_R accumulators per lane), and K is walked in chunks of RS_KC taps: the
// chunk's input samples for the wave's frames are staged in LDS as xs[k][r]
// (frame-fastest, so one tap's RS_R inputs are 4 broadcast ds_read_b128), the
// tap's coefficient kt[k][p] is one coalesced load (the table stays in L2), and
// each tap costs RS_R FMAs per lane.  The sum runs over k in the same order as
// resample_kernel, so the two give identical results.
// (RS_R = 16 frames per wave, RS_KC = 64 taps per chunk, RS_WAVES = 4: ingest.hpp)
__global__ __launch_bounds__(256) void resample_wide_kernel(const float* __restrict__ x, int64_t n_in,
                                                            const float* __restrict__ kt, int orig, int nw, int width,
                                                            int K, float* __restrict__ y, int64_t n_out) {
  __shared__ __attribute__((aligned(16))) float xs[RS_WAVES][RS_KC][RS_R];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = blockIdx.y * 64 + lane;
  const bool pok = p < nw;
  const int64_t j0 = ((int64_t)blockIdx.x * RS_WAVES + wave) * RS_R;  // this wave's first frame
  float acc[RS_R];
#pragma unroll
  for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
  for (int kc = 0; kc < K; kc += RS_KC) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll 4
    for (int e = lane; e < RS_KC * RS_R; e += 64) {
      const int r = e % RS_R, k = e / RS_R;
      const int64_t i = (j0 + r) * orig + kc + k - width;
      xs[wave][k][r] = (kc + k < K && i >= 0 && i < n_in) ? x[i] : 0.f;
    }
    __syncthreads();
    const int kn = K - kc < RS_KC ? K - kc : RS_KC;
    const float* kp = kt + (int64_t)kc * nw + p;
#pragma unroll 4
    for (int k = 0; k < kn; ++k) {
      const float w = pok ? kp[(int64_t)k * nw] : 0.f;
      const float4* xr = (const float4*)&xs[wave][k][0];
#pragma unroll
      for (int q = 0; q < RS_R / 4; ++q) {
        const float4 v = xr[q];
        acc[4 * q + 0] = fmaf(v.x, w, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(v.y, w, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(v.z, w, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(v.w, w, acc[4 * q + 3]);
      }
    }
  }
  if (pok) {
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int64_t m = (j0 + r) * nw + p;
      if (m < n_out) y[m] = acc[r];
    }
  }
}

// ---- max |x| over each window [w*hop, w*hop + window) -------------------------
// torch.max propagates NaN, so a NaN sample makes the window's maximum NaN
// (and `NaN < thr` keeps the window, as in the reference)
__device__ __forceinline__ float nanmax(float a, float b) { return (b > a || b != b) ? b : a; }

__global__ __launch_bounds__(256) void window_absmax_kernel(const float* __restrict__ x, int64_t n, int64_t window,
                                                            int64_t hop, float* __restrict__ out) {
  __shared__ float red[4];
  const int64_t w = blockIdx.x;
  const int64_t b = w * hop;
  const int64_t e = b + window < n ? b + window : n;
  float m = 0.f;  // |x| >= 0: 0 is the identity (an empty window reports 0)
  for (int64_t i = b + threadIdx.x; i < e; i += blockDim.x) m = nanmax(m, fabsf(x[i]));
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[w] = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
}

static unsigned grid_for(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (unsigned)(g < 65536 ? (g > 0 ? g : 1) : 65536);
}

// ---- trainer ingestion: one launch per batch of stored files ------------------
// SpectrogramDataset.__getitem__'s load + resample + 2-segment rule
// (submodel_trainer.py:143-187 of the reference) for a whole batch: the files'
// samples sit as stored (interleaved int16 / fp32) in one byte arena, and file f
// gives rows 2f and 2f + 1 of out [2 n_files, seg_len].  With n_out the file's
// 32 kHz length, row 2f + s holds samples m = s * seg_len + i of the resampled
// mono signal (0 for m >= n_out); a file with n_out < 2 seg_len repeats its
// first segment, which is computed once and stored twice.  Every sample is
// pcm_mono_kernel's value fed to resample_kernel's sum (ascending k, one fmaf
// per tap; a tap outside the samples read multiplies a zero, which leaves the
// fp32 sum unchanged), so the rows are the bits the two-kernel path gives.
//
// A workgroup is one (file, tile) pair read from a table the host builds with
// the batch.  Three block-uniform forms share the kernel:
//   native    the file is at the target rate: mono mix straight to the rows;
//   per-output (nw < 64: 16 / 48 / 96 kHz) TI_TILE consecutive outputs; the mono
//             inputs they need are mixed into LDS once, each thread sums K taps;
//   wide      (nw >= 64: 44.1 / 22.05 kHz) resample_wide_kernel's blocking, 64
//             frames x 64 phases per tile, the mono mix done while staging.
// (TI_TILE = 1024 outputs per tile, TI_SPAN = 8192 LDS floats, TI_MAX_RATES = 8: ingest.hpp)
constexpr int TI_COLS = 6;        // file table columns

struct TrainRates {
  const float* kt[TI_MAX_RATES];  // nullptr: the target rate itself
  int orig[TI_MAX_RATES], nw[TI_MAX_RATES], width[TI_MAX_RATES], K[TI_MAX_RATES];
};

template <typename IT>
__device__ __forceinline__ void ti_tile(float* __restrict__ xs, const IT* __restrict__ x, int64_t n_read,
                                        int64_t n_out, int channels, const float* __restrict__ kt, int orig, int nw,
                                        int width, int K, int tile, int64_t seg_len, float* __restrict__ out0) {
  const float fc = (float)channels;
  const bool dup = n_out < 2 * seg_len;
  const int64_t M = dup ? seg_len : 2 * seg_len;  // samples to produce; row 2f + 1 follows row 2f in memory
  auto store = [&](int64_t m, float v) {
    if (m < M) {
      v = m < n_out ? v : 0.f;
      out0[m] = v;
      if (dup) out0[seg_len + m] = v;
    }
  };
  if (!kt) {  // native rate
    const int64_t m0 = (int64_t)tile * TI_TILE;
#pragma unroll
    for (int q = 0; q < TI_TILE / 256; ++q) {
      const int64_t m = m0 + q * 256 + threadIdx.x;
      if (m < M) store(m, ti_mono(x, m, n_read, channels, fc));
    }
    return;
  }
  if (nw < 64) {  // per-output form
    const int64_t m0 = (int64_t)tile * TI_TILE;
    const int64_t j0 = m0 / nw;
    const int64_t span0 = j0 * orig - width;  // x index of xs[0]
    const int64_t mlast = (m0 + TI_TILE < M ? m0 + TI_TILE : M) - 1;
    const int cnt = mlast < m0 ? 0 : (int)((mlast / nw - j0) * orig) + K;  // <= TI_SPAN (checked on the host)
    for (int e = threadIdx.x; e < cnt; e += 256) xs[e] = ti_mono(x, span0 + e, n_read, channels, fc);
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < TI_TILE / 256; ++q) {
      const int64_t m = m0 + q * 256 + threadIdx.x;
      if (m >= M) continue;
      const int64_t j = m / nw;
      const int p = (int)(m - j * nw);
      const float* xr = xs + (int)((j - j0) * orig);
      const float* kp = kt + p;
      float acc = 0.f;
      for (int k = 0; k < K; ++k) acc = fmaf(xr[k], kp[k * nw], acc);
      store(m, acc);
    }
    return;
  }
  // wide form: tile = frame tile * phase blocks + phase block
  const int npb = (nw + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = (tile % npb) * 64 + lane;
  const bool pok = p < nw;
  const int64_t j0 = ((int64_t)(tile / npb) * RS_WAVES + wave) * RS_R;  // this wave's first frame
  float* xw = xs + wave * (RS_KC * RS_R);                               // xw[k][r]
  float acc[RS_R];
#pragma unroll
  for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
  for (int kc = 0; kc < K; kc += RS_KC) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll 4
    for (int e = lane; e < RS_KC * RS_R; e += 64) {
      const int r = e % RS_R, k = e / RS_R;
      const int64_t i = (j0 + r) * orig + kc + k - width;
      xw[e] = kc + k < K ? ti_mono(x, i, n_read, channels, fc) : 0.f;
    }
    __syncthreads();
    const int kn = K - kc < RS_KC ? K - kc : RS_KC;
    const float* kp = kt + (int64_t)kc * nw + p;
#pragma unroll 4
    for (int k = 0; k < kn; ++k) {
      const float w = pok ? kp[(int64_t)k * nw] : 0.f;
      const float4* xr = (const float4*)(xw + k * RS_R);
#pragma unroll
      for (int q = 0; q < RS_R / 4; ++q) {
        const float4 v = xr[q];
        acc[4 * q + 0] = fmaf(v.x, w, acc[4 * q + 0]);
        acc[4 * q + 1] = fmaf(v.y, w, acc[4 * q + 1]);
        acc[4 * q + 2] = fmaf(v.z, w, acc[4 * q + 2]);
        acc[4 * q + 3] = fmaf(v.w, w, acc[4 * q + 3]);
      }
    }
  }
  if (pok) {
#pragma unroll
    for (int r = 0; r < RS_R; ++r) store((j0 + r) * nw + p, acc[r]);
  }
}

// file_table [n_files][TI_COLS] int64: byte offset, frames read, total frames,
// channels, encoding, rate index; tiles [n_tiles][2] int32: file, tile
__global__ __launch_bounds__(256) void train_ingest_kernel(const unsigned char* __restrict__ arena,
                                                           const int64_t* __restrict__ file_table, int n_files,
                                                           const int32_t* __restrict__ tiles, TrainRates rates,
                                                           int64_t seg_len, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float xs[TI_SPAN];
  const int f = tiles[2 * (int64_t)blockIdx.x], tile = tiles[2 * (int64_t)blockIdx.x + 1];
  if (f < 0 || f >= n_files || tile < 0) return;  // block-uniform
  const int64_t* ft = file_table + (int64_t)f * TI_COLS;
  const int64_t n_read = ft[1], total = ft[2];
  const int channels = (int)ft[3], enc = (int)ft[4], ri = (int)ft[5];
  const float* kt = rates.kt[ri];
  const int orig = rates.orig[ri], nw = rates.nw[ri], width = rates.width[ri], K = rates.K[ri];
  const int64_t n_out = kt ? (nw * total + orig - 1) / orig : total;
  float* out0 = out + 2 * (int64_t)f * seg_len;
  const unsigned char* x = arena + ft[0];
  if (enc == SAD_PCM_I16)
    ti_tile<int16_t>(xs, (const int16_t*)x, n_read, n_out, channels, kt, orig, nw, width, K, tile, seg_len, out0);
  else
    ti_tile<float>(xs, (const float*)x, n_read, n_out, channels, kt, orig, nw, width, K, tile, seg_len, out0);
}

// tiles of one file (0 when the form cannot take the rate: the per-output
// form's input span must fit TI_SPAN)
static int64_t ti_file_tiles(bool native, const RsGeometry& q, int64_t total_frames, int64_t seg_len) {
  const int64_t n_out = native ? total_frames : (q.nw * total_frames + q.orig - 1) / q.orig;
  const int64_t M = n_out < 2 * seg_len ? seg_len : 2 * seg_len;
  if (native) return (M + TI_TILE - 1) / TI_TILE;
  if (q.nw < 64) {
    if (!rs_per_output_fits(q)) return 0;
    return (M + TI_TILE - 1) / TI_TILE;
  }
  const int64_t frames = (M + q.nw - 1) / q.nw;
  return (frames + RS_WAVES * RS_R - 1) / (RS_WAVES * RS_R) * ((q.nw + 63) / 64);
}

}  // namespace sad

using namespace sad;

extern "C" int sad_pcm_mono_run(const void* pcm, int32_t format, int64_t frames, int32_t channels, float* out,
                                int64_t out_len, void* stream) {
  SAD_REQUIRE(format == SAD_PCM_I16 || format == SAD_PCM_F32, "format must be SAD_PCM_I16 or SAD_PCM_F32");
  SAD_REQUIRE(frames >= 0 && channels >= 1 && channels <= 64, "frames / channels");
  SAD_REQUIRE(out_len >= frames, "out_len < frames");
  if (out_len == 0) return SAD_OK;
  SAD_REQUIRE(out && (pcm || frames == 0), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  const float fc = (float)channels;
  if (format == SAD_PCM_I16)
    hipLaunchKernelGGL(pcm_mono_kernel<int16_t>, dim3(grid_for(out_len)), dim3(256), 0, s, (const int16_t*)pcm,
                       frames, channels, fc, out, out_len);
  else
    hipLaunchKernelGGL(pcm_mono_kernel<float>, dim3(grid_for(out_len)), dim3(256), 0, s, (const float*)pcm, frames,
                       channels, fc, out, out_len);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

extern "C" int sad_resample_plan_create(int32_t orig_freq, int32_t new_freq, sad_resample_plan** out) {
  SAD_REQUIRE(out, "null out");
  SAD_REQUIRE(orig_freq > 0 && new_freq > 0, "sample rates must be positive");
  // torchaudio _get_sinc_resample_kernel (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), float64
  const RsGeometry geo = rs_geometry(orig_freq, new_freq);
  const int orig = geo.orig, nw = geo.nw, width = geo.width, K = geo.K;
  const int lpw = 6;
  const double base = geo.base;
  SAD_REQUIRE((int64_t)K * nw * 4 <= (256ll << 20),
              "resample ratio too irregular: the polyphase table would exceed 256 MiB");
  std::vector<float> kt((size_t)K * nw);
  const double scale = base / orig;
  for (int p = 0; p < nw; ++p) {
    for (int k = 0; k < K; ++k) {
      // idx = arange(-width, width + orig, float64) / orig; t = arange(0, -new, -1) / new + idx, where
      // the integer arange / new is a default-dtype (fp32) division, promoted to float64 by the add
      const float ph = (float)(-p) / (float)nw;
      double t = ((double)ph + (double)(k - width) / orig) * base;
      t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
      const double c = cos(t * M_PI / lpw / 2);
      const double window = c * c;
      t *= M_PI;
      const double v = (t == 0.0 ? 1.0 : sin(t) / t) * (window * scale);  // kernels *= window * scale
      kt[(size_t)k * nw + p] = (float)v;
    }
  }
  auto* pl = new sad_resample_plan();
  pl->orig_freq = orig_freq;
  pl->new_freq = new_freq;
  pl->orig = orig;
  pl->nw = nw;
  pl->width = width;
  pl->K = K;
  (void)hipGetDevice(&pl->device);
  if (hipMalloc((void**)&pl->d_kt, kt.size() * 4) != hipSuccess ||
      hipMemcpy(pl->d_kt, kt.data(), kt.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(pl->d_kt);
    delete pl;
    set_error("sad_resample_plan_create: device allocation / upload failed");
    return SAD_ERR_NOMEM;
  }
  *out = pl;
  return SAD_OK;
}

extern "C" int sad_resample_plan_destroy(sad_resample_plan* p) {
  if (!p) return SAD_OK;
  (void)hipFree(p->d_kt);
  delete p;
  return SAD_OK;
}

extern "C" int sad_resample_out_len(const sad_resample_plan* p, int64_t n_in, int64_t* n_out) {
  SAD_REQUIRE(p && n_out && n_in >= 0, "null plan / n_out, or n_in < 0");
  SAD_REQUIRE(n_in <= (INT64_MAX - p->orig) / p->nw, "n_in too large");
  *n_out = (p->nw * n_in + p->orig - 1) / p->orig;  // ceil(new * length / orig)
  return SAD_OK;
}

extern "C" int sad_resample_run(const sad_resample_plan* p, const float* x, int64_t n_in, float* y, int64_t y_len,
                                void* stream) {
  int64_t n_out = 0;
  if (int rc = sad_resample_out_len(p, n_in, &n_out)) return rc;
  SAD_REQUIRE(y_len >= n_out, "y_len < the resampled length (sad_resample_out_len)");
  if (y_len == 0) return SAD_OK;
  SAD_REQUIRE(y && (x || n_in == 0), "null pointer");
  hipStream_t s = (hipStream_t)stream;
  if (p->nw >= 64 && n_out > 0) {
    const int64_t frames = (n_out + p->nw - 1) / p->nw;
    const int64_t gx = (frames + RS_WAVES * RS_R - 1) / (RS_WAVES * RS_R);
    SAD_REQUIRE(gx < (1ll << 31), "input too long for one launch");
    hipLaunchKernelGGL(resample_wide_kernel, dim3((unsigned)gx, (unsigned)((p->nw + 63) / 64)), dim3(256), 0, s, x,
                       n_in, p->d_kt, p->orig, p->nw, p->width, p->K, y, n_out);
    SAD_CHECK_HIP(hipGetLastError());
    if (y_len > n_out) SAD_CHECK_HIP(hipMemsetAsync(y + n_out, 0, (size_t)(y_len - n_out) * 4, s));
    return SAD_OK;
  }
  hipLaunchKernelGGL(resample_kernel, dim3(grid_for(y_len)), dim3(256), 0, s, x, n_in, p->d_kt, p->orig, p->nw,
                     p->width, p->K, y, n_out, y_len);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

extern "C" int sad_window_absmax_run(const float* wav, int64_t n, int64_t window, int64_t hop, int64_t n_windows,
                                     float* out, void* stream) {
  SAD_REQUIRE(n >= 0 && window > 0 && hop > 0 && n_windows >= 0, "n / window / hop / n_windows");
  SAD_REQUIRE(n_windows == 0 || (n_windows - 1) * hop < n, "window start past the end of the waveform");
  SAD_REQUIRE(n_windows <= 0x7FFFFFFF, "too many windows for one launch");
  if (n_windows == 0) return SAD_OK;
  SAD_REQUIRE(wav && out, "null pointer");
  hipLaunchKernelGGL(window_absmax_kernel, dim3((unsigned)n_windows), dim3(256), 0, (hipStream_t)stream, wav, n,
                     window, hop, out);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

// ---- trainer ingestion ---------------------------------------------------------
extern "C" int sad_train_ingest_need_frames(int32_t orig_freq, int32_t new_freq, int64_t seg_len, int64_t* need) {
  SAD_REQUIRE(need, "null need");
  SAD_REQUIRE(orig_freq > 0 && new_freq > 0, "sample rates must be positive");
  SAD_REQUIRE(seg_len > 0 && seg_len <= (1ll << 28), "seg_len must be in [1, 2^28]");
  if (orig_freq == new_freq) {
    *need = 2 * seg_len;
    return SAD_OK;
  }
  // the last of the 2 seg_len outputs, m = j new + p, reads inputs up to j orig + K - 1 - width
  const RsGeometry q = rs_geometry(orig_freq, new_freq);
  *need = (2 * seg_len - 1) / q.nw * q.orig + q.orig + q.width;
  return SAD_OK;
}

extern "C" int sad_train_ingest_file_tiles(int32_t orig_freq, int32_t new_freq, int64_t total_frames,
                                           int64_t seg_len, int64_t* n_tiles) {
  SAD_REQUIRE(n_tiles, "null n_tiles");
  SAD_REQUIRE(orig_freq > 0 && new_freq > 0, "sample rates must be positive");
  SAD_REQUIRE(seg_len > 0 && seg_len <= (1ll << 28), "seg_len must be in [1, 2^28]");
  SAD_REQUIRE(total_frames >= 0 && total_frames <= (1ll << 40), "total_frames must be in [0, 2^40]");
  const RsGeometry q = rs_geometry(orig_freq, new_freq);
  const int64_t t = ti_file_tiles(orig_freq == new_freq, q, total_frames, seg_len);
  SAD_REQUIRE(t > 0, "sample rate not supported by the batched kernel: few phases and a long input span");
  *n_tiles = t;
  return SAD_OK;
}

extern "C" int sad_train_ingest_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                                    const int64_t* d_file_table, int64_t n_files, const int32_t* d_tiles,
                                    int64_t n_tiles, const sad_resample_plan* const* rate_plans, int32_t n_rates,
                                    int64_t seg_len, float* out, void* stream) {
  SAD_REQUIRE(seg_len > 0 && seg_len <= (1ll << 28), "seg_len must be in [1, 2^28]");
  SAD_REQUIRE(n_files >= 0 && n_files <= (1 << 20), "n_files must be in [0, 2^20]");
  SAD_REQUIRE(n_rates >= 1 && n_rates <= TI_MAX_RATES, "n_rates must be in [1, 8]");
  SAD_REQUIRE(arena_bytes >= 0, "arena_bytes < 0");
  if (n_files == 0) return SAD_OK;
  SAD_REQUIRE(arena && file_table && d_file_table && d_tiles && rate_plans && out, "null pointer");
  TrainRates rates = {};
  RsGeometry geo[TI_MAX_RATES] = {};
  for (int r = 0; r < n_rates; ++r) {
    const sad_resample_plan* p = rate_plans[r];  // nullptr: the target rate
    if (!p) continue;
    rates.kt[r] = p->d_kt;
    geo[r].orig = rates.orig[r] = p->orig;
    geo[r].nw = rates.nw[r] = p->nw;
    geo[r].width = rates.width[r] = p->width;
    geo[r].K = rates.K[r] = p->K;
  }
  int64_t tiles = 0;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t* t = file_table + f * TI_COLS;
    const int64_t off = t[0], n_read = t[1], total = t[2], ch = t[3], enc = t[4], ri = t[5];
    SAD_REQUIRE(ch >= 1 && ch <= 64, "file table: channels must be in [1, 64]");
    SAD_REQUIRE(enc == SAD_PCM_I16 || enc == SAD_PCM_F32, "file table: encoding must be SAD_PCM_I16 or SAD_PCM_F32");
    SAD_REQUIRE(ri >= 0 && ri < n_rates, "file table: rate index out of range");
    SAD_REQUIRE(total >= 0 && total <= (1ll << 40) && n_read >= 0 && n_read <= total,
                "file table: frames read / total frames");
    SAD_REQUIRE(off >= 0 && off % 16 == 0, "file table: a file must start at a multiple of 16 bytes");
    const int64_t bytes = n_read * ch * (enc == SAD_PCM_I16 ? 2 : 4);
    SAD_REQUIRE(off <= arena_bytes && bytes <= arena_bytes - off, "file table: a file lies past the end of the arena");
    const int64_t ft = ti_file_tiles(rate_plans[ri] == nullptr, geo[ri], total, seg_len);
    SAD_REQUIRE(ft > 0, "sample rate not supported by the batched kernel: few phases and a long input span");
    tiles += ft;
  }
  SAD_REQUIRE(n_tiles == tiles, "n_tiles is not the sum of the files' tile counts (sad_train_ingest_file_tiles)");
  SAD_REQUIRE(tiles < (1ll << 31), "too many tiles for one launch");
  hipLaunchKernelGGL(train_ingest_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)arena, d_file_table, (int)n_files, d_tiles, rates, seg_len, out);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}
