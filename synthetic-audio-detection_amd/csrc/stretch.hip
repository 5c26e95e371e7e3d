// stretch.hip -- time stretch and pitch shift of a training batch on the device
// (submodel_trainer.py --wave-stretch): the five kinds of the reference's
// audio_augmneter.py that go through librosa (speed_up, slow_down, pitch_up,
// pitch_down, time_pitch_shift; :55-76, :140-145, clip :190).
// tests/stretch_ref.py states the contract in float64 and says where it departs
// from librosa; include/sad.h ("time and pitch") the tables.
//
//   time_stretch(y, r) = istft(phase_vocoder(stft(y), r), round(len / r))
//   pitch_shift(y, n)  = resample_ratio(time_stretch(y, q), q, len), q = 2^(-n / 12)
//
// Four stages, each batched over files through a table of eight int64 per file
// (grid.y is the file, blocks past a file's end leave at once):
//   stft      one workgroup per frame: 2048 windowed samples, a radix-2 complex
//             FFT in LDS (2048 float2 = 16 KB, twiddles 8 KB), bins 0..1024 out
//   vocoder   polar: every bin -> (|D|, angle as a Q0.32 fraction of a turn).
//             The accumulator acc_t = angle(D_0) + sum_{u < t} (angle D[i_u + 1] -
//             angle D[i_u]) mod one turn is a prefix sum of 32-bit integers over
//             the output frames, chunked like the phaser's scan (waveaug.hip):
//               A  per (chunk of PV_CHUNK steps, bin): the chunk's sum
//               B  per bin: exclusive scan of the chunk sums, serial over chunks
//               C  per (chunk, bin): walk the steps again from the chunk's base
//             Integer addition wraps exactly and is associative: the scan's
//             shape does not touch the bits, no precision is lost with length.
//             The step position s = t rate is float64.
//   istft     per frame: Hermitian extension, inverse FFT, window -> workspace;
//             then a gather: each output sample sums its at most four frames in
//             ascending order and divides by the same frames' squared windows
//   resample  one output per lane, position i / rho in float64, taps ascending
// sad_wave_stretch_run chains them per file with the SAME kernels on stage
// tables that a one-thread kernel derives from the stretch table, so
// its result is the stage entries' bit for bit.  Launches for any batch: plan,
// mono, 7 per stretch (stft, polar, A, B, C, frames, gather) x 2, resample = 17.
// No atomics, no allocation; nothing depends on the other files of the batch.
#include <float.h>
#include <math.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "ingest.hpp"

namespace sad {

constexpr int ST_N = 2048, ST_HOP = 512, ST_BINS = 1025, ST_PAD = 1024;
constexpr int ST_THREADS = 256;
constexpr int PV_CHUNK = 64;  // output frames per scan chunk
constexpr int ST_COLS = 8;    // stage table columns
enum { SC_IN = 0, SC_NIN = 1, SC_OUT = 2, SC_NOUT = 3, SC_RATE = 4, SC_FLAGS = 5, SC_WS = 6 };
enum { SF_CLIP = 1, SF_FINAL = 2 };
constexpr int SW_COLS = 8;    // stretch table columns
constexpr int SW_FT_COLS = 6;
enum { SW_KIND = 0, SW_RATE = 1, SW_STEPS = 2, SW_NOUT = 3, SW_OUT = 4, SW_PRATE = 5 };
enum { SW_SPEED_UP = 6, SW_SLOW_DOWN = 7, SW_PITCH_UP = 8, SW_PITCH_DOWN = 9, SW_TIME_PITCH = 10 };
constexpr int SW_TABLES = 7;  // stage tables of the batch entry: stft, vocoder, istft (x 2), resample
constexpr double SW_ROLLOFF = 0.99, SW_LPW = 6.0;
constexpr int64_t SW_MAX_FRAMES = 1ll << 31;  // samples of one file

__host__ __device__ inline double st_f64(int64_t bits) {
  union {
    int64_t i;
    double d;
  } u;
  u.i = bits;
  return u.d;
}
__host__ __device__ inline int64_t st_bits(double d) {
  union {
    int64_t i;
    double d;
  } u;
  u.d = d;
  return u.i;
}
__host__ __device__ inline int64_t st_align(int64_t n) { return (n + 15) & ~15ll; }
__host__ __device__ inline int64_t st_min(int64_t a, int64_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------- geometry
// One time stretch at `rate` of a signal of `total` samples of which the first
// n_need output samples are wanted: output sample m sums the synthesis frames
// t <= (m + 1024) / 512; step t reads the analysis frames int(t rate) and
// int(t rate) + 1; analysis frame f reads the samples below 512 f + 1024.
struct StretchGeo {
  int64_t n;      // output samples computed
  int64_t nF;     // synthesis frames computed
  int64_t nT;     // analysis frames computed
  int64_t n_in;   // input samples read
};
__host__ __device__ inline StretchGeo st_geometry(int64_t total, double rate, int64_t n_need) {
  StretchGeo g;
  const int64_t len = (int64_t)rint((double)total / rate);
  g.n = st_min(n_need, len);
  if (g.n <= 0) {
    g.n = g.nF = g.nT = g.n_in = 0;
    return g;
  }
  const int64_t T = 1 + total / ST_HOP;
  const int64_t steps = (int64_t)ceil((double)T / rate);
  g.nF = st_min(steps, (g.n - 1 + ST_PAD) / ST_HOP + 1);
  g.nT = st_min(T, (int64_t)((double)(g.nF - 1) * rate) + 2);
  g.n_in = st_min(total, (g.nT - 1) * ST_HOP + ST_PAD);
  return g;
}
// the input samples the first n_out outputs of resample_ratio read
__host__ __device__ inline int64_t rs_need(double rho, int64_t n_out) {
  if (n_out <= 0) return 0;
  const double c = SW_ROLLOFF * (rho < 1.0 ? rho : 1.0);
  const int64_t n = (int64_t)ceil((double)(n_out - 1) / rho + SW_LPW / c);
  return n > 0 ? n : 0;
}
__host__ __device__ inline int64_t pv_chunks(int64_t n_frames) { return (n_frames + PV_CHUNK - 1) / PV_CHUNK; }
__host__ __device__ inline int64_t pv_ws_bytes(int64_t T, int64_t n_frames) {
  return st_align(T * ST_BINS * 8) + st_align(pv_chunks(n_frames) * ST_BINS * 4);
}
__host__ __device__ inline int64_t istft_frames(int64_t avail, int64_t length) {
  return st_min(avail, (length + ST_N + ST_HOP - 1) / ST_HOP);
}
__host__ __device__ inline int64_t istft_ws_bytes(int64_t avail, int64_t length) {
  return st_align(istft_frames(avail, length) * ST_N * 4);
}

__host__ __device__ inline int64_t sw_tables_bytes(int64_t n_files) {
  return st_align(n_files * SW_TABLES * ST_COLS * 8);
}

// The stage rows of one file of the batch entry and its workspace bytes.
// rows [SW_TABLES][ST_COLS]: stft0, pv0, istft0, stft1, pv1, istft1, resample;
// every offset is relative to the workspace, except a row flagged SF_FINAL,
// whose output offset is relative to the output arena.
__host__ __device__ inline int64_t sw_plan(int64_t kind, int64_t total, int64_t present, double rate, double prate,
                                           int64_t n_out, int64_t out_off, int64_t ws_off, int64_t* rows) {
  for (int i = 0; i < SW_TABLES * ST_COLS; ++i) rows[i] = 0;
  if (kind < SW_SPEED_UP) return 0;
  const bool pitch = kind >= SW_PITCH_UP, two = kind == SW_TIME_PITCH;
  // the chain's stretch rates, first to last, and the lengths between them
  const double r0 = two ? rate : (pitch ? prate : rate), r1 = prate;
  const int n_st = two ? 2 : 1;
  const int64_t len0 = (int64_t)rint((double)total / r0);  // after the first stretch
  // backwards: what each stage has to deliver
  int64_t need_last = n_out;  // of the last stretch's output
  if (pitch) need_last = rs_need(prate, n_out);
  StretchGeo g[2];
  if (two) {
    g[1] = st_geometry(len0, r1, need_last);
    g[0] = st_geometry(total, r0, g[1].n_in);
  } else {
    g[0] = st_geometry(total, r0, need_last);
  }
  int64_t off = ws_off;
  const int64_t mono_off = off, n_mono = st_min(present, g[0].n_in);
  off += st_align(n_mono * 4);
  int64_t in_off = mono_off, in_n = n_mono;
  for (int s = 0; s < n_st; ++s) {
    const double r = s == 0 ? r0 : r1;
    const bool last = s == n_st - 1, final_ = last && !pitch;
    int64_t* st = rows + (3 * s + 0) * ST_COLS;
    int64_t* pv = rows + (3 * s + 1) * ST_COLS;
    int64_t* is = rows + (3 * s + 2) * ST_COLS;
    const int64_t spec = off;
    off += st_align(g[s].nT * ST_BINS * 8);
    const int64_t pvws = off;
    off += pv_ws_bytes(g[s].nT, g[s].nF);
    const int64_t ospec = off;
    off += st_align(g[s].nF * ST_BINS * 8);
    const int64_t isws = off;
    off += istft_ws_bytes(g[s].nF, g[s].n);
    st[SC_IN] = in_off, st[SC_NIN] = in_n, st[SC_OUT] = spec, st[SC_NOUT] = g[s].nT;
    pv[SC_IN] = spec, pv[SC_NIN] = g[s].nT, pv[SC_OUT] = ospec, pv[SC_NOUT] = g[s].nF, pv[SC_RATE] = st_bits(r),
    pv[SC_WS] = pvws;
    is[SC_IN] = ospec, is[SC_NIN] = g[s].nF, is[SC_NOUT] = g[s].n, is[SC_WS] = isws;
    if (final_) {
      is[SC_OUT] = out_off, is[SC_NOUT] = n_out, is[SC_FLAGS] = SF_CLIP | SF_FINAL;
    } else {
      is[SC_OUT] = off;
      in_off = off, in_n = g[s].n;
      off += st_align(g[s].n * 4);
    }
  }
  if (pitch) {
    int64_t* rs = rows + 6 * ST_COLS;
    rs[SC_IN] = in_off, rs[SC_NIN] = in_n, rs[SC_OUT] = out_off, rs[SC_NOUT] = n_out, rs[SC_RATE] = st_bits(prate),
    rs[SC_FLAGS] = SF_CLIP | SF_FINAL;
  }
  return off - ws_off;
}

// ------------------------------------------------------------------ kernels
__device__ __forceinline__ float st_window(int n) { return 0.5f - 0.5f * cospif((float)n * (1.0f / 1024.0f)); }
__device__ __forceinline__ float st_clip(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

__device__ __forceinline__ void st_twiddles(float2* tw, int tid) {
  for (int m = tid; m < ST_N / 2; m += ST_THREADS) {
    float s, c;
    sincospif((float)m * (1.0f / 1024.0f), &s, &c);
    tw[m] = make_float2(c, -s);  // exp(-2 pi i m / 2048)
  }
}

// in-place radix-2 decimation in time on bit-reversed input; ends synchronised
__device__ __forceinline__ void st_fft(float2* buf, const float2* tw, int tid, bool inverse) {
  __syncthreads();
  for (int s = 0; s < 11; ++s) {
    const int half = 1 << s;
    for (int j = tid; j < ST_N / 2; j += ST_THREADS) {
      const int pos = j & (half - 1);
      const int i0 = ((j >> s) << (s + 1)) + pos, i1 = i0 + half;
      float2 w = tw[pos << (10 - s)];
      if (inverse) w.y = -w.y;
      const float2 a = buf[i0], b = buf[i1];
      const float bx = b.x * w.x - b.y * w.y, by = b.x * w.y + b.y * w.x;
      buf[i0] = make_float2(a.x + bx, a.y + by);
      buf[i1] = make_float2(a.x - bx, a.y - by);
    }
    __syncthreads();
  }
}
__device__ __forceinline__ int st_brev(int i) { return (int)(__brev((unsigned)i) >> 21); }

struct StBases {
  const unsigned char* in;
  unsigned char* out;
  unsigned char* out_final;
  unsigned char* ws;
};
__device__ __forceinline__ unsigned char* st_out(const StBases& b, const int64_t* row) {
  return ((row[SC_FLAGS] & SF_FINAL) ? b.out_final : b.out) + row[SC_OUT];
}

__global__ __launch_bounds__(ST_THREADS) void stft2048_kernel(StBases b, const int64_t* __restrict__ table) {
  __shared__ float2 buf[ST_N];
  __shared__ float2 tw[ST_N / 2];
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t f = blockIdx.x;
  if (f >= row[SC_NOUT]) return;  // block-uniform
  const int tid = threadIdx.x;
  const float* x = (const float*)(b.in + row[SC_IN]);
  const int64_t n_in = row[SC_NIN], s0 = f * ST_HOP - ST_PAD;
  st_twiddles(tw, tid);
  for (int n = tid; n < ST_N; n += ST_THREADS) {
    const int64_t i = s0 + n;
    const float v = (i >= 0 && i < n_in) ? x[i] : 0.f;
    buf[st_brev(n)] = make_float2(v * st_window(n), 0.f);
  }
  st_fft(buf, tw, tid, false);
  float2* out = (float2*)st_out(b, row) + f * ST_BINS;
  for (int k = tid; k < ST_BINS; k += ST_THREADS) out[k] = buf[k];
}

// (|D|, angle in Q0.32 turns) of every bin of the frames present
__global__ __launch_bounds__(ST_THREADS) void pv_polar_kernel(StBases b, const int64_t* __restrict__ table) {
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t n = row[SC_NIN] * ST_BINS;
  const int64_t e = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (e >= n) return;
  const float2 d = ((const float2*)(b.in + row[SC_IN]))[e];
  const float turns = atan2f(d.y, d.x) * 0.15915494309189535f;
  const uint32_t q = (uint32_t)(int64_t)rint((double)turns * 4294967296.0);
  ((uint2*)(b.ws + row[SC_WS]))[e] = make_uint2(__float_as_uint(hypotf(d.x, d.y)), q);
}

template <bool EMIT>
__global__ __launch_bounds__(ST_THREADS) void pv_walk_kernel(StBases b, const int64_t* __restrict__ table) {
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t n_out = row[SC_NOUT], T = row[SC_NIN], c = blockIdx.x;
  if (c * PV_CHUNK >= n_out) return;
  const double rate = st_f64(row[SC_RATE]);
  const uint2* polar = (const uint2*)(b.ws + row[SC_WS]);
  uint32_t* sums = (uint32_t*)(b.ws + row[SC_WS] + st_align(T * ST_BINS * 8)) + c * ST_BINS;
  float2* out = (float2*)st_out(b, row);
  const int64_t t1 = st_min(n_out, (c + 1) * PV_CHUNK);
  for (int k = threadIdx.x; k < ST_BINS; k += ST_THREADS) {
    uint32_t acc = EMIT ? sums[k] : 0u;
    for (int64_t t = c * PV_CHUNK; t < t1; ++t) {
      const double s = (double)t * rate;
      const int64_t i = (int64_t)s;
      const uint2 p0 = i < T ? polar[i * ST_BINS + k] : make_uint2(0u, 0u);
      const uint2 p1 = i + 1 < T ? polar[(i + 1) * ST_BINS + k] : make_uint2(0u, 0u);
      if (EMIT) {
        const float a = (float)(s - (double)i);
        const float mag = (1.0f - a) * __uint_as_float(p0.x) + a * __uint_as_float(p1.x);
        float sn, cs;
        sincospif((float)(int32_t)acc * 4.656612873077393e-10f, &sn, &cs);  // 2^-31: half turns
        out[t * ST_BINS + k] = make_float2(mag * cs, mag * sn);
      }
      acc += p1.y - p0.y;
    }
    if (!EMIT) sums[k] = acc;
  }
}

// B: the chunk sums of one bin -> the accumulator at each chunk's first step
__global__ __launch_bounds__(ST_THREADS) void pv_combine_kernel(StBases b, const int64_t* __restrict__ table) {
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t n_out = row[SC_NOUT], T = row[SC_NIN];
  const int k = blockIdx.x * ST_THREADS + threadIdx.x;
  if (n_out <= 0 || k >= ST_BINS) return;
  const uint2* polar = (const uint2*)(b.ws + row[SC_WS]);
  uint32_t* sums = (uint32_t*)(b.ws + row[SC_WS] + st_align(T * ST_BINS * 8));
  uint32_t base = T > 0 ? polar[k].y : 0u;
  const int64_t nch = pv_chunks(n_out);
  for (int64_t c = 0; c < nch; ++c) {
    const uint32_t s = sums[c * ST_BINS + k];
    sums[c * ST_BINS + k] = base;
    base += s;
  }
}

__global__ __launch_bounds__(ST_THREADS) void istft_frames_kernel(StBases b, const int64_t* __restrict__ table) {
  __shared__ float2 buf[ST_N];
  __shared__ float2 tw[ST_N / 2];
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t t = blockIdx.x;
  if (t >= istft_frames(row[SC_NIN], row[SC_NOUT])) return;
  const int tid = threadIdx.x;
  const float2* S = (const float2*)(b.in + row[SC_IN]) + t * ST_BINS;
  st_twiddles(tw, tid);
  for (int k = tid; k < ST_BINS; k += ST_THREADS) {
    float2 v = S[k];
    if (k == 0 || k == ST_N / 2) {
      v.y = 0.f;  // irfft reads the real part alone
    } else {
      buf[st_brev(ST_N - k)] = make_float2(v.x, -v.y);
    }
    buf[st_brev(k)] = v;
  }
  st_fft(buf, tw, tid, true);
  float* fr = (float*)(b.ws + row[SC_WS]) + t * ST_N;
  for (int n = tid; n < ST_N; n += ST_THREADS) fr[n] = buf[n].x * (1.0f / ST_N) * st_window(n);
}

__global__ __launch_bounds__(ST_THREADS) void istft_gather_kernel(StBases b, const int64_t* __restrict__ table) {
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t len = row[SC_NOUT];
  const int64_t m = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (m >= len) return;
  const int64_t nF = istft_frames(row[SC_NIN], len);
  const float* fr = (const float*)(b.ws + row[SC_WS]);
  const int64_t p = m + ST_PAD;
  const int64_t lo = p < ST_N ? 0 : (p - ST_N) / ST_HOP + 1, hi = st_min(nF - 1, p / ST_HOP);
  float acc = 0.f, wsum = 0.f;
  for (int64_t t = lo; t <= hi; ++t) {
    const int n = (int)(p - t * ST_HOP);
    const float w = st_window(n);
    acc += fr[t * ST_N + n];
    wsum += w * w;
  }
  if (wsum > FLT_MIN) acc /= wsum;
  ((float*)st_out(b, row))[m] = (row[SC_FLAGS] & SF_CLIP) ? st_clip(acc) : acc;
}

__global__ __launch_bounds__(ST_THREADS) void resample_ratio_kernel(StBases b, const int64_t* __restrict__ table) {
  const int64_t* row = table + (int64_t)blockIdx.y * ST_COLS;
  const int64_t n_out = row[SC_NOUT], n_in = row[SC_NIN];
  const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i >= n_out) return;
  const float* x = (const float*)(b.in + row[SC_IN]);
  const double rho = st_f64(row[SC_RATE]);
  const double c = SW_ROLLOFF * (rho < 1.0 ? rho : 1.0), half = SW_LPW / c;
  const double pos = (double)i / rho;
  const float cf = (float)c;
  int64_t j = (int64_t)floor(pos - half);
  const int64_t j1 = st_min((int64_t)floor(pos + half) + 1, n_in - 1);
  if (j < 0) j = 0;
  float acc = 0.f;
  for (; j <= j1; ++j) {
    const double u = pos - (double)j;
    if (fabs(u) >= half) continue;
    const float arg = cf * (float)u;
    const float sinc = arg == 0.f ? 1.0f : sinpif(arg) / (3.14159265358979323846f * arg);
    const float cw = cospif(arg * (1.0f / 12.0f));
    acc = fmaf(x[j], cf * sinc * cw * cw, acc);
  }
  ((float*)st_out(b, row))[i] = (row[SC_FLAGS] & SF_CLIP) ? st_clip(acc) : acc;
}

// ---- the batch entry's two own kernels
// One thread walks the files in order (a file's workspace starts where the one
// before it ends): a few hundred operations per file.
__global__ __launch_bounds__(64) void stretch_plan_kernel(const int64_t* __restrict__ file_table,
                                                          const int64_t* __restrict__ sw_table, int n_files,
                                                          int64_t* __restrict__ tables) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t rows[SW_TABLES * ST_COLS];
  int64_t ws_off = sw_tables_bytes(n_files);
  for (int f = 0; f < n_files; ++f) {
    const int64_t* ft = file_table + (int64_t)f * SW_FT_COLS;
    const int64_t* sw = sw_table + (int64_t)f * SW_COLS;
    ws_off += sw_plan(sw[SW_KIND], ft[2], ft[1], st_f64(sw[SW_RATE]), st_f64(sw[SW_PRATE]), sw[SW_NOUT], sw[SW_OUT],
                      ws_off, rows);
    for (int s = 0; s < SW_TABLES; ++s)
      for (int c = 0; c < ST_COLS; ++c) tables[((int64_t)s * n_files + f) * ST_COLS + c] = rows[s * ST_COLS + c];
  }
}

template <typename IT>
__device__ __forceinline__ void sw_mono(const IT* __restrict__ x, int64_t n_read, int channels, float* out, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
  if (i < n) out[i] = ti_mono(x, i, n_read, channels, (float)channels);
}
__global__ __launch_bounds__(ST_THREADS) void stretch_mono_kernel(const unsigned char* __restrict__ arena,
                                                                  const int64_t* __restrict__ file_table,
                                                                  const int64_t* __restrict__ stft_table,
                                                                  unsigned char* __restrict__ ws) {
  const int64_t* ft = file_table + (int64_t)blockIdx.y * SW_FT_COLS;
  const int64_t* row = stft_table + (int64_t)blockIdx.y * ST_COLS;
  if ((int64_t)blockIdx.x * ST_THREADS >= row[SC_NIN]) return;
  float* out = (float*)(ws + row[SC_IN]);
  if ((int)ft[4] == SAD_PCM_I16)
    sw_mono<int16_t>((const int16_t*)(arena + ft[0]), ft[1], (int)ft[3], out, row[SC_NIN]);
  else
    sw_mono<float>((const float*)(arena + ft[0]), ft[1], (int)ft[3], out, row[SC_NIN]);
}

// -------------------------------------------------------------- host checks
enum StageKind { STG_STFT, STG_PV, STG_ISTFT, STG_RS };

static int64_t stage_in_bytes(StageKind k, const int64_t* r) {
  return k == STG_STFT || k == STG_RS ? r[SC_NIN] * 4 : r[SC_NIN] * ST_BINS * 8;
}
static int64_t stage_out_bytes(StageKind k, const int64_t* r) {
  return k == STG_ISTFT || k == STG_RS ? r[SC_NOUT] * 4 : r[SC_NOUT] * ST_BINS * 8;
}
static int64_t stage_ws_bytes(StageKind k, const int64_t* r) {
  return k == STG_PV ? pv_ws_bytes(r[SC_NIN], r[SC_NOUT]) : k == STG_ISTFT ? istft_ws_bytes(r[SC_NIN], r[SC_NOUT]) : 0;
}
// grid sizes of one stage over a host table of rows `table` (stride in rows)
struct StageGrid {
  int64_t a = 0, c = 0;  // stft: frames | pv: polar blocks, chunks | istft: frames, gather blocks | rs: blocks
};
static StageGrid stage_grid(StageKind k, const int64_t* table, int64_t n_files) {
  StageGrid g;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t* r = table + f * ST_COLS;
    int64_t a = 0, c = 0;
    if (k == STG_STFT) a = r[SC_NOUT];
    if (k == STG_PV && r[SC_NOUT] > 0)
      a = (r[SC_NIN] * ST_BINS + ST_THREADS - 1) / ST_THREADS, c = pv_chunks(r[SC_NOUT]);
    if (k == STG_ISTFT) a = istft_frames(r[SC_NIN], r[SC_NOUT]), c = (r[SC_NOUT] + ST_THREADS - 1) / ST_THREADS;
    if (k == STG_RS) a = (r[SC_NOUT] + ST_THREADS - 1) / ST_THREADS;
    g.a = a > g.a ? a : g.a;
    g.c = c > g.c ? c : g.c;
  }
  return g;
}

static int stage_check(StageKind k, const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                       int64_t n_files, const void* out, int64_t out_bytes, const void* ws, int64_t ws_bytes,
                       int64_t* max_blocks) {
  *max_blocks = 0;
  SAD_REQUIRE(n_files >= 0 && n_files <= 65535, "n_files must be in [0, 65535]");
  SAD_REQUIRE(in_bytes >= 0 && out_bytes >= 0 && ws_bytes >= 0, "a byte count is negative");
  if (n_files == 0) return SAD_OK;
  SAD_REQUIRE(in && out && table && d_table, "null pointer");
  SAD_REQUIRE((uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && (uintptr_t)ws % 16 == 0,
              "in, out and workspace must be 16-byte aligned");
  int64_t out_end = 0, ws_end = 0;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t* r = table + f * ST_COLS;
    SAD_REQUIRE(r[SC_NIN] >= 0 && r[SC_NIN] <= SW_MAX_FRAMES && r[SC_NOUT] >= 0 && r[SC_NOUT] <= SW_MAX_FRAMES,
                "stage table: counts must be in [0, 2^31]");
    SAD_REQUIRE(r[SC_IN] >= 0 && r[SC_IN] % 16 == 0 && r[SC_OUT] >= 0 && r[SC_OUT] % 16 == 0 && r[SC_WS] >= 0 &&
                    r[SC_WS] % 16 == 0,
                "stage table: offsets must be multiples of 16 bytes");
    SAD_REQUIRE((r[SC_FLAGS] & ~(int64_t)(k == STG_ISTFT || k == STG_RS ? SF_CLIP : 0)) == 0,
                "stage table: unknown flag");
    SAD_REQUIRE(r[SC_IN] <= in_bytes && stage_in_bytes(k, r) <= in_bytes - r[SC_IN],
                "stage table: an input lies past the end of its buffer");
    SAD_REQUIRE(r[SC_OUT] >= out_end, "stage table: the outputs must ascend without overlap");
    SAD_REQUIRE(r[SC_OUT] <= out_bytes && stage_out_bytes(k, r) <= out_bytes - r[SC_OUT],
                "stage table: an output lies past the end of its buffer");
    out_end = r[SC_OUT] + stage_out_bytes(k, r);
    if (k == STG_PV || k == STG_RS) {
      const double rate = st_f64(r[SC_RATE]);
      SAD_REQUIRE(rate >= 0.25 && rate <= 4.0, "stage table: the rate must be in [0.25, 4]");
    }
    const int64_t need = stage_ws_bytes(k, r);
    if (need > 0) {
      SAD_REQUIRE(ws, "null workspace");
      SAD_REQUIRE(r[SC_WS] >= ws_end, "stage table: the workspaces must ascend without overlap");
      SAD_REQUIRE(r[SC_WS] <= ws_bytes && need <= ws_bytes - r[SC_WS], "stage table: workspace too small");
      ws_end = r[SC_WS] + need;
    }
  }
  const StageGrid g = stage_grid(k, table, n_files);
  *max_blocks = g.a > g.c ? g.a : g.c;
  SAD_REQUIRE(*max_blocks < (1ll << 31), "a file is too long for one launch");
  return SAD_OK;
}

#define ST_LAUNCH(kernel, gx, gy)                                                                              \
  do {                                                                                                         \
    if ((gx) > 0) {                                                                                            \
      hipLaunchKernelGGL(kernel, dim3((unsigned)(gx), (unsigned)(gy)), dim3(ST_THREADS), 0, s, b, d_table);    \
      SAD_CHECK_HIP(hipGetLastError());                                                                        \
    }                                                                                                          \
  } while (0)

static int stage_launch(StageKind k, const StBases& b, const int64_t* table, const int64_t* d_table, int64_t n_files,
                        hipStream_t s) {
  const StageGrid g = stage_grid(k, table, n_files);
  switch (k) {
    case STG_STFT:
      ST_LAUNCH(stft2048_kernel, g.a, n_files);
      break;
    case STG_PV:
      ST_LAUNCH(pv_polar_kernel, g.a, n_files);
      ST_LAUNCH(pv_walk_kernel<false>, g.c, n_files);
      ST_LAUNCH(pv_combine_kernel, g.c > 0 ? (ST_BINS + ST_THREADS - 1) / ST_THREADS : 0, n_files);
      ST_LAUNCH(pv_walk_kernel<true>, g.c, n_files);
      break;
    case STG_ISTFT:
      ST_LAUNCH(istft_frames_kernel, g.a, n_files);
      ST_LAUNCH(istft_gather_kernel, g.c, n_files);
      break;
    case STG_RS:
      ST_LAUNCH(resample_ratio_kernel, g.a, n_files);
      break;
  }
  return SAD_OK;
}

static int stage_run(StageKind k, const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                     int64_t n_files, void* out, int64_t out_bytes, void* ws, int64_t ws_bytes, void* stream) {
  int64_t max_blocks;
  if (int rc = stage_check(k, in, in_bytes, table, d_table, n_files, out, out_bytes, ws, ws_bytes, &max_blocks))
    return rc;
  if (max_blocks == 0) return SAD_OK;
  const StBases b{(const unsigned char*)in, (unsigned char*)out, (unsigned char*)out, (unsigned char*)ws};
  return stage_launch(k, b, table, d_table, n_files, (hipStream_t)stream);
}

static int stage_ws_size(StageKind k, const int64_t* table, int64_t n_files, size_t* bytes) {
  SAD_REQUIRE(bytes, "null bytes");
  SAD_REQUIRE(n_files >= 0 && n_files <= 65535, "n_files must be in [0, 65535]");
  SAD_REQUIRE(table || n_files == 0, "null pointer");
  int64_t total = 0;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t* r = table + f * ST_COLS;
    SAD_REQUIRE(r[SC_NIN] >= 0 && r[SC_NIN] <= SW_MAX_FRAMES && r[SC_NOUT] >= 0 && r[SC_NOUT] <= SW_MAX_FRAMES,
                "stage table: counts must be in [0, 2^31]");
    total += stage_ws_bytes(k, r);
  }
  *bytes = (size_t)total;
  return SAD_OK;
}

// the batch entry's host tables and checks
struct SwBatch {
  std::vector<int64_t> tables;  // [SW_TABLES][n_files][ST_COLS]
  int64_t ws_bytes = 0;         // the stage tables' device copy, then the files' workspaces
  int64_t max_mono = 0;
  bool any = false, second = false, pitch = false;
};

static int sw_check(const int64_t* file_table, int64_t n_files, const int64_t* sw_table, int64_t arena_bytes,
                    int64_t mono_bytes, bool sizes_only, SwBatch& b) {
  SAD_REQUIRE(n_files >= 0 && n_files <= 65535, "n_files must be in [0, 65535]");
  SAD_REQUIRE(arena_bytes >= 0 && mono_bytes >= 0, "arena_bytes / mono_bytes < 0");
  if (n_files == 0) return SAD_OK;
  SAD_REQUIRE(file_table && sw_table, "null pointer");
  b.tables.assign((size_t)(n_files * SW_TABLES * ST_COLS), 0);
  int64_t ws_off = sw_tables_bytes(n_files), out_end = 0;
  int64_t rows[SW_TABLES * ST_COLS];
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t* t = file_table + f * SW_FT_COLS;
    const int64_t* a = sw_table + f * SW_COLS;
    const int64_t off = t[0], n_read = t[1], total = t[2], ch = t[3], enc = t[4];
    const int64_t kind = a[SW_KIND], n_out = a[SW_NOUT], out_off = a[SW_OUT];
    SAD_REQUIRE(kind >= 0 && kind <= SW_TIME_PITCH, "stretch table: kind must be in [0, 10]");
    if (kind < SW_SPEED_UP) continue;  // sad_wave_augment_run's file
    SAD_REQUIRE(ch >= 1 && ch <= 64, "file table: channels must be in [1, 64]");
    SAD_REQUIRE(enc == SAD_PCM_I16 || enc == SAD_PCM_F32, "file table: encoding must be SAD_PCM_I16 or SAD_PCM_F32");
    SAD_REQUIRE(total >= 0 && total <= SW_MAX_FRAMES && n_read >= 0 && n_read <= total,
                "file table: frames read / total frames");
    SAD_REQUIRE(off >= 0 && off % 16 == 0, "file table: a file must start at a multiple of 16 bytes");
    const int64_t bytes = n_read * ch * (enc == SAD_PCM_I16 ? 2 : 4);
    SAD_REQUIRE(sizes_only || (off <= arena_bytes && bytes <= arena_bytes - off),
                "file table: a file lies past the end of the arena");
    const bool pitch = kind >= SW_PITCH_UP, two = kind == SW_TIME_PITCH;
    double rate = 1.0, steps = 0.0, prate = 1.0;
    if (!pitch || two) {
      rate = st_f64(a[SW_RATE]);
      SAD_REQUIRE(rate >= 0.25 && rate <= 4.0, "stretch table: the rate must be in [0.25, 4]");
    }
    if (pitch) {
      steps = st_f64(a[SW_STEPS]);
      prate = st_f64(a[SW_PRATE]);
      SAD_REQUIRE(steps >= -12.0 && steps <= 12.0, "stretch table: the steps must be in [-12, 12]");
      SAD_REQUIRE(prate >= 0.25 && prate <= 4.0 && fabs(prate * exp2(steps / 12.0) - 1.0) <= 1e-9,
                  "stretch table: column 5 is the pitch rate 2^(-steps / 12)");
    }
    const int64_t len_out = pitch && !two ? total : (int64_t)rint((double)total / rate);
    SAD_REQUIRE(n_out >= 0 && n_out <= len_out, "stretch table: frames out must be in [0, the stretched length]");
    SAD_REQUIRE(out_off >= 0 && out_off % 16 == 0, "stretch table: a file's output must start at a multiple of 16 bytes");
    SAD_REQUIRE(out_off >= out_end, "stretch table: the files' outputs must ascend without overlap");
    SAD_REQUIRE(sizes_only || (out_off <= mono_bytes && n_out * 4 <= mono_bytes - out_off),
                "stretch table: the output arena is too small");
    out_end = out_off + n_out * 4;
    ws_off += sw_plan(kind, total, n_read, rate, prate, n_out, out_off, ws_off, rows);
    for (int s = 0; s < SW_TABLES; ++s)
      memcpy(&b.tables[(size_t)((s * n_files + f) * ST_COLS)], rows + s * ST_COLS, ST_COLS * 8);
    b.any = true;
    b.second |= two;
    b.pitch |= pitch;
    b.max_mono = rows[SC_NIN] > b.max_mono ? rows[SC_NIN] : b.max_mono;
  }
  b.ws_bytes = ws_off;
  return SAD_OK;
}

}  // namespace sad

using namespace sad;

extern "C" int sad_wave_stretch_geometry(int32_t* n_fft, int32_t* hop, int32_t* chunk, int32_t* max_launches) {
  SAD_REQUIRE(n_fft && hop && chunk && max_launches, "null pointer");
  *n_fft = ST_N;
  *hop = ST_HOP;
  *chunk = PV_CHUNK;
  *max_launches = 17;
  return SAD_OK;
}

extern "C" int sad_phase_vocoder_workspace_size(const int64_t* table, int64_t n_files, size_t* bytes) {
  return stage_ws_size(STG_PV, table, n_files, bytes);
}
extern "C" int sad_istft2048_workspace_size(const int64_t* table, int64_t n_files, size_t* bytes) {
  return stage_ws_size(STG_ISTFT, table, n_files, bytes);
}

extern "C" int sad_stft2048_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                                int64_t n_files, void* out, int64_t out_bytes, void* stream) {
  return stage_run(STG_STFT, in, in_bytes, table, d_table, n_files, out, out_bytes, nullptr, 0, stream);
}
extern "C" int sad_phase_vocoder_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                                     int64_t n_files, void* out, int64_t out_bytes, void* ws, size_t ws_bytes,
                                     void* stream) {
  return stage_run(STG_PV, in, in_bytes, table, d_table, n_files, out, out_bytes, ws, (int64_t)ws_bytes, stream);
}
extern "C" int sad_istft2048_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                                 int64_t n_files, void* out, int64_t out_bytes, void* ws, size_t ws_bytes,
                                 void* stream) {
  return stage_run(STG_ISTFT, in, in_bytes, table, d_table, n_files, out, out_bytes, ws, (int64_t)ws_bytes, stream);
}
extern "C" int sad_resample_ratio_run(const void* in, int64_t in_bytes, const int64_t* table, const int64_t* d_table,
                                      int64_t n_files, void* out, int64_t out_bytes, void* stream) {
  return stage_run(STG_RS, in, in_bytes, table, d_table, n_files, out, out_bytes, nullptr, 0, stream);
}

extern "C" int sad_wave_stretch_workspace_size(const int64_t* file_table, const int64_t* stretch_table,
                                               int64_t n_files, size_t* bytes) {
  SAD_REQUIRE(bytes, "null bytes");
  SwBatch b;
  if (int rc = sw_check(file_table, n_files, stretch_table, 0, 0, true, b)) return rc;
  *bytes = (size_t)b.ws_bytes;
  return SAD_OK;
}

extern "C" int sad_wave_stretch_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                                    const int64_t* d_file_table, int64_t n_files, const int64_t* stretch_table,
                                    const int64_t* d_stretch_table, void* mono_out, int64_t mono_bytes, void* ws,
                                    size_t ws_bytes, void* stream) {
  SwBatch b;
  if (int rc = sw_check(file_table, n_files, stretch_table, arena_bytes, mono_bytes, false, b)) return rc;
  if (!b.any) return SAD_OK;
  SAD_REQUIRE(arena && d_file_table && d_stretch_table && mono_out, "null pointer");
  SAD_REQUIRE(ws_bytes >= (size_t)b.ws_bytes, "workspace too small (sad_wave_stretch_workspace_size)");
  SAD_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int64_t* d_tables = (int64_t*)ws;
  hipLaunchKernelGGL(stretch_plan_kernel, dim3(1), dim3(64), 0, s, d_file_table,
                     d_stretch_table, (int)n_files, d_tables);
  SAD_CHECK_HIP(hipGetLastError());
  if (b.max_mono > 0) {
    hipLaunchKernelGGL(stretch_mono_kernel, dim3((unsigned)((b.max_mono + ST_THREADS - 1) / ST_THREADS), (unsigned)n_files),
                       dim3(ST_THREADS), 0, s, (const unsigned char*)arena, d_file_table, d_tables,
                       (unsigned char*)ws);
    SAD_CHECK_HIP(hipGetLastError());
  }
  const StBases bases{(const unsigned char*)ws, (unsigned char*)ws, (unsigned char*)mono_out, (unsigned char*)ws};
  static const StageKind kinds[SW_TABLES] = {STG_STFT, STG_PV, STG_ISTFT, STG_STFT, STG_PV, STG_ISTFT, STG_RS};
  for (int t = 0; t < SW_TABLES; ++t) {
    if ((t >= 3 && t < 6 && !b.second) || (t == 6 && !b.pitch)) continue;
    const int64_t* host = b.tables.data() + (size_t)t * n_files * ST_COLS;
    if (int rc = stage_launch(kinds[t], bases, host, d_tables + (int64_t)t * n_files * ST_COLS, n_files, s)) return rc;
  }
  return SAD_OK;
}
