// waveaug.hip -- waveform augmentation of a training batch on the device
// (submodel_trainer.py --wave-augment): six of the eleven kinds of the
// reference's audio_augmneter.py (:79-137, clip :190), applied to the stored
// samples that --device-ingest already holds in one byte arena, before
// sad_train_ingest_run resamples and cuts them.  tests/waveaug_ref.py states
// the contract in float64; include/sad.h ("waveform augmentation") the tables.
//
//   interleaved PCM of file f  -> mono (ti_mono, ingest.hpp)
//                              -> its kind (one per file)  -> clip(-1, 1)
//                              -> fp32 mono arena, the first n_out frames
//
// A workgroup is one wave and owns one chunk of WA_CHUNK = 64 x WA_SUB frames of
// one file: grid (most chunks of any file, files), blocks past a file's end
// leave at once.  Five kinds are pointwise.  The phaser is three cascaded
// biquads, each modulated by an LFO and added back, so stage k + 1 filters
// stage k's output: per stage a chunked scan of the filter's two-element state
// (transposed direct form II; with no input the state moves by the constant
// A = [[-a1, 1], [-a2, 0]]):
//   A  lane t walks its WA_SUB frames from a zero state -> end state e_t; a
//      wave scan with A^WA_SUB gives the chunk's zero-state end state E_c
//   B  one thread per file: S_c = A^WA_CHUNK S_{c-1} + E_{c-1}, S_0 = 0
//   C  v_0 = e_0 + A^WA_SUB S_c, the same wave scan gives every lane's true
//      start state; the lanes walk again, y_p <- y_p + lfo y_f
// C of stage k and A of stage k + 1 share a launch (the chunk is in LDS), which
// makes seven launches for any batch: A1 | B1 | C1 A2 + the pointwise kinds |
// B2 | C2 A3 | B3 | C3.  The noise's RMS rides along: per-chunk sums of squares
// in the first launch, summed per file in a fixed order in the third.  The
// walks are fp32 FMAs; the states between walks, the scans, the filter
// coefficients and the LFO phases are float64 (a few operations per chunk or
// per frame), so the seams add no rounding of their own.  Global access is
// coalesced; the serial walks read LDS with a stride of WA_SUB + 1 words.
// Nothing depends on which other files share the launch.
#include <math.h>

#include "common.hpp"
#include "ingest.hpp"

namespace sad {

constexpr int WA_SUB = 32;                 // frames a lane walks serially
constexpr int WA_CHUNK = 64 * WA_SUB;      // frames per workgroup (one wave): the scan's chunk
constexpr int WA_PITCH = WA_SUB + 1;       // LDS words between two lanes' runs
constexpr int WA_FT_COLS = 6;              // sad_train_ingest_run's file table
constexpr int WA_COLS = 8;                 // augmentation table columns
constexpr int WA_KINDS = 6;
enum { WA_ORIGINAL = 0, WA_DRC = 1, WA_NOISE = 2, WA_TREMOLO = 3, WA_PHASER = 4, WA_SHIFT = 5 };
constexpr int64_t WA_PHASER_MIN_SR = 5000;  // sin(w) / 2 <= 0 at and below: the pole leaves the unit circle
constexpr int64_t WA_WS_PER_CHUNK = 16 + 16 + 64 * 8 + 8;  // E, S (double2), e (64 float2), P (double)

struct WaWs {
  double* E;  // [chunks][2] zero-state end state of the chunk
  double* S;  // [chunks][2] true start state of the chunk
  float* e;   // [chunks][64][2] zero-state end state of each lane's run
  double* P;  // [chunks] sum of squares (noise)
};

struct M2 {
  double a, b, c, d;
};
__device__ __forceinline__ M2 m2_mul(const M2& x, const M2& y) {
  return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}
__device__ __forceinline__ M2 m2_pow2(M2 m, int log2n) {
  for (int i = 0; i < log2n; ++i) m = m2_mul(m, m);
  return m;
}

// the stage's biquad b = [al, 0, -al], a = [1 + al, -2 cos w, 1 - al], normalised by a[0]
__device__ __forceinline__ void wa_biquad(int stage, double sr, double& b0, double& a1, double& a2) {
  const double f0 = stage == 0 ? 500.0 : stage == 1 ? 1500.0 : 2500.0;
  const double w = 2.0 * M_PI * f0 / sr;
  const double al = sin(w) / 2.0, a0 = 1.0 + al;
  b0 = al / a0;
  a1 = -2.0 * cos(w) / a0;
  a2 = (1.0 - al) / a0;
}

// inclusive scan of two-element states over the wave's lanes with the
// transition m per lane: v_t <- sum_{j <= t} m^(t - j) v_j
__device__ __forceinline__ void wa_scan(double& v0, double& v1, M2 m, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double u0 = __shfl_up(v0, d, 64), u1 = __shfl_up(v1, d, 64);
    if (lane >= d) {
      v0 += m.a * u0 + m.b * u1;
      v1 += m.c * u0 + m.d * u1;
    }
    m = m2_mul(m, m);
  }
}

// sin(2 pi t) of a phase in turns: reduced in float64, rounded once to fp32
__device__ __forceinline__ float wa_sin_turns(double t) { return sinpif(2.0f * (float)(t - rint(t))); }

// n_i of (key, i): the dropout hash of headtrain.hip, two uniforms, Box-Muller
__device__ __forceinline__ float wa_normal(uint64_t key, int64_t i) {
  uint64_t z = key + 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const float u1 = ((float)(uint32_t)(z >> 40) + 1.0f) * (1.0f / 16777216.0f);
  const float u2 = (float)(uint32_t)((z >> 16) & 0xFFFFFFu) * (1.0f / 16777216.0f);
  return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

__device__ __forceinline__ float wa_clip(float v) { return fminf(fmaxf(v, -1.0f), 1.0f); }

template <typename IT>
__device__ __forceinline__ void wa_chunk(float* __restrict__ xs, int stage, const IT* __restrict__ x, int64_t n_read,
                                         int64_t total, int channels, const int64_t* __restrict__ ag,
                                         float* __restrict__ out, const WaWs& ws) {
  const int lane = threadIdx.x;
  const int kind = (int)ag[0];
  const double sr = (double)ag[1];
  const int64_t n_out = ag[2];
  const float p0 = __uint_as_float((uint32_t)ag[4]), p1 = __uint_as_float((uint32_t)((uint64_t)ag[4] >> 32));
  const uint64_t key = (uint64_t)ag[5];
  const int64_t chunk = ag[6] + blockIdx.x;  // index into the workspace
  const int64_t c0 = (int64_t)blockIdx.x * WA_CHUNK;
  const float fc = (float)channels;

  if (kind == WA_NOISE && stage == 0) {  // sum of squares of the chunk: lanes in order, then a fixed tree
    float acc = 0.f;
    for (int j = 0; j < WA_SUB; ++j) {
      const float v = ti_mono(x, c0 + j * 64 + lane, n_read < n_out ? n_read : n_out, channels, fc);
      acc = fmaf(v, v, acc);
    }
    double s = (double)acc;
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) ws.P[chunk] = s;
    return;
  }
  if (kind != WA_PHASER) {
    if (stage != 1) return;
    float amp = 0.f;
    if (kind == WA_NOISE) {  // the file's chunks in a fixed order: a function of the file alone
      const int64_t nch = (n_out + WA_CHUNK - 1) / WA_CHUNK;
      double s = 0.0;
      for (int64_t c = lane; c < nch; c += 64) s += ws.P[ag[6] + c];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      amp = p0 * (float)sqrt(s / (double)n_out);
    }
    const int64_t s_shift = (int64_t)p0;
    const double step = total > 1 ? ((double)total / sr) / (double)(total - 1) : 0.0;
    for (int j = 0; j < WA_SUB; ++j) {
      const int64_t i = c0 + j * 64 + lane;
      if (i >= n_out) break;
      float v;
      if (kind == WA_SHIFT) {
        const int64_t src = i - s_shift;
        v = (s_shift != 0 && src < total) ? ti_mono(x, src, n_read, channels, fc) : 0.f;
      } else {
        const float y = ti_mono(x, i, n_read, channels, fc);
        if (kind == WA_DRC) {
          const float r = powf(fabsf(y), p0);
          v = y > 0.f ? r : (y < 0.f ? -r : 0.f);
        } else if (kind == WA_NOISE) {
          v = fmaf(amp, wa_normal(key, i), y);
        } else if (kind == WA_TREMOLO) {
          const double t = i == total - 1 ? (total > 1 ? (double)total / sr : 0.0) : (double)i * step;
          v = y * fmaf(p1, wa_sin_turns((double)p0 * t), 1.0f - p1);
        } else {
          v = y;
        }
      }
      out[i] = wa_clip(v);
    }
    return;
  }

  // ---- phaser: stage 0 = A1, 1 = C1 A2, 2 = C2 A3, 3 = C3
  for (int e = lane; e < WA_CHUNK; e += 64) {
    const int64_t i = c0 + e;
    float v = 0.f;
    if (i < n_out) v = stage <= 1 ? ti_mono(x, i, n_read, channels, fc) : out[i];
    xs[(e / WA_SUB) * WA_PITCH + (e % WA_SUB)] = v;
  }
  __syncthreads();
  float* run = xs + lane * WA_PITCH;
  if (stage >= 1) {
    double b0d, a1d, a2d;
    wa_biquad(stage - 1, sr, b0d, a1d, a2d);
    const M2 ps = m2_pow2({-a1d, 1.0, -a2d, 0.0}, 5);  // A^WA_SUB
    static_assert(WA_SUB == 32, "A^WA_SUB is five squarings");
    const float2 el = ((const float2*)ws.e)[chunk * 64 + lane];
    double v0 = (double)el.x, v1 = (double)el.y;
    const double s0 = ws.S[2 * chunk], s1 = ws.S[2 * chunk + 1];
    if (lane == 0) {
      v0 += ps.a * s0 + ps.b * s1;
      v1 += ps.c * s0 + ps.d * s1;
    }
    wa_scan(v0, v1, ps, lane);
    const double t0 = __shfl_up(v0, 1, 64), t1 = __shfl_up(v1, 1, 64);
    float z1 = (float)(lane ? t0 : s0), z2 = (float)(lane ? t1 : s1);
    const float b0 = (float)b0d, na1 = (float)-a1d, na2 = (float)-a2d, nb0 = -b0;
    const double dt = (double)p0 / sr;  // LFO turns per frame
    double t = (double)p0 * (double)(c0 + lane * WA_SUB) / sr;
    t -= rint(t);
#pragma unroll 4
    for (int j = 0; j < WA_SUB; ++j) {
      const float xv = run[j];
      const float y = fmaf(b0, xv, z1);
      z1 = fmaf(na1, y, z2);
      z2 = fmaf(na2, y, nb0 * xv);
      run[j] = fmaf(p1 * wa_sin_turns(t), y, xv);
      t += dt;
    }
  }
  if (stage <= 2) {
    double b0d, a1d, a2d;
    wa_biquad(stage, sr, b0d, a1d, a2d);
    const float b0 = (float)b0d, na1 = (float)-a1d, na2 = (float)-a2d, nb0 = -b0;
    float z1 = 0.f, z2 = 0.f;
#pragma unroll 4
    for (int j = 0; j < WA_SUB; ++j) {
      const float xv = run[j];
      const float y = fmaf(b0, xv, z1);
      z1 = fmaf(na1, y, z2);
      z2 = fmaf(na2, y, nb0 * xv);
    }
    ((float2*)ws.e)[chunk * 64 + lane] = make_float2(z1, z2);
    double v0 = (double)z1, v1 = (double)z2;
    wa_scan(v0, v1, m2_pow2({-a1d, 1.0, -a2d, 0.0}, 5), lane);
    if (lane == 63) {
      ws.E[2 * chunk] = v0;
      ws.E[2 * chunk + 1] = v1;
    }
  }
  if (stage >= 1) {
    __syncthreads();
    for (int e = lane; e < WA_CHUNK; e += 64) {
      const int64_t i = c0 + e;
      if (i >= n_out) break;
      const float v = xs[(e / WA_SUB) * WA_PITCH + (e % WA_SUB)];
      out[i] = stage == 3 ? wa_clip(v) : v;
    }
  }
}

__global__ __launch_bounds__(64) void wave_augment_kernel(int stage, const unsigned char* __restrict__ arena,
                                                          const int64_t* __restrict__ file_table,
                                                          const int64_t* __restrict__ aug_table,
                                                          unsigned char* __restrict__ mono, WaWs ws) {
  __shared__ float xs[64 * WA_PITCH];
  const int64_t* ft = file_table + (int64_t)blockIdx.y * WA_FT_COLS;
  const int64_t* ag = aug_table + (int64_t)blockIdx.y * WA_COLS;
  if ((int64_t)blockIdx.x * WA_CHUNK >= ag[2]) return;  // block-uniform
  float* out = (float*)(mono + ag[3]);
  if ((int)ft[4] == SAD_PCM_I16)
    wa_chunk<int16_t>(xs, stage, (const int16_t*)(arena + ft[0]), ft[1], ft[2], (int)ft[3], ag, out, ws);
  else
    wa_chunk<float>(xs, stage, (const float*)(arena + ft[0]), ft[1], ft[2], (int)ft[3], ag, out, ws);
}

// B: the chunks' true start states of every phaser file, one thread per file
__global__ __launch_bounds__(64) void wave_augment_combine_kernel(int stage, const int64_t* __restrict__ aug_table,
                                                                  int n_files, WaWs ws) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_files) return;
  const int64_t* ag = aug_table + (int64_t)f * WA_COLS;
  if ((int)ag[0] != WA_PHASER) return;
  double b0, a1, a2;
  wa_biquad(stage, (double)ag[1], b0, a1, a2);
  const M2 pc = m2_pow2({-a1, 1.0, -a2, 0.0}, 11);  // A^WA_CHUNK
  static_assert(WA_CHUNK == 2048, "A^WA_CHUNK is eleven squarings");
  const int64_t nch = (ag[2] + WA_CHUNK - 1) / WA_CHUNK, base = ag[6];
  double s0 = 0.0, s1 = 0.0;
  for (int64_t c = 0; c < nch; ++c) {
    ws.S[2 * (base + c)] = s0;
    ws.S[2 * (base + c) + 1] = s1;
    const double e0 = ws.E[2 * (base + c)], e1 = ws.E[2 * (base + c) + 1];
    const double n0 = pc.a * s0 + pc.b * s1 + e0;
    s1 = pc.c * s0 + pc.d * s1 + e1;
    s0 = n0;
  }
}

// The phaser as one thread per file, the three stages in one serial pass over
// the file: the yardstick tools/bench_wave_augment.py times the scan against.
// Same arithmetic per frame as wa_chunk's walks (fp32 FMAs, float64 phase).
template <typename IT>
__device__ __forceinline__ void wa_serial(const IT* __restrict__ x, int64_t n_read, int channels,
                                          const int64_t* __restrict__ ag, float* __restrict__ out) {
  const double sr = (double)ag[1];
  const int64_t n_out = ag[2];
  const float p1 = __uint_as_float((uint32_t)((uint64_t)ag[4] >> 32));
  const double dt = (double)__uint_as_float((uint32_t)ag[4]) / sr;
  float b0[3], na1[3], na2[3], z1[3] = {0.f, 0.f, 0.f}, z2[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < 3; ++k) {
    double b, a1, a2;
    wa_biquad(k, sr, b, a1, a2);
    b0[k] = (float)b;
    na1[k] = (float)-a1;
    na2[k] = (float)-a2;
  }
  for (int64_t i = 0; i < n_out; ++i) {
    float v = ti_mono(x, i, n_read, channels, (float)channels);
    const float lfo = p1 * wa_sin_turns((double)i * dt);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float y = fmaf(b0[k], v, z1[k]);
      z1[k] = fmaf(na1[k], y, z2[k]);
      z2[k] = fmaf(na2[k], y, -b0[k] * v);
      v = fmaf(lfo, y, v);
    }
    out[i] = wa_clip(v);
  }
}

__global__ __launch_bounds__(64) void wave_phaser_serial_kernel(const unsigned char* __restrict__ arena,
                                                                const int64_t* __restrict__ file_table,
                                                                const int64_t* __restrict__ aug_table, int n_files,
                                                                unsigned char* __restrict__ mono) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_files) return;
  const int64_t* ft = file_table + (int64_t)f * WA_FT_COLS;
  const int64_t* ag = aug_table + (int64_t)f * WA_COLS;
  if ((int)ag[0] != WA_PHASER) return;
  float* out = (float*)(mono + ag[3]);
  if ((int)ft[4] == SAD_PCM_I16)
    wa_serial<int16_t>((const int16_t*)(arena + ft[0]), ft[1], (int)ft[3], ag, out);
  else
    wa_serial<float>((const float*)(arena + ft[0]), ft[1], (int)ft[3], ag, out);
}

static int64_t wa_chunks(int64_t n_out) { return (n_out + WA_CHUNK - 1) / WA_CHUNK; }

}  // namespace sad

using namespace sad;

extern "C" int sad_wave_augment_geometry(int32_t* chunk, int32_t* sub) {
  SAD_REQUIRE(chunk && sub, "null pointer");
  *chunk = WA_CHUNK;
  *sub = WA_SUB;
  return SAD_OK;
}

extern "C" int sad_wave_augment_workspace_size(const int64_t* aug_table, int64_t n_files, size_t* bytes) {
  SAD_REQUIRE(bytes, "null bytes");
  SAD_REQUIRE(n_files >= 0 && n_files <= 65535, "n_files must be in [0, 65535]");
  SAD_REQUIRE(aug_table || n_files == 0, "null pointer");
  int64_t chunks = 0;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t n_out = aug_table[f * WA_COLS + 2];
    SAD_REQUIRE(n_out >= 0 && n_out <= (1ll << 40), "augmentation table: frames out must be in [0, 2^40]");
    chunks += wa_chunks(n_out);
  }
  *bytes = (size_t)(chunks * WA_WS_PER_CHUNK);
  return SAD_OK;
}

// the host tables' checks, shared by the two entries
struct WaBatch {
  int64_t chunks = 0, max_chunks = 0;
  bool phaser = false, noise = false;
};

static int wa_check(const void* arena, int64_t arena_bytes, const int64_t* file_table, const int64_t* d_file_table,
                    int64_t n_files, const int64_t* aug_table, const int64_t* d_aug_table, const void* mono_out,
                    int64_t mono_bytes, WaBatch& b) {
  SAD_REQUIRE(n_files >= 0 && n_files <= 65535, "n_files must be in [0, 65535]");
  SAD_REQUIRE(arena_bytes >= 0 && mono_bytes >= 0, "arena_bytes / mono_bytes < 0");
  if (n_files == 0) return SAD_OK;
  SAD_REQUIRE(arena && file_table && d_file_table && aug_table && d_aug_table && mono_out, "null pointer");
  int64_t chunks = 0, max_chunks = 0, out_end = 0;
  bool phaser = false, noise = false;
  for (int64_t f = 0; f < n_files; ++f) {
    const int64_t* t = file_table + f * WA_FT_COLS;
    const int64_t* a = aug_table + f * WA_COLS;
    const int64_t off = t[0], n_read = t[1], total = t[2], ch = t[3], enc = t[4];
    const int64_t kind = a[0], sr = a[1], n_out = a[2], out_off = a[3];
    SAD_REQUIRE(ch >= 1 && ch <= 64, "file table: channels must be in [1, 64]");
    SAD_REQUIRE(enc == SAD_PCM_I16 || enc == SAD_PCM_F32, "file table: encoding must be SAD_PCM_I16 or SAD_PCM_F32");
    SAD_REQUIRE(total >= 0 && total <= (1ll << 40) && n_read >= 0 && n_read <= total,
                "file table: frames read / total frames");
    SAD_REQUIRE(off >= 0 && off % 16 == 0, "file table: a file must start at a multiple of 16 bytes");
    const int64_t bytes = n_read * ch * (enc == SAD_PCM_I16 ? 2 : 4);
    SAD_REQUIRE(off <= arena_bytes && bytes <= arena_bytes - off, "file table: a file lies past the end of the arena");
    SAD_REQUIRE(kind >= 0 && kind < WA_KINDS, "augmentation table: kind must be in [0, 5]");
    SAD_REQUIRE(sr > 0 && sr <= (1 << 24), "augmentation table: sample rate must be in [1, 2^24]");
    SAD_REQUIRE(kind != WA_PHASER || sr > WA_PHASER_MIN_SR,
                "augmentation table: the phaser needs a sample rate above 5000 Hz");
    SAD_REQUIRE(n_out >= 0 && n_out <= total, "augmentation table: frames out must be in [0, total frames]");
    SAD_REQUIRE(out_off >= 0 && out_off % 16 == 0,
                "augmentation table: a file's output must start at a multiple of 16 bytes");
    SAD_REQUIRE(out_off >= out_end, "augmentation table: the files' outputs must ascend without overlap");
    SAD_REQUIRE(out_off <= mono_bytes && n_out * 4 <= mono_bytes - out_off,
                "augmentation table: the output arena is too small");
    out_end = out_off + n_out * 4;
    float p0, p1;
    const uint32_t lo = (uint32_t)a[4], hi = (uint32_t)((uint64_t)a[4] >> 32);
    memcpy(&p0, &lo, 4);
    memcpy(&p1, &hi, 4);
    SAD_REQUIRE(p0 == p0 && p1 == p1 && fabsf(p0) <= 16777216.f && fabsf(p1) <= 16777216.f,
                "augmentation table: parameters must be finite");
    SAD_REQUIRE(kind != WA_DRC || p0 > 0.f, "augmentation table: the compression exponent must be positive");
    SAD_REQUIRE(kind != WA_SHIFT || p0 == (float)(int64_t)p0, "augmentation table: the shift is a whole number of frames");
    SAD_REQUIRE(a[6] == chunks, "augmentation table: column 6 is the sum of the earlier files' chunk counts");
    const int64_t fc = wa_chunks(n_out);
    chunks += fc;
    max_chunks = fc > max_chunks ? fc : max_chunks;
    phaser |= kind == WA_PHASER;
    noise |= kind == WA_NOISE;
  }
  SAD_REQUIRE(max_chunks < (1ll << 31), "a file is too long for one launch");
  b.chunks = chunks;
  b.max_chunks = max_chunks;
  b.phaser = phaser;
  b.noise = noise;
  return SAD_OK;
}

extern "C" int sad_wave_augment_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                                    const int64_t* d_file_table, int64_t n_files, const int64_t* aug_table,
                                    const int64_t* d_aug_table, void* mono_out, int64_t mono_bytes, void* ws,
                                    size_t ws_bytes, void* stream) {
  WaBatch b;
  if (int rc = wa_check(arena, arena_bytes, file_table, d_file_table, n_files, aug_table, d_aug_table, mono_out,
                        mono_bytes, b))
    return rc;
  const int64_t chunks = b.chunks, max_chunks = b.max_chunks;
  const bool phaser = b.phaser, noise = b.noise;
  SAD_REQUIRE(ws_bytes >= (size_t)(chunks * WA_WS_PER_CHUNK), "workspace too small (sad_wave_augment_workspace_size)");
  if (max_chunks == 0) return SAD_OK;
  SAD_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "workspace must be 16-byte aligned");
  WaWs w;
  w.E = (double*)ws;
  w.S = w.E + 2 * chunks;
  w.P = w.S + 2 * chunks;
  w.e = (float*)(w.P + chunks);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)max_chunks, (unsigned)n_files);
  // A1 | B1 | C1 A2 + pointwise | B2 | C2 A3 | B3 | C3; without a phaser file only
  // the pointwise launch (and the noise's sums before it) has work
  for (int stage = 0; stage <= 3; ++stage) {
    if (stage == 0 ? (phaser || noise) : (stage == 1 || phaser)) {
      hipLaunchKernelGGL(wave_augment_kernel, grid, dim3(64), 0, s, stage, (const unsigned char*)arena, d_file_table,
                         d_aug_table, (unsigned char*)mono_out, w);
      SAD_CHECK_HIP(hipGetLastError());
    }
    if (stage <= 2 && phaser) {
      hipLaunchKernelGGL(wave_augment_combine_kernel, dim3((unsigned)((n_files + 63) / 64)), dim3(64), 0, s, stage,
                         d_aug_table, (int)n_files, w);
      SAD_CHECK_HIP(hipGetLastError());
    }
  }
  return SAD_OK;
}

extern "C" int sad_wave_phaser_serial_run(const void* arena, int64_t arena_bytes, const int64_t* file_table,
                                          const int64_t* d_file_table, int64_t n_files, const int64_t* aug_table,
                                          const int64_t* d_aug_table, void* mono_out, int64_t mono_bytes,
                                          void* stream) {
  WaBatch b;
  if (int rc = wa_check(arena, arena_bytes, file_table, d_file_table, n_files, aug_table, d_aug_table, mono_out,
                        mono_bytes, b))
    return rc;
  if (!b.phaser) return SAD_OK;
  hipLaunchKernelGGL(wave_phaser_serial_kernel, dim3((unsigned)((n_files + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, (const unsigned char*)arena, d_file_table, d_aug_table, (int)n_files,
                     (unsigned char*)mono_out);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}
