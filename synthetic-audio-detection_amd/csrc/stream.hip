// stream.hip -- stateful ingestion for live feeds (include/sad.h "streaming")
//
// ingest.hip turns a finished recording into mono 32 kHz fp32; here the same
// samples are formed chunk by chunk, for many feeds in one launch, while the
// recordings are still arriving.  A stream bank of S slots lives on the device
// (caller-owned memory, sized by sad_stream_bank_size):
//
//   ring   [S][2 CAP] fp32: the slot's recent 32 kHz samples, addressed by
//          GLOBAL sample index g.  Sample g is stored at g mod CAP and at
//          CAP + g mod CAP (a mirrored ring), so any run of up to CAP
//          consecutive samples is contiguous in memory from g mod CAP on, and
//          sad_scan_select_run / sad_frontend_run_windows read windows in
//          place from the bank's one arena.  Nothing is ever slid to the
//          front: source and destination would overlap inside one launch.
//   carry  [S][2][SB_CARRY] fp32: the resampler's state, the mono-mixed INPUT
//          samples from frame J orig - width on (fewer than K of them), where J
//          is the first polyphase frame whose taps are not all present yet.
//          They are stored as the mix's fp32 values, so a tap reads the same
//          bits whichever push delivered its sample.  Two buffers, chosen by
//          the slot's push parity: within one launch some workgroups of a slot
//          still read the old carry while another writes the new one.
//
// The emission rule.  After F frames of a feed (rates reduced to orig -> new,
// width and K as in the resample plan) the outputs whose taps are all present
// are those of frames j < J(F) = (F - width) / orig (0 for F < width), so a
// push that takes the feed from F0 to F1 frames forms outputs
// [J(F0) new, J(F1) new) with resample_kernel's sum (ascending k, one fmaf per
// tap); at the feed's own rate it forms [F0, F1).  A final push forms the rest
// up to n_out = ceil(new F1 / orig) with the missing inputs as zeros, then
// zeros up to one window (preprocess_waveform's pad).  A feed opened at
// start_frame S0 = J0 orig has silence before S0 and emits nothing below
// g0 = J0 new.  The host is the authority on every counter (the table below);
// the device mutates only the ring and the carry.
//
// Workgroups are (row, tile) pairs from a host-built table, as in
// train_ingest_kernel, with its three block-uniform forms and its tap order.
// An input sample is read through one accessor (SbIn): silence before the
// feed's start, the carry, the chunk, silence after the end.
#include <math.h>

#include <vector>

#include "common.hpp"
#include "ingest.hpp"

namespace sad {

constexpr int SB_COLS = 10;       // push table columns (include/sad.h "streaming")
constexpr int SB_CARRY = 8192;    // floats per carry buffer: K <= SB_CARRY
constexpr int SB_MIN_ROOM = 4096; // CAP - window is at least this
static const int64_t SB_MAX_FRAMES = 1ll << 40;

// What one table row does, from the host's counters alone.  Host and device
// use the same function.
struct SbRow {
  int64_t mA;   // first 32 kHz sample this push stores (global index)
  int64_t mE;   // one past the last sample it stores
  int64_t mV;   // samples at or past mV are zeros (the pad)
  int64_t cb0;  // absolute input frame of the old carry's element 0
  int64_t cb1;  // ... of the new carry's
};

__host__ __device__ inline int64_t sb_max(int64_t a, int64_t b) { return a > b ? a : b; }

__host__ __device__ inline SbRow sb_row(bool native, int orig, int nw, int width, int64_t start, int64_t fb,
                                        int64_t n, bool fin, int64_t window) {
  SbRow r;
  const int64_t F1 = fb + n;
  if (native) {
    r.mA = fb;
    r.mV = F1;
    r.mE = fin ? sb_max(F1, start + window) : F1;
    r.cb0 = r.cb1 = 0;
    return r;
  }
  const int64_t J0 = start / orig;
  const int64_t ja = fb >= width ? (fb - width) / orig : 0, jb = F1 >= width ? (F1 - width) / orig : 0;
  const int64_t Ja = sb_max(ja, J0), Jb = sb_max(jb, J0);
  r.mA = Ja * nw;
  if (fin) {
    r.mV = (nw * F1 + orig - 1) / orig;
    r.mE = sb_max(r.mV, J0 * nw + window);
  } else {
    r.mV = r.mE = Jb * nw;
  }
  r.cb0 = sb_max(Ja * orig - width, start);
  r.cb1 = sb_max(Jb * orig - width, start);
  return r;
}

// tiles that form outputs (the carry tiles follow them)
__host__ __device__ inline int64_t sb_out_tiles(bool native, int nw, const SbRow& r) {
  const int64_t A = r.mE - r.mA;
  if (native || nw < 64) return (A + TI_TILE - 1) / TI_TILE;
  const int64_t frames = (A + nw - 1) / nw;
  return (frames + RS_WAVES * RS_R - 1) / (RS_WAVES * RS_R) * ((nw + 63) / 64);
}

// tiles that write the new carry: none at the feed's own rate or at its end
__host__ __device__ inline int64_t sb_carry_tiles(bool native, int K, bool fin) {
  return (native || fin) ? 0 : (K + TI_TILE - 1) / TI_TILE;
}

struct StreamRates {
  const float* kt[TI_MAX_RATES];  // nullptr: the target rate itself
  int orig[TI_MAX_RATES], nw[TI_MAX_RATES], width[TI_MAX_RATES], K[TI_MAX_RATES];
};

// one input sample by absolute frame index
template <typename IT>
struct SbIn {
  const IT* x;         // the chunk: frames [fb, fb + n)
  const float* carry;  // the old carry: frames [cb0, fb)
  int64_t start, fb, n, cb0;
  int channels;
  float fc;
  __device__ __forceinline__ float operator()(int64_t i) const {
    if (i < start) return 0.f;
    if (i < fb) {
      const int64_t c = i - cb0;
      return (c >= 0 && c < SB_CARRY) ? carry[c] : 0.f;
    }
    return ti_mono(x, i - fb, n, channels, fc);
  }
};

template <typename IT>
__device__ __forceinline__ void sb_tile(float* __restrict__ xs, const SbIn<IT>& in, const SbRow& R,
                                        const float* __restrict__ kt, int orig, int nw, int width, int K,
                                        int64_t tile, bool fin, float* __restrict__ ring, int64_t cap,
                                        float* __restrict__ carry_new) {
  auto store = [&](int64_t m, float v) {
    if (m >= R.mA && m < R.mE) {
      v = m < R.mV ? v : 0.f;
      const int64_t o = m % cap;
      ring[o] = v;
      ring[cap + o] = v;
    }
  };
  const int64_t out_tiles = sb_out_tiles(!kt, nw, R);
  if (tile >= out_tiles) {  // a carry tile: the inputs the next push's taps reach back to
    const int64_t c = tile - out_tiles;
    const int64_t len = in.fb + in.n - R.cb1;  // < K
    if (!kt || fin) return;
#pragma unroll
    for (int q = 0; q < TI_TILE / 256; ++q) {
      const int64_t e = c * TI_TILE + q * 256 + threadIdx.x;
      if (e < len && e < SB_CARRY) carry_new[e] = in(R.cb1 + e);
    }
    return;
  }
  if (!kt) {  // native rate
    const int64_t m0 = R.mA + tile * TI_TILE;
#pragma unroll
    for (int q = 0; q < TI_TILE / 256; ++q) {
      const int64_t m = m0 + q * 256 + threadIdx.x;
      if (m < R.mE) store(m, m < R.mV ? in(m) : 0.f);
    }
    return;
  }
  if (nw < 64) {  // per-output form
    const int64_t m0 = R.mA + tile * TI_TILE;
    const int64_t j0 = m0 / nw;
    const int64_t span0 = j0 * orig - width;  // input frame of xs[0]
    const int64_t mlim = m0 + TI_TILE < R.mV ? m0 + TI_TILE : R.mV;  // outputs below mlim are summed
    const int cnt = mlim <= m0 ? 0 : (int)(((mlim - 1) / nw - j0) * orig) + K;  // <= TI_SPAN (checked on the host)
    for (int e = threadIdx.x; e < cnt; e += 256) xs[e] = in(span0 + e);
    __syncthreads();
#pragma unroll 1
    for (int q = 0; q < TI_TILE / 256; ++q) {
      const int64_t m = m0 + q * 256 + threadIdx.x;
      if (m >= R.mE) continue;
      float acc = 0.f;
      if (m < mlim) {
        const int64_t j = m / nw;
        const int p = (int)(m - j * nw);
        const float* xr = xs + (int)((j - j0) * orig);
        const float* kp = kt + p;
        for (int k = 0; k < K; ++k) acc = fmaf(xr[k], kp[k * nw], acc);
      }
      store(m, acc);
    }
    return;
  }
  // wide form: tile = frame tile * phase blocks + phase block
  const int npb = (nw + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int p = (int)(tile % npb) * 64 + lane;
  const bool pok = p < nw;
  const int64_t j0 = R.mA / nw + ((tile / npb) * RS_WAVES + wave) * RS_R;  // this wave's first frame
  float* xw = xs + wave * (RS_KC * RS_R);                                  // xw[k][r]
  float acc[RS_R];
#pragma unroll
  for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
  for (int kc = 0; kc < K; kc += RS_KC) {
    __syncthreads();  // the previous chunk's reads are done
#pragma unroll 4
    for (int e = lane; e < RS_KC * RS_R; e += 64) {
      const int r = e % RS_R, k = e / RS_R;
      const int64_t i = (j0 + r) * orig + kc + k - width;
      xw[e] = kc + k < K ? in(i) : 0.f;
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

// table [n_rows][SB_COLS] int64: slot, byte offset, frames, frames before,
// final, rate index, channels, encoding, start frame, push parity;
// tiles [n_tiles][2] int32: row, tile
__global__ __launch_bounds__(256) void stream_push_kernel(const unsigned char* __restrict__ chunks,
                                                          const int64_t* __restrict__ table, int n_rows,
                                                          const int32_t* __restrict__ tiles, StreamRates rates,
                                                          float* __restrict__ arena, float* __restrict__ carry,
                                                          int64_t slots, int64_t cap, int64_t window) {
  __shared__ __attribute__((aligned(16))) float xs[TI_SPAN];
  const int row = tiles[2 * (int64_t)blockIdx.x], tile = tiles[2 * (int64_t)blockIdx.x + 1];
  if (row < 0 || row >= n_rows || tile < 0) return;  // block-uniform
  const int64_t* t = table + (int64_t)row * SB_COLS;
  const int64_t slot = t[0], n = t[2], fb = t[3], start = t[8];
  const bool fin = t[4] != 0;
  const int ri = (int)t[5], channels = (int)t[6], enc = (int)t[7], par = (int)(t[9] & 1);
  if (slot < 0 || slot >= slots || ri < 0 || ri >= TI_MAX_RATES) return;
  const float* kt = rates.kt[ri];
  const int orig = rates.orig[ri], nw = rates.nw[ri], width = rates.width[ri], K = rates.K[ri];
  const SbRow R = sb_row(!kt, orig, nw, width, start, fb, n, fin, window);
  float* ring = arena + slot * 2 * cap;
  const float* c_old = carry + (slot * 2 + par) * SB_CARRY;
  float* c_new = carry + (slot * 2 + (par ^ 1)) * SB_CARRY;
  const unsigned char* x = chunks + t[1];
  if (enc == SAD_PCM_I16) {
    const SbIn<int16_t> in{(const int16_t*)x, c_old, start, fb, n, R.cb0, channels, (float)channels};
    sb_tile<int16_t>(xs, in, R, kt, orig, nw, width, K, tile, fin, ring, cap, c_new);
  } else {
    const SbIn<float> in{(const float*)x, c_old, start, fb, n, R.cb0, channels, (float)channels};
    sb_tile<float>(xs, in, R, kt, orig, nw, width, K, tile, fin, ring, cap, c_new);
  }
}

// the rule of sad_train_ingest_file_tiles, and a carry that fits its buffer
static bool sb_rate_ok(bool native, const RsGeometry& q) {
  if (native) return true;
  if (q.K > SB_CARRY) return false;
  return q.nw >= 64 || rs_per_output_fits(q);
}

static const char* SB_RATE_MSG =
    "sample rate not supported by the batched kernel: few phases and a long input span, or more than 8192 taps";

}  // namespace sad

using namespace sad;

extern "C" int sad_stream_bank_size(int64_t slots, int64_t window, int64_t hop, int64_t max_chunk_frames,
                                    int32_t target_rate, int64_t* cap, int64_t* arena_len, int64_t* carry_len) {
  SAD_REQUIRE(cap && arena_len && carry_len, "null cap / arena_len / carry_len");
  SAD_REQUIRE(slots >= 1 && slots <= (1 << 20), "slots must be in [1, 2^20]");
  SAD_REQUIRE(window >= 1 && window <= (1ll << 28), "window must be in [1, 2^28]");
  SAD_REQUIRE(hop >= 1 && hop <= window, "hop must be in [1, window]");
  SAD_REQUIRE(max_chunk_frames >= 1 && max_chunk_frames <= (1ll << 24), "max_chunk_frames must be in [1, 2^24]");
  SAD_REQUIRE(target_rate > 0, "sample rates must be positive");
  // room for what one launch can add: a chunk at up to 4 outputs per frame (8 kHz -> 32 kHz)
  const int64_t room = 4 * max_chunk_frames > SB_MIN_ROOM ? 4 * max_chunk_frames : SB_MIN_ROOM;
  *cap = (window + room + 3) / 4 * 4;  // float4-aligned slots
  *arena_len = slots * 2 * *cap;
  *carry_len = slots * 2 * SB_CARRY;
  return SAD_OK;
}

extern "C" int sad_stream_open_check(int32_t rate, int32_t target_rate, int32_t channels, int64_t window,
                                     int64_t hop, int64_t cap, int64_t start_frame, int64_t* first_sample) {
  SAD_REQUIRE(first_sample, "null first_sample");
  SAD_REQUIRE(rate > 0 && target_rate > 0, "sample rates must be positive");
  SAD_REQUIRE(channels >= 1 && channels <= 64, "channels must be in [1, 64]");
  SAD_REQUIRE(hop >= 1 && window >= hop, "hop must be in [1, window]");
  SAD_REQUIRE(window <= cap, "window > CAP: the bank's rings are shorter than one window");
  SAD_REQUIRE(start_frame >= 0 && start_frame <= SB_MAX_FRAMES, "start_frame must be in [0, 2^40]");
  const bool native = rate == target_rate;
  const RsGeometry q = rs_geometry(rate, target_rate);
  SAD_REQUIRE(sb_rate_ok(native, q), SB_RATE_MSG);
  // the least a launch can add is one polyphase frame; the most the end of a feed adds is its tail
  SAD_REQUIRE(native || (int64_t)q.nw * (2 + (q.width + q.orig - 1) / q.orig) <= cap - window,
              "sample rate not supported by this bank: one frame's outputs and the end-of-feed tail exceed "
              "CAP - window");
  SAD_REQUIRE(start_frame % q.orig == 0, "start_frame must be a multiple of orig (the rate reduced by the gcd)");
  const int64_t g0 = start_frame / q.orig * q.nw;
  SAD_REQUIRE(g0 % hop == 0, "start_frame must map to a 32 kHz sample that is a multiple of hop");
  *first_sample = g0;
  return SAD_OK;
}

extern "C" int sad_stream_push_tiles(int32_t rate, int32_t target_rate, int64_t start_frame, int64_t frames_before,
                                     int64_t n_frames, int32_t final, int64_t window, int64_t* first_out,
                                     int64_t* end_out, int64_t* n_tiles) {
  SAD_REQUIRE(n_tiles, "null n_tiles");
  SAD_REQUIRE(rate > 0 && target_rate > 0, "sample rates must be positive");
  SAD_REQUIRE(window >= 1 && window <= (1ll << 28), "window must be in [1, 2^28]");
  SAD_REQUIRE(start_frame >= 0 && frames_before >= start_frame && n_frames >= 0 &&
                  frames_before <= SB_MAX_FRAMES && n_frames <= SB_MAX_FRAMES,
              "frames: 0 <= start_frame <= frames_before <= 2^40, 0 <= n_frames <= 2^40");
  const bool native = rate == target_rate;
  const RsGeometry q = rs_geometry(rate, target_rate);
  SAD_REQUIRE(sb_rate_ok(native, q), SB_RATE_MSG);
  SAD_REQUIRE(start_frame % q.orig == 0, "start_frame must be a multiple of orig (the rate reduced by the gcd)");
  const SbRow R = sb_row(native, q.orig, q.nw, q.width, start_frame, frames_before, n_frames, final != 0, window);
  if (first_out) *first_out = R.mA;
  if (end_out) *end_out = R.mE;
  *n_tiles = sb_out_tiles(native, q.nw, R) + sb_carry_tiles(native, q.K, final != 0);
  return SAD_OK;
}

extern "C" int sad_stream_push_run(const void* chunks, int64_t chunk_bytes, const int64_t* table,
                                   const int64_t* d_table, int64_t n_rows, const int32_t* d_tiles, int64_t n_tiles,
                                   const sad_resample_plan* const* rate_plans, int32_t n_rates, float* arena,
                                   float* carry, int64_t slots, int64_t cap, int64_t window, void* stream) {
  SAD_REQUIRE(slots >= 1 && slots <= (1 << 20), "slots must be in [1, 2^20]");
  SAD_REQUIRE(window >= 1 && window <= (1ll << 28), "window must be in [1, 2^28]");
  SAD_REQUIRE(window <= cap, "window > CAP: the bank's rings are shorter than one window");
  SAD_REQUIRE(cap <= (1ll << 30) && cap % 4 == 0, "CAP must be a multiple of 4, at most 2^30");
  SAD_REQUIRE(n_rows >= 0 && n_rows <= slots, "n_rows must be in [0, slots]");
  SAD_REQUIRE(n_rates >= 1 && n_rates <= TI_MAX_RATES, "n_rates must be in [1, 8]");
  SAD_REQUIRE(chunk_bytes >= 0, "chunk_bytes < 0");
  if (n_rows == 0) return SAD_OK;
  SAD_REQUIRE(chunks && table && d_table && d_tiles && rate_plans && arena && carry, "null pointer");
  StreamRates rates = {};
  RsGeometry geo[TI_MAX_RATES] = {};
  for (int r = 0; r < n_rates; ++r) {
    const sad_resample_plan* p = rate_plans[r];  // nullptr: the target rate
    geo[r].orig = rates.orig[r] = 1;
    geo[r].nw = rates.nw[r] = 1;
    if (!p) continue;
    rates.kt[r] = p->d_kt;
    geo[r].orig = rates.orig[r] = p->orig;
    geo[r].nw = rates.nw[r] = p->nw;
    geo[r].width = rates.width[r] = p->width;
    geo[r].K = rates.K[r] = p->K;
    SAD_REQUIRE(sb_rate_ok(false, geo[r]), SB_RATE_MSG);
  }
  std::vector<char> seen((size_t)slots, 0);
  int64_t tiles = 0;
  for (int64_t i = 0; i < n_rows; ++i) {
    const int64_t* t = table + i * SB_COLS;
    const int64_t slot = t[0], off = t[1], n = t[2], fb = t[3], fin = t[4], ri = t[5], ch = t[6], enc = t[7],
                  start = t[8], par = t[9];
    SAD_REQUIRE(slot >= 0 && slot < slots, "push table: slot out of range");
    SAD_REQUIRE(!seen[(size_t)slot], "push table: a slot appears twice in one launch");
    seen[(size_t)slot] = 1;
    SAD_REQUIRE(ch >= 1 && ch <= 64, "push table: channels must be in [1, 64]");
    SAD_REQUIRE(enc == SAD_PCM_I16 || enc == SAD_PCM_F32, "push table: encoding must be SAD_PCM_I16 or SAD_PCM_F32");
    SAD_REQUIRE(ri >= 0 && ri < n_rates, "push table: rate index out of range");
    SAD_REQUIRE((fin == 0 || fin == 1) && (par == 0 || par == 1), "push table: final / parity must be 0 or 1");
    SAD_REQUIRE(start >= 0 && fb >= start && fb <= SB_MAX_FRAMES && n >= 0 && n <= SB_MAX_FRAMES,
                "push table: frames: 0 <= start frame <= frames before <= 2^40, 0 <= frames <= 2^40");
    SAD_REQUIRE(off >= 0 && off % 16 == 0, "push table: a chunk must start at a multiple of 16 bytes");
    const int64_t bytes = n * ch * (enc == SAD_PCM_I16 ? 2 : 4);
    SAD_REQUIRE(off <= chunk_bytes && bytes <= chunk_bytes - off, "push table: a chunk lies past the end of the arena");
    const bool native = rate_plans[ri] == nullptr;
    const RsGeometry& q = geo[ri];
    SAD_REQUIRE(start % q.orig == 0, "push table: start frame must be a multiple of orig");
    const SbRow R = sb_row(native, q.orig, q.nw, q.width, start, fb, n, fin != 0, window);
    // the ring keeps less than one window of examined samples; what a launch adds must fit beside it
    SAD_REQUIRE(R.mE - R.mA <= cap - window || R.mE - start / q.orig * q.nw <= cap,
                "push table: a chunk adds more samples than CAP - window (split it)");
    tiles += sb_out_tiles(native, q.nw, R) + sb_carry_tiles(native, q.K, fin != 0);
  }
  SAD_REQUIRE(n_tiles == tiles, "n_tiles is not the sum of the rows' tile counts (sad_stream_push_tiles)");
  SAD_REQUIRE(tiles < (1ll << 31), "too many tiles for one launch");
  if (tiles == 0) return SAD_OK;
  hipLaunchKernelGGL(stream_push_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream,
                     (const unsigned char*)chunks, d_table, (int)n_rows, d_tiles, rates, arena, carry, slots, cap,
                     window);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}
