// ingest.hpp -- what the ingestion kernels share (ingest.hip, stream.hip): the
// resample plan, torchaudio's polyphase geometry, the blocking constants of the
// wide form and the mono mix of one stored frame.
#pragma once
#include <math.h>

#include "common.hpp"

struct sad_resample_plan {
  int32_t orig_freq = 0, new_freq = 0;
  int orig = 1, nw = 1, width = 0, K = 0;  // reduced by the gcd
  float* d_kt = nullptr;                    // [K][nw] fp32
  int device = 0;
};

namespace sad {

// resample_wide_kernel's blocking: RS_R frames per wave, RS_KC taps per LDS chunk
constexpr int RS_R = 16, RS_KC = 64, RS_WAVES = 4;
constexpr int TI_TILE = 1024;     // outputs per tile, native and per-output forms
constexpr int TI_SPAN = 8192;     // LDS floats: the per-output form's input span
constexpr int TI_MAX_RATES = 8;   // distinct sample rates in one launch
static_assert(TI_SPAN >= RS_WAVES * RS_KC * RS_R, "the wide form's staging fits the span buffer");

// pcm_mono_kernel's value at frame i; 0 outside the frames that were read
template <typename IT>
__device__ __forceinline__ float ti_mono(const IT* __restrict__ x, int64_t i, int64_t n_read, int channels,
                                         float fc) {
  const float scale = sizeof(IT) == 2 ? (1.0f / 32768.0f) : 1.0f;
  if (i < 0 || i >= n_read) return 0.f;
  const IT* p = x + i * channels;
  float s = (float)p[0] * scale;
  for (int c = 1; c < channels; ++c) s += (float)p[c] * scale;
  return channels == 1 ? s : s / fc;
}

// torchaudio's polyphase geometry for orig_freq -> new_freq (sinc_interp_hann,
// lowpass_filter_width 6, rolloff 0.99): rates reduced by their gcd, the filter
// half-width in input samples and the taps per output
struct RsGeometry {
  int orig, nw, width, K;
  double base;
};

inline int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

inline RsGeometry rs_geometry(int32_t orig_freq, int32_t new_freq) {
  const int64_t g = gcd64(orig_freq, new_freq);
  RsGeometry q;
  q.orig = (int)(orig_freq / g);
  q.nw = (int)(new_freq / g);
  q.base = (double)(q.orig < q.nw ? q.orig : q.nw) * 0.99;
  q.width = (int)ceil(6 * (double)q.orig / q.base);
  q.K = 2 * q.width + q.orig;
  return q;
}

// the per-output form (nw < 64) stages the inputs of TI_TILE outputs in LDS:
// a rate whose span does not fit TI_SPAN is refused by the batched kernels
inline bool rs_per_output_fits(const RsGeometry& q) {
  return ((int64_t)(TI_TILE - 1) / q.nw + 1) * q.orig + q.K <= TI_SPAN;
}

}  // namespace sad
