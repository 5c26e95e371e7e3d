// evidence.hip -- evidence maps (Grad-CAM of the eval-mode head on the layer4
// activation; include/sad.h "evidence"):
//   E[b, m, p] = (1 / hw) sum_c g_m[b, c] A[b, p, c]
// for every map m of one backbone in ONE pass over A, plus the two small
// helpers of sad_heads_grad_run (ReLU-mask multiply, weight transpose).
//
// evidence_kernel.  Workgroup = 64 pixels of one window, 4 waves.  The
// workgroup stages g_m[b, :] of all maps in LDS (n_maps * C floats).  A wave
// takes 4 pixels at a time; lane l loads 16 B of each pixel's NHWC row per
// chunk (8 channels of a 16-bit layout, 4 of fp32; split-bf16: the 16 B of hi
// and the 16 B of lo of 8 channels, value = hi + lo) and reads its g slice of
// every map from LDS once per chunk for the 4 pixels.  Accumulation is fp32
// FMA per lane in channel order; the 4 * NM per-lane sums are then reduced
// over the 64 lanes by a reduce-scatter (lane bit s at step s: a lane keeps
// half of its values and adds its partner's), so every sum goes through the
// same tree (bit 0, 1, .. 5) and lands in lane 4 m + p.  No atomics; the order
// is a function of (C, layout) alone: the output is bit-reproducible and does
// not depend on B, on the window's position in the batch or on n_maps.
#include "common.hpp"
#include "kernels.hpp"

using namespace sad;

namespace {

constexpr int EV_MAX_MAPS = 16;
constexpr int EV_PIX_WG = 64;            // pixels per workgroup
constexpr int EV_LDS_FLOATS = 32 * 1024; // 128 KiB of g

struct EvG {
  const float* g[EV_MAX_MAPS];
};

enum { L_BF16 = 0, L_F16 = 1, L_F32 = 2, L_X3 = 3 };

template <int L>
constexpr int ev_cpl() {  // channels per lane and chunk
  return L == L_F32 ? 4 : 8;
}

// the CPL channels of pixel row `row` starting at channel c0, as floats
template <int L>
__device__ __forceinline__ void ev_load(const void* row, int c0, float (&a)[ev_cpl<L>()]) {
  if constexpr (L == L_F32) {
    const float4 v = *(const float4*)((const float*)row + c0);
    a[0] = v.x;
    a[1] = v.y;
    a[2] = v.z;
    a[3] = v.w;
  } else if constexpr (L == L_X3) {
    // [hi 32 | lo 32] per 32 channels: c0 is a multiple of 8, so the 8 hi (and
    // the 8 lo, 32 elements on) are 16 contiguous, aligned bytes
    const u16* p = (const u16*)row + ((c0 >> 5) << 6) + (c0 & 31);
    const uint4 h = *(const uint4*)p;
    const uint4 l = *(const uint4*)(p + 32);
    const uint32_t hq[4] = {h.x, h.y, h.z, h.w}, lq[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[2 * i] = lo16<u16>(hq[i]) + lo16<u16>(lq[i]);
      a[2 * i + 1] = hi16<u16>(hq[i]) + hi16<u16>(lq[i]);
    }
  } else {
    using E = typename std::conditional<L == L_F16, f16, u16>::type;
    const uint4 v = *(const uint4*)((const u16*)row + c0);
    const uint32_t q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[2 * i] = lo16<E>(q[i]);
      a[2 * i + 1] = hi16<E>(q[i]);
    }
  }
}

template <int L, int NM>
__global__ __launch_bounds__(256) void evidence_kernel(const void* __restrict__ l4, int hw, int C, EvG gp, int n_maps,
                                                       int tiles, float* __restrict__ out) {
  extern __shared__ float gs[];  // [n_maps][C]
  constexpr int CPL = ev_cpl<L>();
  constexpr int V = 4 * NM;  // values per lane: 4 pixels x NM maps (a power of two)
  const int64_t b = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    if (m < n_maps) {
      const float* g = gp.g[m] + b * C;
      for (int c = tid * 4; c < C; c += 1024) *(float4*)(gs + m * C + c) = *(const float4*)(g + c);
    }
  }
  __syncthreads();
  // bytes per pixel row: 2 B (16-bit), 4 B (fp32, split-bf16) per channel
  const int64_t row_bytes = (int64_t)C * (L == L_BF16 || L == L_F16 ? 2 : 4);
  const char* img = (const char*)l4 + b * hw * row_bytes;
  for (int it = 0; it < EV_PIX_WG / 16; ++it) {
    const int pix0 = tile * EV_PIX_WG + it * 16 + wave * 4;
    if (pix0 >= hw) break;  // (wave-uniform)
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    for (int c0 = lane * CPL; c0 < C; c0 += 64 * CPL) {
      float a[4][CPL];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (pix0 + p < hw) {
          ev_load<L>(img + (int64_t)(pix0 + p) * row_bytes, c0, a[p]);
        } else {
#pragma unroll
          for (int j = 0; j < CPL; ++j) a[p][j] = 0.f;
        }
      }
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        if (m < n_maps) {
          float gv[CPL];
#pragma unroll
          for (int j = 0; j < CPL; j += 4) {
            const float4 t = *(const float4*)(gs + m * C + c0 + j);
            gv[j] = t.x;
            gv[j + 1] = t.y;
            gv[j + 2] = t.z;
            gv[j + 3] = t.w;
          }
#pragma unroll
          for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int j = 0; j < CPL; ++j) acc[m * 4 + p] = __builtin_fmaf(a[p][j], gv[j], acc[m * 4 + p]);
        }
      }
    }
    // reduce-scatter over the lanes: after step s a lane holds the values whose
    // index bit s equals its lane bit s, summed over the lane pair
    int n = V;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      if (n > 1) {
        const bool up = (lane >> s) & 1;
#pragma unroll
        for (int i = 0; i < V / 2; ++i) {
          if (i < n / 2) {
            const float keep = up ? acc[2 * i + 1] : acc[2 * i];
            const float send = up ? acc[2 * i] : acc[2 * i + 1];
            acc[i] = keep + __shfl_xor(send, 1 << s);
          }
        }
        n >>= 1;
      } else {
        acc[0] += __shfl_xor(acc[0], 1 << s);
      }
    }
    // lane i < V holds value i = 4 m + p
    const int m = lane >> 2, p = lane & 3;
    if (lane < V && m < n_maps && pix0 + p < hw) out[(b * n_maps + m) * hw + pix0 + p] = acc[0] / (float)hw;
  }
}

template <int L, int NM>
int launch_ev(const void* l4, int64_t B, int hw, int C, const EvG& g, int n_maps, float* out, hipStream_t s) {
  const int smem = n_maps * C * (int)sizeof(float);
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)evidence_kernel<L, NM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              EV_LDS_FLOATS * (int)sizeof(float));
    attr = true;
  }
  const int tiles = (hw + EV_PIX_WG - 1) / EV_PIX_WG;
  hipLaunchKernelGGL((evidence_kernel<L, NM>), dim3((unsigned)(B * tiles)), dim3(256), smem, s, l4, hw, C, g, n_maps,
                     tiles, out);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

template <int L>
int launch_ev_l(const void* l4, int64_t B, int hw, int C, const EvG& g, int n_maps, float* out, hipStream_t s) {
  if (n_maps <= 1) return launch_ev<L, 1>(l4, B, hw, C, g, n_maps, out, s);
  if (n_maps <= 2) return launch_ev<L, 2>(l4, B, hw, C, g, n_maps, out, s);
  if (n_maps <= 4) return launch_ev<L, 4>(l4, B, hw, C, g, n_maps, out, s);
  if (n_maps <= 8) return launch_ev<L, 8>(l4, B, hw, C, g, n_maps, out, s);
  return launch_ev<L, 16>(l4, B, hw, C, g, n_maps, out, s);
}

// out[r][c] = y[r][c] > 0 ? (vec ? vec[c] : out[r][c]) : 0  (the ReLU gradient mask: a unit at exactly 0 is off)
__global__ __launch_bounds__(256) void relu_mask_kernel(const float* __restrict__ y, int64_t y_stride,
                                                        const float* __restrict__ vec, float* out, int64_t rows,
                                                        int cols) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const int64_t r = i / cols;
  const int c = (int)(i % cols);
  const bool on = y[r * y_stride + c] > 0.f;
  out[i] = on ? (vec ? vec[c] : out[i]) : 0.f;
}

// dst [cols][rows] = src [rows][cols]^T (plan build, once)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                        int rows, int cols) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * cols) return;
  const int r = (int)(i % rows), c = (int)(i / rows);  // consecutive threads write consecutive dst
  dst[i] = src[(int64_t)r * cols + c];
}

}  // namespace

int sad::launch_relu_mask(const float* y, int64_t y_stride, const float* vec, float* out, int64_t rows, int cols,
                          hipStream_t s) {
  if (rows == 0) return SAD_OK;
  const int64_t n = rows * cols;
  hipLaunchKernelGGL(relu_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, y, y_stride, vec, out, rows,
                     cols);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

int sad::launch_transpose(const float* src, float* dst, int rows, int cols, hipStream_t s) {
  const int64_t n = (int64_t)rows * cols;
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, rows, cols);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

extern "C" int sad_evidence_run(const void* l4, int32_t dtype, int64_t B, int32_t hw, int32_t C,
                                const float* const* g, int32_t n_maps, float* out, void* stream) {
  SAD_REQUIRE(l4 && g && out, "evidence: null l4, g or out");
  SAD_REQUIRE(dtype == SAD_F32 || dtype == SAD_BF16 || dtype == SAD_BF16X3 || dtype == SAD_F16, "evidence: dtype");
  SAD_REQUIRE(n_maps >= 1 && n_maps <= EV_MAX_MAPS, "evidence: n_maps must be in 1..16");
  SAD_REQUIRE(hw >= 1, "evidence: hw must be at least 1");
  SAD_REQUIRE(C > 0 && C % 64 == 0, "evidence: C must be a positive multiple of 64");
  SAD_REQUIRE((int64_t)n_maps * C <= EV_LDS_FLOATS, "evidence: n_maps * C exceeds 32768 (the maps' gradients stay in LDS)");
  SAD_REQUIRE(B >= 0 && B * ((hw + EV_PIX_WG - 1) / EV_PIX_WG) < (1ll << 31), "evidence: batch");
  EvG eg{};
  for (int m = 0; m < n_maps; ++m) {
    SAD_REQUIRE(g[m], "evidence: null gradient pointer");
    eg.g[m] = g[m];
  }
  if (B == 0) return SAD_OK;
  hipStream_t s = (hipStream_t)stream;
  switch (dtype) {
    case SAD_BF16: return launch_ev_l<L_BF16>(l4, B, hw, C, eg, n_maps, out, s);
    case SAD_F16: return launch_ev_l<L_F16>(l4, B, hw, C, eg, n_maps, out, s);
    case SAD_F32: return launch_ev_l<L_F32>(l4, B, hw, C, eg, n_maps, out, s);
    default: return launch_ev_l<L_X3>(l4, B, hw, C, eg, n_maps, out, s);
  }
}
