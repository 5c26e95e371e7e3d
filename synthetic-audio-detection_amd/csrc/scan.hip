// scan.hip -- the device side of the catalogue scan (sad/scan.py): many files'
// waveforms sit back to back in one fp32 arena, and the two per-file jobs that
// inference_runner.main does on the host run here for all of them at once:
//
//   sad_scan_select_run   slice_waveform (inference_runner.py:176-190) for every
//     file of the arena: candidate starts at the hop, max |x| per candidate
//     (float4 loads; at overlap 0 the arena is read once), the fp32 silence
//     test, and an order-preserving compaction of the kept windows' ABSOLUTE
//     offsets (file order, then time order) + CSR row ranges per file.  The
//     offsets feed sad_frontend_run_windows with the arena as its waveform.
//   sad_scan_post_run     summarize (inference_runner.py:292-349) for every
//     file: sigmoid, the optional scipy gaussian_filter1d(sigma=2) along a
//     file's own rows + row normalisation, the Real / first-argmax label, and
//     the per-file column means in float64.
//
// Everything is sized by the host (it knows the file lengths) but DECIDED on
// the device, so a pack of files costs the host no look at the samples.  No
// atomics: compaction is a three-step prefix scan (1024-candidate tiles, one
// block over the tile sums, tiles again), sums run in a fixed order, and the
// same inputs give the same bytes.  Device-resident sizes (file_start,
// file_len, row_start) are clamped before they index anything.
#include <math.h>

#include "common.hpp"

namespace sad {

constexpr int SCAN_T = 256;               // threads per block, every kernel here
constexpr int SCAN_TILE = 4 * SCAN_T;     // candidates per compaction tile
constexpr int SCAN_RADIUS = 8;            // int(4.0 * sigma + 0.5), sigma = 2

// torch.max propagates NaN (ingest.hip nanmax)
__device__ __forceinline__ float scan_nanmax(float a, float b) { return (b > a || b != b) ? b : a; }

// len(range(0, len - window + 1, hop)) for a file that lies inside the arena
__device__ __forceinline__ int64_t file_candidates(int64_t start, int64_t len, int64_t wav_len, int64_t window,
                                                   int64_t hop) {
  if (start < 0 || len < window || start > wav_len - len) return 0;
  return (len - window) / hop + 1;
}

// exclusive scan of one int64 per thread over the block (Hillis-Steele in LDS);
// *total = the block's sum.  Every thread of the block must call it.
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t v, int64_t* sh, int64_t* total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < SCAN_T; o <<= 1) {
    const int64_t a = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += a;
    __syncthreads();
  }
  const int64_t incl = sh[t];
  *total = sh[SCAN_T - 1];
  __syncthreads();  // sh may be reused by the caller's next round
  return incl - v;
}

// cand_start[f] = candidates of files < f; cand_start[n_files] = all of them.  One block.
__global__ __launch_bounds__(SCAN_T) void scan_count_kernel(const int64_t* __restrict__ file_start,
                                                            const int64_t* __restrict__ file_len, int64_t n_files,
                                                            int64_t wav_len, int64_t window, int64_t hop,
                                                            int64_t* __restrict__ cand_start) {
  __shared__ int64_t sh[SCAN_T];
  int64_t carry = 0;
  for (int64_t base = 0; base < n_files; base += SCAN_T) {
    const int64_t f = base + threadIdx.x;
    const int64_t cnt = f < n_files ? file_candidates(file_start[f], file_len[f], wav_len, window, hop) : 0;
    int64_t tot;
    const int64_t ex = block_exclusive_scan(cnt, sh, &tot);
    if (f < n_files) cand_start[f] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) cand_start[n_files] = carry;
}

// One block per candidate c: its file by binary search in cand_start, max |x|
// over its window, keep[c] and its absolute offset cand_off[c].
__global__ __launch_bounds__(SCAN_T) void scan_absmax_kernel(const float* __restrict__ wav,
                                                             const int64_t* __restrict__ file_start,
                                                             const int64_t* __restrict__ cand_start, int64_t n_files,
                                                             int64_t window, int64_t hop, float thr, int64_t cap,
                                                             int32_t* __restrict__ keep,
                                                             int64_t* __restrict__ cand_off) {
  __shared__ float red[SCAN_T / 64];
  const int64_t all = cand_start[n_files];
  const int64_t total = all < cap ? all : cap;
  for (int64_t c = blockIdx.x; c < total; c += gridDim.x) {
    int64_t lo = 0, hi = n_files;  // first f with cand_start[f] > c; cand_start[0] = 0 <= c
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (cand_start[mid] > c) hi = mid; else lo = mid + 1;
    }
    const int64_t f = lo - 1;
    const int64_t b = file_start[f] + (c - cand_start[f]) * hop;  // inside the arena: file_candidates
    const float* p = wav + b;
    // scalar head up to a 16-byte boundary, float4 body, scalar tail
    int64_t head = (4 - (int64_t)(((uintptr_t)p >> 2) & 3)) & 3;
    if (head > window) head = window;
    const int64_t nv = (window - head) >> 2;
    const int64_t tail = head + 4 * nv;
    float m = 0.f;
    if (threadIdx.x < head) m = fabsf(p[threadIdx.x]);
    const float4* q = (const float4*)(p + head);
    for (int64_t i = threadIdx.x; i < nv; i += SCAN_T) {
      const float4 v = q[i];
      m = scan_nanmax(m, fabsf(v.x));
      m = scan_nanmax(m, fabsf(v.y));
      m = scan_nanmax(m, fabsf(v.z));
      m = scan_nanmax(m, fabsf(v.w));
    }
    if (tail + threadIdx.x < window) m = scan_nanmax(m, fabsf(p[tail + threadIdx.x]));
    for (int o = 32; o > 0; o >>= 1) m = scan_nanmax(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      const float mx = scan_nanmax(scan_nanmax(red[0], red[1]), scan_nanmax(red[2], red[3]));
      keep[c] = mx < thr ? 0 : 1;  // slice_waveform skips iff max < thr (NaN: kept)
      cand_off[c] = b;
    }
    __syncthreads();
  }
}

// tile_sum[b] = kept candidates of tile b
__global__ __launch_bounds__(SCAN_T) void scan_tile_sum_kernel(const int32_t* __restrict__ keep,
                                                               const int64_t* __restrict__ cand_start,
                                                               int64_t n_files, int64_t cap,
                                                               int64_t* __restrict__ tile_sum) {
  __shared__ int64_t sh[SCAN_T];
  const int64_t all = cand_start[n_files];
  const int64_t total = all < cap ? all : cap;
  const int64_t c0 = (int64_t)blockIdx.x * SCAN_TILE + 4 * threadIdx.x;
  int64_t n = 0;
  for (int j = 0; j < 4; ++j)
    if (c0 + j < total) n += keep[c0 + j];
  int64_t tot;
  block_exclusive_scan(n, sh, &tot);
  if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// tile_sum -> its exclusive scan, in place; pos[total] = the kept count.  One block.
__global__ __launch_bounds__(SCAN_T) void scan_tile_scan_kernel(int64_t* __restrict__ tile_sum, int64_t n_tiles,
                                                                const int64_t* __restrict__ cand_start,
                                                                int64_t n_files, int64_t cap,
                                                                int64_t* __restrict__ pos) {
  __shared__ int64_t sh[SCAN_T];
  const int64_t all = cand_start[n_files];
  const int64_t total = all < cap ? all : cap;
  int64_t carry = 0;
  for (int64_t base = 0; base < n_tiles; base += SCAN_T) {
    const int64_t b = base + threadIdx.x;
    const int64_t v = b < n_tiles ? tile_sum[b] : 0;
    int64_t tot;
    const int64_t ex = block_exclusive_scan(v, sh, &tot);
    if (b < n_tiles) tile_sum[b] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) pos[total] = carry;
}

// pos[c] = kept candidates before c; kept candidates write their offset at pos[c]
__global__ __launch_bounds__(SCAN_T) void scan_compact_kernel(const int32_t* __restrict__ keep,
                                                              const int64_t* __restrict__ cand_off,
                                                              const int64_t* __restrict__ tile_sum,
                                                              const int64_t* __restrict__ cand_start,
                                                              int64_t n_files, int64_t cap, int64_t* __restrict__ pos,
                                                              int64_t* __restrict__ offsets) {
  __shared__ int64_t sh[SCAN_T];
  const int64_t all = cand_start[n_files];
  const int64_t total = all < cap ? all : cap;
  const int64_t c0 = (int64_t)blockIdx.x * SCAN_TILE + 4 * threadIdx.x;
  int32_t k[4];
  int64_t n = 0;
  for (int j = 0; j < 4; ++j) {
    k[j] = c0 + j < total ? keep[c0 + j] : 0;
    n += k[j];
  }
  int64_t tot;
  int64_t at = tile_sum[blockIdx.x] + block_exclusive_scan(n, sh, &tot);
  for (int j = 0; j < 4; ++j) {
    if (c0 + j >= total) break;
    pos[c0 + j] = at;
    if (k[j]) offsets[at++] = cand_off[c0 + j];  // at < kept count <= total <= cap
  }
}

// row_start[f] = kept candidates of files < f
__global__ __launch_bounds__(SCAN_T) void scan_row_start_kernel(const int64_t* __restrict__ cand_start,
                                                                const int64_t* __restrict__ pos, int64_t n_files,
                                                                int64_t cap, int64_t* __restrict__ row_start) {
  const int64_t all = cand_start[n_files];
  const int64_t total = all < cap ? all : cap;
  for (int64_t f = (int64_t)blockIdx.x * SCAN_T + threadIdx.x; f <= n_files; f += (int64_t)gridDim.x * SCAN_T) {
    const int64_t c = cand_start[f];
    row_start[f] = pos[c < total ? c : total];
  }
}

// ---- post-processing ---------------------------------------------------------
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

__global__ __launch_bounds__(SCAN_T) void post_sigmoid_kernel(const float* __restrict__ x, int64_t n,
                                                              float* __restrict__ y) {
  for (int64_t i = (int64_t)blockIdx.x * SCAN_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * SCAN_T)
    y[i] = sigmoid_f32(x[i]);
}

__device__ __forceinline__ int64_t clamp_row(int64_t v, int64_t B) { return v < 0 ? 0 : (v > B ? B : v); }

// rows [*lo, *hi) of the file that owns row r; a row no file owns is its own file
__device__ __forceinline__ void file_rows(const int64_t* __restrict__ row_start, int64_t n_files, int64_t B,
                                          int64_t r, int64_t* lo, int64_t* hi) {
  int64_t a = 0, b = n_files + 1;  // first index with row_start[index] > r
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (row_start[mid] > r) b = mid; else a = mid + 1;
  }
  *lo = r;
  *hi = r + 1;
  if (a >= 1 && a <= n_files) {
    const int64_t l = clamp_row(row_start[a - 1], B), h = clamp_row(row_start[a], B);
    if (l <= r && r < h) {
      *lo = l;
      *hi = h;
    }
  }
}

// scipy's mode 'reflect' (d c b a | a b c d | d c b a), repeated for short lines
__device__ __forceinline__ int64_t reflect_index(int64_t j, int64_t n) {
  const int64_t p = 2 * n;
  j %= p;
  if (j < 0) j += p;
  return j < n ? j : p - 1 - j;
}

// numpy's float32 sum of a contiguous row of n <= 128 values (its pairwise sum
// below the block size): sequential below 8 values, else 8 interleaved partial
// sums combined as a tree, then the remainder in order
__device__ __forceinline__ float numpy_row_sum(const float* __restrict__ r, int n) {
  float s;
  if (n < 8) {
    s = 0.f;
    for (int i = 0; i < n; ++i) s += r[i];
  } else {
    float q[8];
    for (int j = 0; j < 8; ++j) q[j] = r[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) q[j] += r[i + j];
    s = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    for (; i < n; ++i) s += r[i];
  }
  return s;
}

struct GaussTaps {
  double w[SCAN_RADIUS + 1];  // w[d] = weight at distance d from the centre
};

// One thread per row: (smooth: filter the file's sigmoid rows in `raw`, normalise) -> probs, label.
template <bool SMOOTH>
__global__ __launch_bounds__(SCAN_T) void post_rows_kernel(const float* __restrict__ logits,
                                                           const float* __restrict__ raw, int64_t B, int C,
                                                           const int64_t* __restrict__ row_start, int64_t n_files,
                                                           float thr, GaussTaps taps, float* __restrict__ probs,
                                                           int32_t* __restrict__ label) {
  for (int64_t r = (int64_t)blockIdx.x * SCAN_T + threadIdx.x; r < B; r += (int64_t)gridDim.x * SCAN_T) {
    float* pr = probs + r * C;
    if (SMOOTH) {
      int64_t lo, hi;
      file_rows(row_start, n_files, B, r, &lo, &hi);
      const int64_t n = hi - lo, i = r - lo;
      const float* base = raw + lo * C;
      for (int c = 0; c < C; ++c) {
        // scipy correlate1d, symmetric filter: centre tap, then the pairs from the far end inwards
        double acc = __dmul_rn((double)base[i * C + c], taps.w[0]);
        for (int d = SCAN_RADIUS; d >= 1; --d) {
          const double pair = __dadd_rn((double)base[reflect_index(i - d, n) * C + c],
                                        (double)base[reflect_index(i + d, n) * C + c]);
          acc = __dadd_rn(acc, __dmul_rn(pair, taps.w[d]));
        }
        pr[c] = (float)acc;
      }
      const float s = numpy_row_sum(pr, C);  // this thread's own stores
      if (s > 0.f)
        for (int c = 0; c < C; ++c) pr[c] = pr[c] / s;
    } else {
      const float* lg = logits + r * C;
      for (int c = 0; c < C; ++c) pr[c] = sigmoid_f32(lg[c]);
    }
    // Real iff p_real >= thr and every synthetic p < thr; else the first argmax (NaN counts as the maximum)
    bool any = false;
    int best = 0;
    float bv = pr[0];
    for (int c = 0; c < C - 1; ++c) {
      const float v = pr[c];
      if (!(v < thr)) any = true;
      if (v > bv || (v != v && bv == bv)) {
        bv = v;
        best = c;
      }
    }
    label[r] = (pr[C - 1] >= thr && !any) ? -1 : best;
  }
}

// mean[f][c]: thread t sums rows t, t + 256, ... in float64, then a fixed tree over the block
__global__ __launch_bounds__(SCAN_T) void post_mean_kernel(const float* __restrict__ probs, int64_t B, int C,
                                                           const int64_t* __restrict__ row_start, int64_t n_files,
                                                           double* __restrict__ mean) {
  __shared__ double sh[SCAN_T];
  const int c = blockIdx.y;
  for (int64_t f = blockIdx.x; f < n_files; f += gridDim.x) {
    const int64_t lo = clamp_row(row_start[f], B), hi = clamp_row(row_start[f + 1], B);
    double s = 0.0;
    for (int64_t r = lo + threadIdx.x; r < hi; r += SCAN_T) s += (double)probs[r * C + c];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = SCAN_T / 2; o > 0; o >>= 1) {
      if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) mean[f * C + c] = hi > lo ? sh[0] / (double)(hi - lo) : 0.0;
    __syncthreads();
  }
}

static unsigned blocks_for(int64_t n, int64_t per_block, int64_t max_blocks) {
  const int64_t g = (n + per_block - 1) / per_block;
  return (unsigned)(g < 1 ? 1 : (g < max_blocks ? g : max_blocks));
}

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// select workspace: cand_start [n_files + 1] | cand_off [cap] | pos [cap + 1] | tile_sum [tiles] | keep [cap] (int32)
struct SelectLayout {
  size_t cand_start, cand_off, pos, tile_sum, keep, bytes;
  int64_t tiles;
};
static SelectLayout select_layout(int64_t n_files, int64_t cap) {
  SelectLayout L;
  L.tiles = (cap + SCAN_TILE - 1) / SCAN_TILE;
  size_t o = 0;
  L.cand_start = o, o = align256(o + (size_t)(n_files + 1) * 8);
  L.cand_off = o, o = align256(o + (size_t)cap * 8);
  L.pos = o, o = align256(o + (size_t)(cap + 1) * 8);
  L.tile_sum = o, o = align256(o + (size_t)(L.tiles + 1) * 8);
  L.keep = o, o = align256(o + (size_t)cap * 4);
  L.bytes = o;
  return L;
}

}  // namespace sad

using namespace sad;

static const int64_t SCAN_MAX = 1ll << 40;  // files / candidates / rows: keeps every size product inside int64

extern "C" int sad_scan_select_workspace_size(int64_t n_files, int64_t max_candidates, size_t* bytes) {
  SAD_REQUIRE(bytes, "null bytes");
  SAD_REQUIRE(n_files >= 0 && n_files <= SCAN_MAX && max_candidates >= 0 && max_candidates <= SCAN_MAX,
              "n_files / max_candidates");
  *bytes = select_layout(n_files, max_candidates).bytes;
  return SAD_OK;
}

extern "C" int sad_scan_select_run(const float* wav, int64_t wav_len, const int64_t* file_start,
                                   const int64_t* file_len, int64_t n_files, int64_t window, int64_t hop,
                                   float silence_threshold, int64_t max_candidates, int64_t* offsets,
                                   int64_t* row_start, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(n_files >= 0 && n_files <= SCAN_MAX && max_candidates >= 0 && max_candidates <= SCAN_MAX,
              "n_files / max_candidates");
  SAD_REQUIRE(wav_len >= 0 && wav_len <= SCAN_MAX && window > 0 && hop > 0, "wav_len / window / hop");
  SAD_REQUIRE(row_start && ws, "null row_start / workspace");
  SAD_REQUIRE(n_files == 0 || (file_start && file_len), "null file_start / file_len");
  SAD_REQUIRE(max_candidates == 0 || (wav && offsets), "null wav / offsets");
  SAD_REQUIRE(((uintptr_t)ws & 7) == 0 && ((uintptr_t)wav & 3) == 0, "misaligned workspace / wav");
  const SelectLayout L = select_layout(n_files, max_candidates);
  if (ws_bytes < L.bytes) {
    set_error("sad_scan_select_run: workspace too small (sad_scan_select_workspace_size)");
    return SAD_ERR_NOMEM;
  }
  char* w = (char*)ws;
  int64_t* cand_start = (int64_t*)(w + L.cand_start);
  int64_t* cand_off = (int64_t*)(w + L.cand_off);
  int64_t* pos = (int64_t*)(w + L.pos);
  int64_t* tile_sum = (int64_t*)(w + L.tile_sum);
  int32_t* keep = (int32_t*)(w + L.keep);
  hipStream_t s = (hipStream_t)stream;
  const int64_t cap = max_candidates;
  hipLaunchKernelGGL(scan_count_kernel, dim3(1), dim3(SCAN_T), 0, s, file_start, file_len, n_files, wav_len, window,
                     hop, cand_start);
  if (cap > 0) {
    hipLaunchKernelGGL(scan_absmax_kernel, dim3(blocks_for(cap, 1, 1 << 20)), dim3(SCAN_T), 0, s, wav, file_start,
                       cand_start, n_files, window, hop, silence_threshold, cap, keep, cand_off);
    hipLaunchKernelGGL(scan_tile_sum_kernel, dim3((unsigned)L.tiles), dim3(SCAN_T), 0, s, keep, cand_start, n_files,
                       cap, tile_sum);
  }
  hipLaunchKernelGGL(scan_tile_scan_kernel, dim3(1), dim3(SCAN_T), 0, s, tile_sum, L.tiles, cand_start, n_files, cap,
                     pos);
  if (cap > 0)
    hipLaunchKernelGGL(scan_compact_kernel, dim3((unsigned)L.tiles), dim3(SCAN_T), 0, s, keep, cand_off, tile_sum,
                       cand_start, n_files, cap, pos, offsets);
  hipLaunchKernelGGL(scan_row_start_kernel, dim3(blocks_for(n_files + 1, SCAN_T, 4096)), dim3(SCAN_T), 0, s,
                     cand_start, pos, n_files, cap, row_start);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

extern "C" int sad_scan_post_workspace_size(int64_t B, int32_t C, int32_t smooth, size_t* bytes) {
  SAD_REQUIRE(bytes, "null bytes");
  SAD_REQUIRE(B >= 0 && B <= SCAN_MAX && C >= 2 && C <= 128, "B, or C outside [2, 128]");
  *bytes = smooth ? align256((size_t)B * C * 4) : 0;  // the sigmoid rows the filter reads
  return SAD_OK;
}

extern "C" int sad_scan_post_run(const float* logits, int64_t B, int32_t C, const int64_t* row_start,
                                 int64_t n_files, float threshold, int32_t smooth, float* probs, int32_t* label,
                                 double* mean, void* ws, size_t ws_bytes, void* stream) {
  size_t need = 0;
  if (int rc = sad_scan_post_workspace_size(B, C, smooth, &need)) return rc;
  SAD_REQUIRE(n_files >= 0 && n_files <= SCAN_MAX, "n_files");
  SAD_REQUIRE(row_start, "null row_start");
  SAD_REQUIRE(n_files == 0 || mean, "null mean");
  SAD_REQUIRE(B == 0 || (logits && probs && label), "null logits / probs / label");
  SAD_REQUIRE(need == 0 || ws, "null workspace");
  if (ws_bytes < need) {
    set_error("sad_scan_post_run: workspace too small (sad_scan_post_workspace_size)");
    return SAD_ERR_NOMEM;
  }
  hipStream_t s = (hipStream_t)stream;
  GaussTaps taps;
  {  // scipy _gaussian_kernel1d(sigma=2, order=0, radius=8): exp(-x^2 / (2 sigma^2)), normalised to sum 1
    double phi[2 * SCAN_RADIUS + 1], sum = 0.0;
    for (int x = -SCAN_RADIUS; x <= SCAN_RADIUS; ++x) sum += phi[x + SCAN_RADIUS] = exp(-0.5 / 4.0 * (double)(x * x));
    for (int d = 0; d <= SCAN_RADIUS; ++d) taps.w[d] = phi[SCAN_RADIUS + d] / sum;
  }
  if (B > 0) {
    float* raw = (float*)ws;
    const unsigned g = blocks_for(B, SCAN_T, 65536);
    if (smooth) {
      hipLaunchKernelGGL(post_sigmoid_kernel, dim3(blocks_for(B * C, SCAN_T, 65536)), dim3(SCAN_T), 0, s, logits,
                         B * C, raw);
      hipLaunchKernelGGL(post_rows_kernel<true>, dim3(g), dim3(SCAN_T), 0, s, logits, raw, B, (int)C, row_start,
                         n_files, threshold, taps, probs, label);
    } else {
      hipLaunchKernelGGL(post_rows_kernel<false>, dim3(g), dim3(SCAN_T), 0, s, logits, raw, B, (int)C, row_start,
                         n_files, threshold, taps, probs, label);
    }
  }
  if (n_files > 0)
    hipLaunchKernelGGL(post_mean_kernel, dim3(blocks_for(n_files, 1, 32768), (unsigned)C), dim3(SCAN_T), 0, s, probs,
                       B, (int)C, row_start, n_files, mean);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}
