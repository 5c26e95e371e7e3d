// halo256r.hip -- variant 31: patch-resident 256 x 256 block conv with the
// weights streamed straight into registers (bf16, gfx950).
//
// Replaces the same timm BasicBlock halves as variants 13 / 30 (conv -> bn
// [-> + shortcut] -> relu, inference_runner.py:49-51 via timm resnet18
// forward_features) for the layer3 / layer4 convs with stride 1:
//   out[px, co] = act( sum_{tap, ci} X0[px + tap; ci] W0[co, tap, ci]
//                    + sum_{k1} X1[px * ss1; k1] W1[co, k1] + bias[co] + R[px, co] )
// (X1: the downsample shortcut's source as K columns; R: the identity shortcut
// as an epilogue residual, bf16 only; the split-bf16 form takes both as X1)
//
// Why a third form.  Variants 13 and 30 stage BOTH operands in LDS and so need
// a workgroup barrier per 64-deep K-step (the weight stage of step g+1 is
// filled by DMA while step g reads the other one).  Their stamps put a K-step
// at ~3,600 cycles for 2,048 cycles of MFMA per SIMD: after every barrier both
// waves of a SIMD read fragments and issue DMA at the same time, so the matrix
// pipe idles ~1,000 cycles per step, and a DMA burst stalls the issuing wave.
// Here each of the 8 waves owns 32 output channels x all 256 pixels of the
// 16 x 16 tile:
//  * its weight fragments (2 channel tiles x 2 K-halves, 16 B per lane each)
//    are read from global memory (L2) straight into VGPRs, one K-step ahead,
//    with a counted wait -- no LDS, no barrier, no redundancy (the waves own
//    disjoint channels);
//  * the pixel operand is the 18 x 18 input patch of a 64-channel chunk in LDS
//    (variant 30's column-keyed swizzle: a fragment is a lane constant + an
//    immediate row offset), DMA'd during the previous chunk, one piece per
//    wave per tap;
//  * so the only barrier is per chunk (every 9 K-steps): within a chunk the
//    two waves of a SIMD drift freely and one's fragment reads overlap the
//    other's MFMAs.
//  * a chunk's 9 steps are unrolled (weight set, ky, kx and the step's piece
//    are constants of the code) and carry no branch: the weights alternate
//    between two register sets, a piece's lane constants come from a table
//    built once per launch, and a piece the chunk lacks is masked, not skipped.
// Per K-step and wave: 4 x 16-B weight loads, 32 ds_read_b128 (LDS ~50 % busy
// at the MFMA rate), 64 MFMA 16x16x32.  Accumulators 128 VGPRs (2 x 16 tiles).
// Epilogue: register-only (bias, ReLU, bf16, 8-B stores) or the fused average
// pool (a wave holds all 256 pixels of its channels: no cross-wave reduction).
//
// BC = 128 (layer2's 128-channel stride-1 convs): the 8 waves are 4 channel
// groups x 2 pixel halves (rows 0-7 / 8-15 of the tile), so a wave keeps the
// same 2 MFMAs per fragment read and the same weight-load count per K-step;
// the two pixel halves of a channel group load the same weights (from L2).
#include "common.hpp"
#include "igemm.hpp"
#include "kernels.hpp"
#include "rwconv.hpp"

namespace sad {

namespace h31 {
constexpr int NW = 8, TC = 2;           // waves; per wave 2 x 16 channels
constexpr int TW = 16, TH = 16, PW = TW + 2, PR = PW * (TH + 2);
constexpr int NDP = (PR + 7) / 8;       // 41 pieces per conv chunk
constexpr int SCR = PW * TH;            // shortcut chunk: slots ty * 18 + tx
constexpr int NDS = SCR / 8;            // 36 pieces per shortcut chunk
constexpr int PATCH = NDP * 1024;
constexpr int ROWB = PW * 128;
constexpr int NKT = (NDP + NW - 1) / NW + (NDS + NW - 1) / NW;  // table entries per wave: conv and shortcut pieces
constexpr int SMEM = 2 * PATCH + NW * NKT * 256 + 1024;        // two patch buffers, the waves' piece tables, a dummy piece
constexpr int BAD = 0x7FFFFFF0;
constexpr uint64_t KEY = 0xd92dad912240ull;  // variant 30's column key {0,0,1,1,2,2,4,4,5,5,6,6,2,2,6,6,0,0}
static_assert(SMEM <= 160 * 1024, "LDS budget");
}  // namespace h31

__device__ __forceinline__ int h31_key(int px) { return (int)((h31::KEY >> (3 * px)) & 7); }

typedef unsigned int h31_v4 __attribute__((ext_vector_type(4)));
typedef __bf16 h31_bf2 __attribute__((ext_vector_type(2)));
typedef float h31_f2 __attribute__((ext_vector_type(2)));
// two floats -> packed bf16 pair (RNE): one v_cvt_pk_bf16_f32
template <typename E = u16>
__device__ __forceinline__ uint32_t h31_pk(float lo, float hi) {
  if constexpr (is_f16_v<E>) return pk_f16(lo, hi);  // v_cvt_pk_f16_f32, saturating
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((h31_f2){lo, hi}, h31_bf2));
}
// ReLU of a packed bf16 pair: as int16, negative bf16 values (and -0) are
// negative, so max(x, 0) per half is relu (= relu before the rounding)
__device__ __forceinline__ uint32_t h31_relu2(uint32_t x) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(x));
  return r;
}

// BC channels per workgroup (256 or 128): NCG channel groups of 32 x NPG pixel
// groups of TP tile rows.
// X3: split-bf16 parity mode (block.hip's layout: a 128-B chunk holds 32 logical
// channels, bytes 0-63 hi = bf16(v), 64-127 lo = bf16(v - hi), for pixels and
// weights alike).  A K-step's two halves then run W_hi.X_hi + W_lo.X_hi (half 0,
// both weight halves on the hi fragment) + W_hi.X_lo (half 1): 96 MFMAs per
// K-step and wave on the same operand reads and weight loads as bf16's 64; the
// epilogue splits the fp32 result into hi / lo again.
// RES (bf16): the epilogue adds a residual tensor (a BasicBlock's identity
// shortcut: x is added in fp32 to the accumulators the wave already holds,
// out = bf16(relu(acc + x)), the pooled form sums relu(acc + x)) -- its own
// instantiations, so the launches without a residual do not carry its loads.
// E = f16 (SAD_F16): fp16 tensors -- the f16 MFMA, v_cvt_pk_f16_f32 with
// saturation in the stores, v_cvt_f32_f16 for the residual's halves.
template <int BC, bool POOL, bool X3 = false, bool RES = false, typename E = u16>
__global__ __launch_bounds__(512, 1) void halo256r_kernel(BlockConvArgs a) {
  static_assert(!is_f16_v<E> || !X3, "fp16 has no split form");
  f16_kernel_entry<E>();
  using namespace h31;
  constexpr int NCG = BC / 32, NPG = NW / NCG, TP = 16 / NPG;
  static_assert(NCG * NPG == NW && (!POOL || NPG == 1), "wave split");
  static_assert(!(RES && X3), "the epilogue residual is bf16 only");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int n_tc = a.Cout / BC;
  const int w = xcd_remap(blockIdx.x, gridDim.x);
  const int tc = w % n_tc;  // both channel tiles of a pixel range share an XCD
  const int gp = gridDim.x / n_tc, wi = w / n_tc;
  const int tiles_x = a.W / TW, tiles_img = tiles_x * (a.H / TH);
  const int tiles_p = a.N * tiles_img;
  const int tp_begin = (int)((int64_t)wi * tiles_p / gp), tp_end = (int)((int64_t)(wi + 1) * tiles_p / gp);
  const int c0 = tc * BC;
  if (tp_begin >= tp_end) return;  // whole workgroup (uniform)
  const int cgrp = wave % NCG, pgrp = wave / NCG;
  const int cw = c0 + cgrp * 16 * TC;  // this wave's first output channel
  const int r0w = pgrp * TP;           // this wave's first tile row

  const int cinb = a.Cin * 2;
  const int nc0 = cinb / 128;                    // conv chunks (9 taps each)
  const int nk1 = a.in1 ? a.Cin1 * 2 / 128 : 0;  // shortcut chunks (1 step each)
  const int nch = nc0 + nk1;

  const __amdgpu_buffer_rsrc_t r0 =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.in0, (short)0, (int)a.in0_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t r1 =
      __builtin_amdgcn_make_buffer_rsrc((void*)(a.in1 ? a.in1 : a.in0), (short)0, (int)a.in1_bytes, 0x00020000);
  // (ablations 1 / 4: no record of the weights in range -- every weight load
  // returns zeros without traffic -- so the K loop carries no branch for them)
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.wt, (short)0, (a.ablate & 5) ? 0 : (int)a.wt_bytes, 0x00020000);
  const int ps0 = (int)a.in0_pstride * 2, ps1 = (int)a.in1_pstride * 2;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int lrow = lane >> 3;
  const int ab = a.ablate;  // timing ablations (wrong results): 1 no loads / DMA in the loop, 2 no patch DMA,
                            // 4 no weight loads, 8 no epilogue, 128 no epilogue stores

  // ---- weights: lane (fr, fg) of fragment (i, h) = row cw + i*16 + fr, K bytes
  // kb + h*64 + fg*16 of the step (kb = tap * cinb + chunk * 128); the wave-
  // uniform part kb + i*16 rows rides in the load's SGPR offset, h*64 in its
  // immediate: one lane offset serves the four loads
  const int wrow = a.wt_ld * 2;
  const int wlane = (cw + fr) * wrow + fg * 16;
  auto load_w = [&](int kb, h31_v4 (&wv)[TC][2]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        wv[i][h] = __builtin_amdgcn_raw_buffer_load_b128(rw, wlane + h * 64,
                                                         __builtin_amdgcn_readfirstlane(kb + i * 16 * wrow), 0);
  };
  auto kb_of = [&](int c, int tap) __attribute__((always_inline)) {
    return c < nc0 ? tap * cinb + c * 128 : 9 * cinb + (c - nc0) * 128;
  };

  // ---- patch pieces: piece q = wave + 8k of a chunk covers patch slots 8q ..
  // 8q + 7, a lane's slot is s = 8q + lane / 8.  What a lane needs of slot s
  // never changes during a launch, so it is tabled here, once (l1block.hip's
  // DREL), for the wave's 6 conv pieces (k = 5: wave 0 only) and 5 shortcut
  // pieces.  An entry: bits 4-29 the source offset relative to the tile's
  // first patch pixel with the swizzled chunk position folded in (a multiple of
  // 16); bits 0-3 the patch edges the slot lies on -- first / last patch row,
  // first / last patch column: a slot on an edge that the tile shares with the
  // image loads zeros; bit 30 always set; bit 31 a slot that no pixel has (past
  // the patch; a shortcut chunk's columns 16 / 17).  A piece is bad (zeros, no
  // traffic) where entry & mask is non-zero: the mask (NextP) is the tile's edge
  // bits | bit 31, or all ones for a piece that the chunk does not have, which
  // then goes to a dummy KB of LDS -- no branch, no division in a K-step.
  // The table lies in LDS behind the patch buffers (256 B per wave and piece;
  // held in 11 VGPRs it made the compiler spill): a step reads the entry of
  // the next step's piece, so the read's latency hides behind the step.
  constexpr int NKC = (NDP + NW - 1) / NW, NKS = (NDS + NW - 1) / NW;
  static_assert(NKC + NKS == NKT, "table entries per wave");
  int* const tab = (int*)(smem + 2 * PATCH) + wave * (NKT * 64) + lane;  // conv entry k at tab[64 k], shortcut at tab[64 (NKC + k)]
#pragma unroll
  for (int k = 0; k < NKC; ++k) {
    const int s = 8 * (wave + NW * k) + lrow, py = s / PW, px = s - py * PW;
    const int edge = (py == 0 ? 1 : 0) | (py == TH + 1 ? 2 : 0) | (px == 0 ? 4 : 0) | (px == TW + 1 ? 8 : 0);
    const int off = (py * a.W + px) * ps0 + (((lane & 7) ^ h31_key(px)) << 4);
    tab[64 * k] = s < PR ? (off & 0x3FFFFFF0) | edge | (1 << 30) : (int)0xC0000000;
  }
#pragma unroll
  for (int k = 0; k < NKS; ++k) {
    const int s = 8 * (wave + NW * k) + lrow, ty = s / PW, tx = s - ty * PW;
    const int off = (ty * a.W1 + tx) * (a.ss1 * ps1) + (((lane & 7) ^ h31_key(tx)) << 4);
    tab[64 * (NKC + k)] = tx < TW ? (off & 0x3FFFFFF0) | (1 << 30) : (int)0xC0000000;
  }
  // the wave-uniform part of a chunk's pieces (chunk c of tile t), decoded once
  // per chunk: source, base offset, mask, piece count (0 past the workgroup's
  // last tile, and in the loop under the ablations 1 / 2), table offset
  struct NextP {
    __amdgpu_buffer_rsrc_t r;
    int base, mask, lim, tk;
  };
  auto next_p = [&](int t, int c, int abm) __attribute__((always_inline)) {
    const int tt = __builtin_amdgcn_readfirstlane(t);
    const int b = tt / tiles_img, rem = tt - b * tiles_img;
    const int ty = rem / tiles_x;
    const int oy0 = ty * TH, ox0 = (rem - ty * tiles_x) * TW;
    const bool sc = c >= nc0;
    const int base = sc ? ((b * a.H1 + oy0 * a.ss1) * a.W1 + ox0 * a.ss1) * ps1 + (c - nc0) * 128
                        : ((b * a.H + oy0 - 1) * a.W + ox0 - 1) * ps0 + c * 128;
    const int mask = (int)0x80000000 | (sc ? 0
                                           : (oy0 == 0 ? 1 : 0) | (oy0 + TH == a.H ? 2 : 0) | (ox0 == 0 ? 4 : 0) |
                                                 (ox0 + TW == a.W ? 8 : 0));
    return NextP{sc ? r1 : r0, base, mask, tt < tp_end && !(ab & abm) ? (sc ? NDS : NDP) : 0, sc ? 64 * NKC : 0};
  };
  // the table entry of piece k of the chunk np describes (a shortcut chunk has
  // no k = 5: the read then lands on the next wave's table or the dummy piece,
  // inside the allocation, and the piece is masked whatever it returns)
  auto entry = [&](const NextP& np, int k) __attribute__((always_inline)) { return tab[np.tk + 64 * k]; };
  // piece k of this wave into the buffer at LDS offset boff (e: its table entry)
  auto piece = [&](const NextP& np, int boff, int k, int e) __attribute__((always_inline)) {
    const int q = wave + NW * k;
    const bool has = q < np.lim;  // uniform
    const int m = has ? np.mask : -1;
    dma16_m0(np.r, (e & m) ? BAD : np.base + (e & 0x3FFFFFF0), lds0 + (has ? boff + q * 1024 : SMEM - 1024));
  };
  auto pieces = [&](const NextP& np, int boff) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < NKC; ++k) piece(np, boff, k, entry(np, k));
  };

  // ---- prologue loads: the first chunk's patch, step 0's weights, the bias of
  // this lane's channels (every tile's accumulators start at the bias: the
  // epilogue adds nothing)
  pieces(next_p(tp_begin, 0, 0), 0);
  f32x4 biasv[TC];
#pragma unroll
  for (int i = 0; i < TC; ++i) biasv[i] = *(const f32x4*)(a.bias + cw + i * 16 + fg * 4);
  // two weight sets used in turn: step s of a chunk multiplies from set s & 1
  // while set (s + 1) & 1 is loaded for the next one -- no copies between the
  // steps of a chunk.  A chunk has an odd number of steps (9, a shortcut chunk
  // 1), so its last step leaves the next chunk's first weights in set 1: they
  // move to set 0 once per chunk, behind the chunk's wait.  (One chunk body per
  // set parity instead costs no move, but the compiler then no longer keeps the
  // accumulators and the sets in place across the bodies: 200-580 VGPRs
  // spilled in every instantiation.)  The loads are compiler-tracked buffer
  // loads, so the compiler waits for a set before the step's first MFMA; the
  // patch DMA pieces (inline asm) are not tracked, and being older than the
  // loads that follow them, each such wait also covers the pieces issued before
  // it -- conservative, never short.  An inline-asm load with a hand-counted
  // vmcnt gave wrong results: the register allocator may copy an asm output
  // before the data has landed.
  h31_v4 wset[2][TC][2];
  load_w(0, wset[1]);

  f32x4 acc[TC][TP];
#pragma unroll
  for (int i = 0; i < TC; ++i)
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = biasv[i];

  // the lane's fragment offsets for tap column kx and K-half h: patch column
  // kx + fr, chunk (4 h + fg) at its key position, plus this wave's first row;
  // a step adds the buffer's offset and immediates (ky, the fragment's row)
  int fb[3][2];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int h = 0; h < 2; ++h)
      fb[kx][h] = r0w * ROWB + (kx + fr) * 128 + (((4 * h + fg) ^ h31_key(kx + fr)) << 4);

  // ---- one K-step: 64 MFMAs from weight set wv; the pixel fragment of output
  // row j, half h is at patch row j + KY, column KX + fr of the buffer at LDS
  // offset boff (shortcut chunks: KY = KX = 0)
  auto step = [&](int boff, auto kyc, auto kxc, const h31_v4 (&wv)[TC][2]) __attribute__((always_inline)) {
    constexpr int KY = decltype(kyc)::value, KX = decltype(kxc)::value;
    auto half = [&](auto hc) __attribute__((always_inline)) {
      constexpr int h = decltype(hc)::value;
      // bf16: W_h.X_h.  Split-bf16, half 0 (the hi fragment): W_hi.X_hi and
      // W_lo.X_hi; half 1 (the lo fragment): W_hi.X_lo.
      constexpr int NM = X3 && h == 0 ? 2 : 1;  // weight halves per fragment
      // one add per half, opaque, or the compiler keeps the sums in registers
      unsigned po;
      asm volatile("v_add_u32 %0, %1, %2" : "=v"(po) : "s"(lds0 + boff), "v"(fb[KX][h]));
      const auto* pb = (const __attribute__((address_space(3))) char*)(uintptr_t)po + KY * ROWB;
      uint4 bf[TP];
#pragma unroll
      for (int j = 0; j < TP; ++j) bf[j] = __builtin_bit_cast(uint4, *(const __attribute__((address_space(3))) h31_v4*)(pb + j * ROWB));
#pragma unroll
      for (int j = 0; j < TP; ++j)
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
          for (int i = 0; i < TC; ++i)
            mfma_chunk<E>(__builtin_bit_cast(uint4, wv[i][X3 ? m : h]), bf[j], acc[i][j]);
      // reads run 4 fragments ahead of the MFMAs that consume them
      __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
      for (int j = 0; j < TP - 4; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, NM * TC, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x008, 4 * NM * TC, 0);
    };
    half(std::integral_constant<int, 0>{});
    half(std::integral_constant<int, 1>{});
  };

  auto epilogue = [&](int t) __attribute__((always_inline)) {
    int el;  // opaque lane id: the store addresses' lane parts are not kept in registers across the K loop
    asm volatile("v_mov_b32 %0, %1" : "=v"(el) : "v"(lane));
    const int fr = el & 15, fg = el >> 4;
    const int b = t / tiles_img, rem = t - b * tiles_img;
    const int oy0 = (rem / tiles_x) * TH, ox0 = (rem - (rem / tiles_x) * tiles_x) * TW;
    // RES: tile rows j, j + 1 of a 16-channel group are ONE 16-B load in the
    // store layout below (lane rows 0/2: 8 channels of pixel row j, rows 1/3:
    // of row j + 1), un-swapped into the accumulator layout by the stores' own
    // v_permlane16_swap (it is its own inverse).  The tile's pixel and the
    // wave's channels ride in the load's SGPR offset, the channel group in its
    // immediate.  RB tile rows per batch, two register sets: batch k + 1 is in
    // flight while batch k is added (and, unpooled, stored).
    constexpr int RB = 4;
    h31_v4 rv[2][RB / 2][TC];
    [[maybe_unused]] auto res_load = [&](int jb, h31_v4 (&v)[RB / 2][TC]) __attribute__((always_inline)) {
      const __amdgpu_buffer_rsrc_t rr =
          __builtin_amdgcn_make_buffer_rsrc((void*)a.res, (short)0, (int)a.res_bytes, 0x00020000);
      const int rps = (int)a.res_pstride * 2;
      const int rlane = ((fg & 1) * a.W + fr) * rps + (fg >> 1) * 16;
#pragma unroll
      for (int jj = 0; jj < RB / 2; ++jj) {
        const int so = __builtin_amdgcn_readfirstlane(((b * a.H + oy0 + r0w + jb + 2 * jj) * a.W + ox0) * rps + cw * 2);
#pragma unroll
        for (int i = 0; i < TC; ++i) v[jj][i] = __builtin_amdgcn_raw_buffer_load_b128(rr, rlane + i * 32, so, 0);
      }
    };
    [[maybe_unused]] auto res_add = [&](int jb, const h31_v4 (&v)[RB / 2][TC]) __attribute__((always_inline)) {
#pragma unroll
      for (int jj = 0; jj < RB / 2; ++jj)
#pragma unroll
        for (int i = 0; i < TC; ++i) {
          uint32_t q[4] = {v[jj][i][0], v[jj][i][1], v[jj][i][2], v[jj][i][3]};
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const auto r = __builtin_amdgcn_permlane16_swap(q[e], q[e + 2], false, false);
            q[e] = r[0];
            q[e + 2] = r[1];
          }
          // q[0..1]: this lane's 4 channels of row j, q[2..3]: of row j + 1
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            f32x4& c = acc[i][jb + 2 * jj + (e >> 1)];
            c[2 * (e & 1)] += lo16<E>(q[e]);
            c[2 * (e & 1) + 1] += hi16<E>(q[e]);
          }
        }
    };
    // batch jb: the next batch's loads first, then this batch's adds
    [[maybe_unused]] auto res_batch = [&](int jb) __attribute__((always_inline)) {
      if (jb + RB < TP) res_load(jb + RB, rv[(jb / RB + 1) & 1]);
      res_add(jb, rv[(jb / RB) & 1]);
    };
    if constexpr (RES) res_load(0, rv[0]);
    if constexpr (POOL) {
      if constexpr (RES) {
#pragma unroll
        for (int jb = 0; jb < TP; jb += RB) res_batch(jb);
      }
      // the wave holds all 256 pixels of its channels: relu(acc) (the bias is
      // in acc) summed over its 16 row fragments, then over the 16 lanes of a
      // row (DPP)
#pragma unroll
      for (int i = 0; i < TC; ++i) {
        float ps[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = 0.f;
#pragma unroll
          for (int j = 0; j < TP; ++j) v += fmaxf(acc[i][j][r], 0.f);
          ps[r] = row16_sum(v);
        }
        if (fr == 0)
          *(float4*)(a.pool_out + (int64_t)b * a.Cout + cw + i * 16 + fg * 4) =
              make_float4(ps[0] * (1.f / 256), ps[1] * (1.f / 256), ps[2] * (1.f / 256), ps[3] * (1.f / 256));
      }
    } else {
      // 16-B stores (the store tail is issue-bound): for fragment rows j, j+1
      // one v_permlane16_swap per dword pairs lane row fg's 4 channels with its
      // neighbour row's, so lane rows 0/2 hold 8 channels of pixel row j and
      // rows 1/3 of row j + 1 (cdna_hip_programming.md T21, 16-lane form)
      u16* __restrict__ out = (u16*)a.out;
#pragma unroll
      for (int j = 0; j < TP; j += 2) {
        if constexpr (RES) {
          if (j % RB == 0) res_batch(j);
        }
        const int64_t px = (int64_t)(b * a.H + oy0 + r0w + j + (fg & 1)) * a.W + ox0 + fr;
#pragma unroll
        for (int i = 0; i < TC; ++i) {
          if constexpr (X3) {
            // ReLU in fp32, then hi = bf16(v), lo = bf16(v - hi) (block.hip's
            // split); hi and lo go to the two 32-channel halves of the wave's
            // 128-B output chunk (cw is a multiple of 32)
            float v[2][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              v[0][r] = a.relu ? fmaxf(acc[i][j][r], 0.f) : acc[i][j][r];
              v[1][r] = a.relu ? fmaxf(acc[i][j + 1][r], 0.f) : acc[i][j + 1][r];
            }
            uint32_t qh[4], ql[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float x0 = v[e >> 1][2 * (e & 1)], x1 = v[e >> 1][2 * (e & 1) + 1];
              qh[e] = h31_pk(x0, x1);
              ql[e] = h31_pk(x0 - __uint_as_float(qh[e] << 16), x1 - __uint_as_float(qh[e] & 0xFFFF0000u));
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              const auto rh = __builtin_amdgcn_permlane16_swap(qh[e], qh[e + 2], false, false);
              qh[e] = rh[0];
              qh[e + 2] = rh[1];
              const auto rl = __builtin_amdgcn_permlane16_swap(ql[e], ql[e + 2], false, false);
              ql[e] = rl[0];
              ql[e + 2] = rl[1];
            }
            u16* op = out + px * a.out_pstride + 2 * cw + i * 16 + (fg >> 1) * 8;
            *(uint4*)op = make_uint4(qh[0], qh[1], qh[2], qh[3]);
            *(uint4*)(op + 32) = make_uint4(ql[0], ql[1], ql[2], ql[3]);
            continue;
          }
          const int co = cw + i * 16 + (fg >> 1) * 8;
          uint32_t q[4] = {h31_pk<E>(acc[i][j][0], acc[i][j][1]), h31_pk<E>(acc[i][j][2], acc[i][j][3]),
                           h31_pk<E>(acc[i][j + 1][0], acc[i][j + 1][1]), h31_pk<E>(acc[i][j + 1][2], acc[i][j + 1][3])};
          if (a.relu)
#pragma unroll
            for (int e = 0; e < 4; ++e) q[e] = h31_relu2(q[e]);
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const auto r = __builtin_amdgcn_permlane16_swap(q[e], q[e + 2], false, false);
            q[e] = r[0];
            q[e + 2] = r[1];
          }
          if (ab & 128) {  // timing: conversion + permutes kept, no store
            asm volatile("" ::"v"(q[0]), "v"(q[1]), "v"(q[2]), "v"(q[3]));
          } else {
            *(uint4*)(out + px * a.out_pstride + co) = make_uint4(q[0], q[1], q[2], q[3]);
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
      for (int j = 0; j < TP; ++j) acc[i][j] = biasv[i];
  };

  // ---- the K loop: tiles -> chunks -> steps, the steps of a chunk unrolled:
  // weight set, ky, kx and the step's piece are constants of the code.  Per
  // chunk: the wait and the barrier that publish its patch (and free the other
  // buffer), the weight set's move.  Per step: the next step's weights into the
  // other set (after the chunk's last step the next chunk's first; after a
  // tile's last a harmless reload of step 0's, so the wait counts stay
  // uniform), this step's patch piece for the next chunk (conv taps 1..6: one
  // piece per wave; a shortcut chunk: all of them), and the MFMAs.  A shortcut
  // chunk is the conv chunk's step 0 (ky = kx = 0) and leaves after it.
  int pbuf = 0;  // chunk counter & 1: the chunk's patch buffer
  bool post_epi = false;
  for (int t = tp_begin; t < tp_end; ++t) {
    for (int c = 0; c < nch; ++c) {
      const bool sc = c >= nc0;
      const int nt = c + 1 < nch ? t : t + 1, ncn = c + 1 < nch ? c + 1 : 0;  // next chunk
      const NextP np = next_p(nt, ncn, 3);
      const int kbn0 = kb_of(ncn, 0);
      const int boff = pbuf * PATCH, nboff = PATCH - boff;
      // the chunk's patch pieces (this wave's); after a tile's epilogue its
      // stores (the youngest operations) may stay in flight
      if (post_epi)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(POOL ? 0 : (X3 ? 2 : 1) * TC * TP / 2) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      post_epi = false;
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");  // LDS changed behind the barrier
#pragma unroll
      for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) wset[0][i][h] = wset[1][i][h];
      load_w(sc ? kbn0 : cinb + c * 128, wset[1]);
      if (sc) pieces(np, nboff);  // waited for at the next step (a chunk start)
      int trel = entry(np, 0);  // the table entry of the next step's piece
      __builtin_amdgcn_sched_barrier(0);
      step(boff, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, wset[0]);
      if (!sc)
        l1b_for<8>([&](auto tc1) __attribute__((always_inline)) {
          constexpr int tap = decltype(tc1)::value + 1;
          __builtin_amdgcn_sched_barrier(0);  // nothing moves between steps
          load_w(tap < 8 ? (tap + 1) * cinb + c * 128 : kbn0, wset[(tap + 1) & 1]);
          if constexpr (tap <= NKC) piece(np, nboff, tap - 1, trel);
          if constexpr (tap < NKC) trel = entry(np, tap);
          __builtin_amdgcn_sched_barrier(0);
          step(boff, std::integral_constant<int, tap / 3>{}, std::integral_constant<int, tap % 3>{}, wset[tap & 1]);
        });
      pbuf ^= 1;
    }
    if (!(ab & 8)) epilogue(t);
    post_epi = true;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int BC, bool POOL, bool X3, bool RES = false, typename E = u16>
static int launch_halo256r_t(const BlockConvArgs& a, hipStream_t s) {
  using namespace h31;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)halo256r_kernel<BC, POOL, X3, RES, E>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
    attr = true;
  }
  const int n_tc = a.Cout / BC;
  const int64_t tiles_p = (int64_t)a.N * (a.H / TH) * (a.W / TW);
  int64_t g = std::min<int64_t>(tiles_p * n_tc, 256);
  g = std::max<int64_t>(n_tc, g / n_tc * n_tc);
  hipLaunchKernelGGL((halo256r_kernel<BC, POOL, X3, RES, E>), dim3((unsigned)g), dim3(512), SMEM, s, a);
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

// (a: the kernel's bf16 channel counts and strides, as launch_block_conv passes
// them; x3: the split-bf16 layout, Cin / Cin1 / strides / wt_ld already doubled,
// Cout and the bias logical)
int launch_halo256r(const BlockConvArgs& a, hipStream_t s, bool x3, bool h16) {
  SAD_REQUIRE(!(x3 && h16), "variant 31: fp16 has no split form");
  SAD_REQUIRE(a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1, "variant 31: 3x3, stride 1, pad 1");
  SAD_REQUIRE(!a.st_part, "variant 31: no fused statistics");
  SAD_REQUIRE(!a.res || (!x3 && !a.in1),
              "variant 31: the epilogue residual is bf16 only and excludes a shortcut source (split-bf16: shortcut as in1)");
  SAD_REQUIRE(!a.res || (a.res_pstride >= a.Cout && a.res_pstride % 8 == 0 && ((uintptr_t)a.res & 15) == 0 &&
                         a.res_bytes == ((a.M - 1) * a.res_pstride + a.Cout) * 2 && a.res_bytes < (1ll << 31) - 65536),
              "variant 31: residual [M, res_pstride] bf16, 16-B aligned pixels, within the 2 GiB buffer range");
  SAD_REQUIRE(a.Cout % 128 == 0, "variant 31: Cout must be a multiple of 128");
  SAD_REQUIRE(a.H % 16 == 0 && a.W % 16 == 0 && a.Ho == a.H && a.Wo == a.W, "variant 31: image must tile by 16 x 16");
  SAD_REQUIRE((a.Cin * 2) % 128 == 0 && (!a.in1 || (a.Cin1 * 2) % 128 == 0), "variant 31: whole 128-B chunks");
  SAD_REQUIRE(!a.in1 || ((a.Ho - 1) * a.ss1 < a.H1 && (a.Wo - 1) * a.ss1 < a.W1), "variant 31: shortcut source");
  SAD_REQUIRE(a.wt_ld >= 9 * a.Cin + (a.in1 ? a.Cin1 : 0) && (a.wt_ld * 2) % 16 == 0, "variant 31: weight rows");
  SAD_REQUIRE(a.out_pstride % 8 == 0 && a.in0_pstride % 8 == 0 && (!a.in1 || a.in1_pstride % 8 == 0),
              "variant 31: pixel strides");
  SAD_REQUIRE(a.out || a.pool_out, "null output");
  SAD_REQUIRE(a.M == (int64_t)a.N * a.H * a.W, "variant 31: M = N H W");
  SAD_REQUIRE((int64_t)(18 * a.W + 18) * a.in0_pstride * 2 < (1 << 30) &&
                  (!a.in1 || (int64_t)(16 * a.W1 + 16) * a.ss1 * a.in1_pstride * 2 < (1 << 30)),
              "variant 31: a patch's source offsets must fit the piece table's 30 bits");
  if (h16) {  // bf16's instantiations, element type fp16
    if (a.pool_out) {
      SAD_REQUIRE(a.H == 16 && a.W == 16 && a.Cout % 256 == 0,
                  "variant 31 fused average pool: a 16 x 16 tile must be one image, Cout % 256");
      return a.res ? launch_halo256r_t<256, true, false, true, f16>(a, s)
                   : launch_halo256r_t<256, true, false, false, f16>(a, s);
    }
    if (a.res)
      return a.Cout % 256 == 0 ? launch_halo256r_t<256, false, false, true, f16>(a, s)
                               : launch_halo256r_t<128, false, false, true, f16>(a, s);
    return a.Cout % 256 == 0 ? launch_halo256r_t<256, false, false, false, f16>(a, s)
                             : launch_halo256r_t<128, false, false, false, f16>(a, s);
  }
  if (a.pool_out) {
    SAD_REQUIRE(a.H == 16 && a.W == 16 && a.Cout % 256 == 0,
                "variant 31 fused average pool: a 16 x 16 tile must be one image, Cout % 256");
    if (a.res) return launch_halo256r_t<256, true, false, true>(a, s);
    return x3 ? launch_halo256r_t<256, true, true>(a, s) : launch_halo256r_t<256, true, false>(a, s);
  }
  if (a.res)
    return a.Cout % 256 == 0 ? launch_halo256r_t<256, false, false, true>(a, s)
                             : launch_halo256r_t<128, false, false, true>(a, s);
  if (x3)
    return a.Cout % 256 == 0 ? launch_halo256r_t<256, false, true>(a, s) : launch_halo256r_t<128, false, true>(a, s);
  return a.Cout % 256 == 0 ? launch_halo256r_t<256, false, false>(a, s) : launch_halo256r_t<128, false, false>(a, s);
}

}  // namespace sad
