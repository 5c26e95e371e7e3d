// l2conv.hip -- variant 41: resident-weight, patch-resident 3x3 conv for
// Cin = Cout = 128, stride 1 (bf16, gfx950): layer2's second BasicBlock,
//   out = act(conv3x3(x; W) + b [+ res])
// (inference_runner.py:49-51 via timm resnet18 forward_features; conv1 ->
// bn1 -> act1 with res = 0, conv2 -> bn2 -> + identity -> act2 with res = the
// block input).
//
// The register-resident weight scheme of the fused layer1 block (variant 40,
// l1block.hip) fits one 128-channel conv exactly: a wave owning 32 output
// channels holds 32 x 1,152 K x 2 B / 64 lanes = 288 registers of weights
// (256 in AGPRs, read by inline-asm MFMAs; 32 in VGPRs).  4 waves, one per
// SIMD, each 32 channels x all 256 pixels of a 16 x 16 tile (2 x 16 MFMA
// fragments, 128 accumulator VGPRs starting at the bias); per K-step of 32
// channels a wave reads 16 pixel fragments from LDS and issues 32 MFMAs: no
// weight traffic and no weight ring.
//
// LDS: the 18 x 18 input patch of each 64-channel chunk (variant 30's column
// swizzle: fragment addresses are lane constants + immediates), double-
// buffered by chunk -- chunk 0 of a tile in buffer 0, chunk 1 in buffer 1, the
// next chunk's patch DMA'd while the current one is computed, one barrier per
// chunk -- plus, with a residual, the tile's 16 x 16 x 128 residual (DMA'd in
// chunk 0, read by the epilogue; 16-B chunks XOR-swizzled by pixel column so the
// epilogue's 8-B reads are conflict-free), the bias and the waves' patch-piece
// tables (11 KB, written once per launch).  157.5 KB.
// Epilogue: bias already in the accumulators, + residual, ReLU on packed bf16,
// 16-B stores (v_permlane16_swap pairs fragment rows j, j + 1).
//
// DS (layer2's first block, conv2 + downsample): the 1x1/2 downsample of the
// 64-channel block input is two more K-steps after the conv's 36 (its weights
// the 64 K columns behind the taps, 16 more VGPRs per wave), over a 16 x 16
// pixel patch of the input at stride 2 DMA'd to LDS during chunk 0 (16-B chunk
// c of pixel p at c ^ ((p >> 1) & 7): conflict-free fragment reads), its 32
// fragments read through a ring of 8.
//
// X3 (variant 42, round 4): the split-bf16 parity mode's layer1 convs, logical
// Cin = Cout = 64 = 128 bf16 input channels ([hi 32 | lo 32] x 2 chunks, the
// same 2 x 128-B chunks per pixel as the bf16 128-channel conv): the same 288
// resident weight registers per wave then hold 32 logical output channels'
// hi and lo weights, so the 4 waves are 2 channel groups x 2 pixel halves (8
// fragments each).  Per fragment and tap the hi fragment feeds W_hi.X_hi and
// W_lo.X_hi, the lo fragment W_hi.X_lo: 3 MFMAs per fragment read (bf16: 2).
// The identity residual (hi + lo, 256 B per pixel) has the 128-channel conv's
// LDS tile layout; the epilogue splits relu(acc + res) into hi / lo again.
#include "common.hpp"
#include "igemm.hpp"
#include "kernels.hpp"
#include "rwconv.hpp"

namespace sad {

namespace l2c {
constexpr int NW = 4;
constexpr int PW = 18, PR = PW * PW;           // 18 x 18 patch per 64-channel chunk
constexpr int NDP = (PR + 7) / 8;              // 41 DMA pieces of 8 pixel rows
constexpr int PATCH = NDP * 1024;
constexpr int ROWB = PW * 128;
constexpr int QP = (NDP + NW - 1) / NW;        // 11 pieces per wave per chunk
constexpr int RESB = 256 * 256;                // residual tile: 256 pixels x 128 ch bf16
constexpr int NRP = RESB / 1024 / NW;          // 16 residual pieces per wave
constexpr int NDS = 256 * 128 / 1024 / NW;     // 8 downsample pieces per wave
constexpr int OFF_RES = 2 * PATCH;
constexpr int SMEM_RES = OFF_RES + RESB;
constexpr int NS = 36;                         // K-steps: 2 chunks x 9 taps x 2 halves of 32 channels
constexpr int NSC = 18;                        // per chunk
constexpr int DQ = 4;                          // fragment reads in flight
constexpr int WV = 8;                          // K-steps of channel tile 1 whose weights sit in VGPRs
constexpr int BAD = 0x7FFFFFF0;
constexpr uint64_t KEY = 0xd92dad912240ull;    // variant 30's column key
// behind the buffers: the bias (512 B), then the waves' patch-piece tables
// [wave][piece k][lane] int, written once per launch
constexpr int TABB = NW * QP * 256;
constexpr int TAIL = 512 + TABB;
constexpr int ESH = 27;                        // a table entry's edge bits start here
static_assert(SMEM_RES + TAIL <= 160 * 1024, "LDS budget");
static_assert(PATCH % 128 == 0 && OFF_RES % 256 == 0, "buffer offsets commute with the chunk XORs");
}  // namespace l2c

__device__ __forceinline__ int l2c_key(int x) { return (int)((l2c::KEY >> (3 * x)) & 7); }

// ST (the trainer's raw conv, bf16 plain form): also the fused BN statistics,
// fp32 sums of the accumulators and their squares per channel, one row of
// a.st_part ([rows][2][128]) per workgroup
//
// With one wave per SIMD nothing hides behind a partner wave, so, as in
// l1block.hip, the tile loop keeps what is not the convolution out of its way:
// the timing ablations are a second kernel (AB); the tile origin is stepped; a
// patch piece is one table read, 4 VALU and the DMA; a residual / downsample
// piece is one lane constant plus a scalar; the fragment, store, residual and
// bias addresses are lane constants formed once per launch.
// E = f16 (SAD_F16): fp16 tensors in the bf16 inference forms -- the f16 MFMA,
// saturating v_cvt_pk_f16_f32 stores, v_cvt_f32_f16 for the residual's halves.
template <bool RES, bool DS, bool X3, bool ST, bool AB, typename E = u16>
__device__ __forceinline__ void l2conv_body(const BlockConvArgs& a) {
  static_assert(!is_f16_v<E> || (!X3 && !ST && !AB), "fp16: the plain inference forms");
  f16_kernel_entry<E>();
  static_assert(!(RES && DS) && !(X3 && DS), "one shortcut form");
  static_assert(!ST || (!RES && !DS && !X3), "statistics: the plain bf16 form");
  static_assert(!AB || (!X3 && !ST), "ablations: the bf16 forms");
  using namespace l2c;
  constexpr int TP = X3 ? 8 : 16;       // fragments (tile rows) per wave
  constexpr int UPT = 2 * TP;           // units per tap: (fragment, K-half)
  constexpr int NUC = 9 * UPT;          // units per chunk
  constexpr int PDIV = X3 ? 8 : 16;     // units between patch DMA pieces
  constexpr int DQ = X3 ? 8 : l2c::DQ;  // fragment reads in flight (X3: 143 VGPRs leave room)
  constexpr int OFF_B = RES || DS ? SMEM_RES : OFF_RES;  // the bias
  constexpr int OFF_T = OFF_B + 512;                     // the piece tables
  extern __shared__ __attribute__((aligned(256))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  // timing ablations (wrong results; tools/l2bench.py --ablate): 8 no output
  // stores, 32 no patch DMA in the tile loop
  const int ab = AB ? a.ablate : 0;
  // this wave's first output channel (logical) and first tile row
  const int cw = X3 ? (wave & 1) * 32 : wave * 32;
  const int r0w = X3 ? (wave >> 1) * 8 : 0;
  const int w = xcd_remap(blockIdx.x, gridDim.x);
  const int tiles_x = a.W / 16, tiles_img = tiles_x * (a.H / 16);
  const int tiles_p = a.N * tiles_img;
  const int tp_begin = (int)((int64_t)w * tiles_p / gridDim.x), tp_end = (int)((int64_t)(w + 1) * tiles_p / gridDim.x);
  if (tp_begin >= tp_end) {  // whole workgroup (uniform); its statistics row is zero
    if constexpr (ST) a.st_part[(int64_t)w * 256 + tid] = 0.f;
    return;
  }

  // the DMA sources' buffer descriptors (base, stride 0, num_records, raw
  // 32-bit data format) put together by hand and made opaque as one value each:
  // they stay in four aligned SGPRs for the launch
  l1b_v4 rx = {(unsigned)(uintptr_t)a.in0, (unsigned)((uintptr_t)a.in0 >> 32) & 0xFFFFu, (unsigned)a.in0_bytes, 0x00020000u};
  asm volatile("" : "+s"(rx));
  const void* const rrp = RES ? (const void*)a.res : (const void*)a.in1;
  l1b_v4 rr = {(unsigned)(uintptr_t)rrp, (unsigned)((uintptr_t)rrp >> 32) & 0xFFFFu,
               (unsigned)(RES ? a.res_bytes : a.in1_bytes), 0x00020000u};
  if constexpr (RES || DS) asm volatile("" : "+s"(rr));
  const __amdgpu_buffer_rsrc_t ro =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.out, (short)0, (int)a.out_bytes, 0x00020000);
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int ps = (int)a.in0_pstride * 2;   // bytes per input pixel
  const int pso = (int)a.out_pstride * 2;  // per output pixel
  // the shortcut source: bytes per tile pixel column and per tile pixel row
  // (RES: the residual; DS: the block input at stride ss1, H1 = ss1 H)
  const int pss = RES ? (int)a.res_pstride * 2 : DS ? a.ss1 * (int)a.in1_pstride * 2 : 0;
  const int srow = RES ? a.W * pss : DS ? a.ss1 * a.W1 * (int)a.in1_pstride * 2 : 0;
  const int orow = a.W * pso;

  // ---- tile origin (uniform): byte offsets of the tile's first pixel in the
  // input, the shortcut source and the output.  Tiles run along rows (tx
  // fastest).  Decoded by division once, for the workgroup's first tile; the
  // tile loop steps it: 16 pixels right, else down 16 rows to column 0 (images
  // are contiguous, so the first tile of the next image is the same step)
  struct TileO {
    int base, oy0, ox0, sbase, obase;
  };
  auto tile_o = [&](int t) __attribute__((always_inline)) {
    const int b = t / tiles_img, rem = t - b * tiles_img;
    const int ty = rem / tiles_x;
    TileO o;
    o.oy0 = ty * 16;
    o.ox0 = (rem - ty * tiles_x) * 16;
    o.base = ((b * a.H + o.oy0) * a.W + o.ox0) * ps;
    o.obase = ((b * a.H + o.oy0) * a.W + o.ox0) * pso;
    o.sbase = RES  ? ((b * a.H + o.oy0) * a.W + o.ox0) * pss
              : DS ? ((b * a.H1 + o.oy0 * a.ss1) * a.W1 + o.ox0 * a.ss1) * (int)(a.in1_pstride * 2)
                   : 0;
    return o;
  };
  const int wrap_i = 15 * a.W * ps, wrap_o = 15 * orow, wrap_s = 16 * srow - a.W * pss;
  auto tile_step = [&](const TileO& o) __attribute__((always_inline)) {
    TileO n;
    n.ox0 = o.ox0 + 16;
    n.oy0 = o.oy0;
    n.base = o.base + 16 * ps;
    n.obase = o.obase + 16 * pso;
    n.sbase = o.sbase + 16 * pss;
    if (n.ox0 == a.W) {
      n.ox0 = 0;
      n.oy0 += 16;
      n.base += wrap_i;
      n.obase += wrap_o;
      n.sbase += wrap_s;
      if (n.oy0 == a.H) n.oy0 = 0;
    }
    return n;
  };

  // ---- patch pieces: piece k of this wave is q = wave + 4k, patch slots 8q ..
  // 8q + 7; a lane's slot r = 8q + lane / 8 is patch pixel (Y, X) = (r / 18,
  // r % 18).  What a lane needs of its slot never changes during a launch and
  // is the same for both chunks, so it is tabled in LDS, once.  An entry: bits
  // 0-26 the source offset from the tile's first patch pixel (one row up, one
  // pixel left of its origin) with the swizzled chunk folded in, in 16-B units;
  // bit 27 "slot >= 324", bits 28-31 the patch edges the slot lies on -- row 0 /
  // row 17 / column 0 / column 17.  A slot past the patch, or on an edge that
  // the tile shares with the image, loads zeros (offset past num_records): the
  // tile's mask always holds bit 27.  (The shift by 4 that makes bytes of the
  // offset drops bits 28-31 and leaves bit 27 on top -- only where zeros are
  // selected anyway.)
  const int TA = (int)lds0 + OFF_T + (wave * (QP * 64) + lane) * 4;  // piece k at TA + 256 k
  auto piece_entry = [&](int k) __attribute__((always_inline)) {
    const int r = 8 * (wave + NW * k) + (lane >> 3);
    const int Y = (r * 3641) >> 16, X = r - PW * Y;  // r / 18 exactly for r < 330
    const int edge = (r >= PR ? 1 : 0) | (Y == 0 ? 2 : 0) | (Y == PW - 1 ? 4 : 0) | (X == 0 ? 8 : 0) | (X == PW - 1 ? 16 : 0);
    const unsigned off = (unsigned)((Y * a.W + X) * ps + (((lane & 7) ^ l2c_key(X)) << 4)) >> 4;
    return (int)(((unsigned)edge << ESH) | (off & ((1u << ESH) - 1)));
  };
  auto patch_base = [&](const TileO& o) __attribute__((always_inline)) { return o.base - (a.W + 1) * ps; };
  auto patch_mask = [&](const TileO& o) __attribute__((always_inline)) {
    return (int)((unsigned)(1 | (o.oy0 == 0 ? 2 : 0) | (o.oy0 + 16 == a.H ? 4 : 0) | (o.ox0 == 0 ? 8 : 0) |
                            (o.ox0 + 16 == a.W ? 16 : 0))
                 << ESH);
  };
  const unsigned dstw = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);  // this wave's piece 0 in buffer 0
  // piece k of chunk c (pbase: the tile's patch base + 128 c) with table entry
  // e into buffer c; branch-free but for k = QP - 1, which only wave 0 has
  auto issue_piece = [&](auto kc, auto cc, int e, int pbase, int pmask) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value, c = decltype(cc)::value;
    if constexpr (NW * k + NW - 1 >= NDP)
      if (wave + NW * k >= NDP) return;  // uniform
    l1b_dma16<c * PATCH + k * NW * 1024>(rx, (e & pmask) ? BAD : pbase + (int)((unsigned)e << 4), dstw);
  };
  // residual piece k (q = wave + 4k: pixels 4q..4q+3 of the tile, 256 B each,
  // 16-B chunk p of pixel px at position p ^ (px & 15)): tile row k, pixel
  // column 4 wave + lane / 16 -- the lane's part is the same for every k
  const int pxr = 4 * wave + (lane >> 4);
  const int RV = pxr * pss + (((lane & 15) ^ pxr) << 4);
  auto issue_res = [&](auto kc, const TileO& o) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    l1b_dma16<OFF_RES + k * NW * 1024>(rr, RV + (o.sbase + k * srow), dstw);
  };
  // downsample piece k (q = wave + 4k: pixels 8q..8q+7 of the tile, 128 B
  // each, source pixel (2 oy, 2 ox) of the 64-channel block input): tile row
  // 2k + wave / 2, pixel column 8 (wave & 1) + lane / 8, chunk position
  // p ^ ((px >> 1) & 7)
  const int pxd = 8 * (wave & 1) + (lane >> 3);
  const int DV = (wave >> 1) * srow + pxd * pss + (((lane & 7) ^ ((pxd >> 1) & 7)) << 4);
  auto issue_ds = [&](auto kc, const TileO& o) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    l1b_dma16<OFF_RES + k * NW * 1024>(rr, DV + (o.sbase + 2 * k * srow), dstw);
  };
  // the downsample's weights: K-steps h = 0, 1 (channels (fg + 4h)*8..+7)
  l1b_v4 wds[2][2];
  if constexpr (DS) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int h = 0; h < 2; ++h)
        wds[i][h] = *(const l1b_v4*)((const u16*)a.wt + (size_t)(cw + 16 * i + fr) * a.wt_ld + 9 * 128 + (fg + 4 * h) * 8);
  }

  // ---- weights into registers: K-step s = (chunk c, tap, half h) -> lane
  // (fr, fg) holds channels c*64 + (fg + 4h)*8 .. +7 of tap `tap` for output
  // channel cw + 16 i + fr
  l1b_v4 wr[2][NS];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int c = s / NSC, tap = (s % NSC) >> 1, h = s & 1;
      wr[i][s] = *(const l1b_v4*)((const u16*)a.wt + (size_t)(cw + 16 * i + fr) * a.wt_ld + tap * 128 + c * 64 +
                                  (fg + 4 * h) * 8);
    }
  // the bias (the accumulators' start value) behind the LDS buffers
  if (tid < (X3 ? 16 : 32)) *(float4*)(smem + OFF_B + 16 * tid) = *(const float4*)(a.bias + 4 * tid);
  TileO ocur = tile_o(tp_begin);
  l1b_for<QP>([&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    const int e = piece_entry(k);
    l1b_st<int>(TA + 256 * k, e);
    issue_piece(kc, std::integral_constant<int, 0>{}, e, patch_base(ocur), patch_mask(ocur));
  });

  // ---- lane constants of the tile loop, once per launch (LDS byte addresses
  // with the LDS base included; the XORs below stay inside a pixel's chunk
  // bits, and every buffer offset is a multiple of 128)
  // fragment reads -- tile row j, tap (ky, kx), K-half h of chunk c:
  // ((I2[kx] + c PATCH) ^ 64 h) + (j + ky) ROWB, the wave's first row folded in
  int I2[3];
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
    I2[kx] = (int)lds0 + r0w * ROWB + (fr + kx) * 128 + ((fg ^ l2c_key(fr + kx)) << 4);
  // the bias of channels cw + 16 i + 4 fg .. + 3 at BA + 64 i
  const int BA = (int)lds0 + OFF_B + (cw + fg * 4) * 4;
  // the lane's part of a store's offset: rows (j, j + 1) are paired, lane rows
  // 0/2 store pixel row j, 1/3 row j + 1; 8 channels (X3: of the hi half) from
  // cw + 16 i + 8 (fg / 2) (X3: split column 64 (cw / 32) + ...)
  const int OV = ((r0w + (fg & 1)) * a.W + fr) * pso + ((X3 ? 64 * (cw >> 5) : cw) + (fg >> 1) * 8) * 2;
  // the residual of channels cw + 16 i + 4 fg .. + 3 of pixel (row, fr): 16-B
  // chunk ch = cw / 8 + 2 i + fg / 2 at position ch ^ fr, 8-B half fg & 1: (RB ^
  // 32 i) + row * 4096 (cw / 8 + fg / 2 has bit 1 clear; X3: chunk 8 (cw / 32)
  // + 2 i + fg / 2 (hi), + 4 (lo, bit 2 clear: ^ 64))
  const int RB = (int)lds0 + OFF_RES + (r0w * 16 + fr) * 256 + ((((X3 ? 8 * (cw >> 5) : cw >> 3) + (fg >> 1)) ^ fr) << 4) +
                 (fg & 1) * 8;
  // the downsample patch's fragment of tile row j, K-half h: (DD ^ 64 h) + j * 2048
  const int DD = (int)lds0 + OFF_RES + fr * 128 + ((fg ^ ((fr >> 1) & 7)) << 4);
  // ReLU as a floor per packed bf16 half, decided here (ST: none)
  const int rl = a.relu ? 0 : (int)0x80008000u;
  const bool relu = a.relu;

  // the first patch has landed before the first barrier (the loop's chunk-0
  // wait lets 16 younger operations, the previous tile's stores, stay in
  // flight); the bias is visible after it
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  f32x4 acc[2][TP];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const f32x4 b0 = l1b_ld<f32x4>(BA + 64 * i);
#pragma unroll
    for (int j = 0; j < TP; ++j) acc[i][j] = b0;
  }

  // ST: per-lane partial sums of channels cw + 16 i + 4 fg + e over this
  // workgroup's pixels (column fr of every tile row), then across fr at the end
  float st_s[2][4] = {}, st_q[2][4] = {};
  for (int t = tp_begin; t < tp_end; ++t) {
    // the next tile (after the last one: this tile's again, into the free
    // buffer, which nothing reads -- no branch around the DMA)
    const TileO ostep = tile_step(ocur);
    const TileO onext = t + 1 < tp_end ? ostep : ocur;
    const TileO o = ocur;
    // the uniform part of the pieces issued in chunk 0 (this tile's chunk 1)
    // and in chunk 1 (the next tile's chunk 0)
    const int pb1 = patch_base(o) + 128, pm1 = patch_mask(o);
    const int pb0n = patch_base(onext), pm0n = patch_mask(onext);

    l1b_for<2>([&](auto cc) __attribute__((always_inline)) {
      constexpr int c = decltype(cc)::value;
      // the chunk's patch (this wave's pieces; the tile's stores, youngest, may
      // stay in flight) is published by the barrier
      if constexpr (c == 0)
        asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      int pe = l1b_ld<int>(TA);  // the table entry of the next piece, read one piece ahead
      // this chunk's buffer in the bases, so the immediates stay < 64 KB
      int I2c[3][2];
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        I2c[kx][0] = I2[kx] + c * PATCH;
        I2c[kx][1] = I2c[kx][0] ^ 64;
      }
      // unit u of the chunk: tap u / UPT; bf16: K-half h = (u % UPT) / 16,
      // fragment j = u % 16 (K-half-outer, as round 3); X3: fragment
      // j = (u % UPT) / 2, h = u % 2 (the hi fragment, then the lo one)
      auto rd = [&](auto uc) __attribute__((always_inline)) -> l1b_v4 {
        constexpr int u = decltype(uc)::value;
        constexpr int tap = u / UPT, ky = tap / 3, kx = tap % 3;
        constexpr int j = X3 ? (u % UPT) / 2 : u % 16, h = X3 ? u % 2 : (u % UPT) / 16;
        return l1b_ld<l1b_v4>(I2c[kx][h] + (j + ky) * ROWB);
      };
      l1b_v4 bq[DQ];
      l1b_for<DQ>([&](auto uc) __attribute__((always_inline)) { bq[decltype(uc)::value] = rd(uc); });
      l1b_for<NUC>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value;
        constexpr int tap = u / UPT;
        constexpr int j = X3 ? (u % UPT) / 2 : u % 16, h = X3 ? u % 2 : (u % UPT) / 16;
        constexpr int s = c * NSC + 2 * tap + h;   // this fragment's K-step (bf16; X3: its hi / lo weights)
        constexpr int s_hi = c * NSC + 2 * tap, s_lo = s_hi + 1;
        const l1b_v4 bf = bq[u % DQ];
        if constexpr (u + DQ < NUC) bq[u % DQ] = rd(std::integral_constant<int, u + DQ>{});
        // DMA: chunk 0 carries this tile's chunk-1 patch and residual; chunk 1
        // the next tile's chunk-0 patch
        if constexpr (u % PDIV == 0 && u / PDIV < QP) {
          constexpr int k = u / PDIV;
          if (!(ab & 32))
            issue_piece(std::integral_constant<int, k>{}, std::integral_constant<int, c ^ 1>{}, pe, c == 0 ? pb1 : pb0n,
                        c == 0 ? pm1 : pm0n);
          if constexpr (k + 1 < QP) pe = l1b_ld<int>(TA + 256 * (k + 1));
        }
        if constexpr (RES && c == 0 && u % PDIV == PDIV / 2 && u / PDIV < NRP)
          issue_res(std::integral_constant<int, u / PDIV>{}, o);
        if constexpr (DS && c == 0 && u % 32 == 8 && u / 32 < NDS) issue_ds(std::integral_constant<int, u / 32>{}, o);
        auto mm = [&](auto ic, auto sc) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value, ss = decltype(sc)::value;
          if constexpr (i == 1 && ss >= NS - WV)
            l1b_mfma_v<E>(acc[i][j], wr[i][ss], bf);
          else
            l1b_mfma_a<E>(acc[i][j], wr[i][ss], bf);
        };
        if constexpr (!X3) {
          mm(std::integral_constant<int, 0>{}, std::integral_constant<int, s>{});
          mm(std::integral_constant<int, 1>{}, std::integral_constant<int, s>{});
        } else if constexpr (u == NUC - 2) {
          // the chunk's last fragment (both its units) as ONE asm statement
          // ending in the 8-pass XDL result wait: hipcc does not pad for asm
          // MFMAs, and around the chunk end its register allocator moves
          // accumulators (v_mov) -- inside one statement it cannot, and after
          // it the results are complete (tools/asm_hazards.py audits this)
          const l1b_v4 xl = bq[(u + 1) % DQ];
          static_assert(j == TP - 1 && h == 0, "last fragment");
          if constexpr (s_hi >= NS - WV)
            asm volatile(
                "v_mfma_f32_16x16x32_bf16 %0, %2, %6, %0\n\t"
                "v_mfma_f32_16x16x32_bf16 %1, %3, %6, %1\n\t"
                "v_mfma_f32_16x16x32_bf16 %0, %4, %6, %0\n\t"
                "v_mfma_f32_16x16x32_bf16 %1, %5, %6, %1\n\t"
                "v_mfma_f32_16x16x32_bf16 %0, %2, %7, %0\n\t"
                "v_mfma_f32_16x16x32_bf16 %1, %3, %7, %1\n\t"
                "s_nop 11"
                : "+v"(acc[0][j]), "+v"(acc[1][j])
                : "a"(wr[0][s_hi]), "v"(wr[1][s_hi]), "a"(wr[0][s_lo]), "v"(wr[1][s_lo]), "v"(bf), "v"(xl));
          else
            asm volatile(
                "v_mfma_f32_16x16x32_bf16 %0, %2, %6, %0\n\t"
                "v_mfma_f32_16x16x32_bf16 %1, %3, %6, %1\n\t"
                "v_mfma_f32_16x16x32_bf16 %0, %4, %6, %0\n\t"
                "v_mfma_f32_16x16x32_bf16 %1, %5, %6, %1\n\t"
                "v_mfma_f32_16x16x32_bf16 %0, %2, %7, %0\n\t"
                "v_mfma_f32_16x16x32_bf16 %1, %3, %7, %1\n\t"
                "s_nop 11"
                : "+v"(acc[0][j]), "+v"(acc[1][j])
                : "a"(wr[0][s_hi]), "a"(wr[1][s_hi]), "a"(wr[0][s_lo]), "a"(wr[1][s_lo]), "v"(bf), "v"(xl));
        } else if constexpr (u == NUC - 1) {
          // (issued with the previous unit)
        } else if constexpr (h == 0) {  // the hi fragment: W_hi.X_hi, W_lo.X_hi
          mm(std::integral_constant<int, 0>{}, std::integral_constant<int, s_hi>{});
          mm(std::integral_constant<int, 1>{}, std::integral_constant<int, s_hi>{});
          mm(std::integral_constant<int, 0>{}, std::integral_constant<int, s_lo>{});
          mm(std::integral_constant<int, 1>{}, std::integral_constant<int, s_lo>{});
        } else {  // the lo fragment: W_hi.X_lo
          mm(std::integral_constant<int, 0>{}, std::integral_constant<int, s_hi>{});
          mm(std::integral_constant<int, 1>{}, std::integral_constant<int, s_hi>{});
        }
      });
    });
    if constexpr (DS) {
      // the downsample: 2 K-steps over the stride-2 input patch (published by
      // the chunk-1 barrier, whose wait covered its pieces)
      // unit u = (K-half h = u / 16, tile row j = u % 16), DQD reads in flight
      // (all 16 rows of a K-half at once would need 64 registers)
      constexpr int DQD = 8;
      const int DD1 = DD ^ 64;
      auto rdd = [&](auto uc) __attribute__((always_inline)) -> l1b_v4 {
        constexpr int u = decltype(uc)::value;
        return l1b_ld<l1b_v4>((u / 16 ? DD1 : DD) + (u % 16) * 16 * 128);
      };
      l1b_v4 bd[DQD];
      l1b_for<DQD>([&](auto uc) __attribute__((always_inline)) { bd[decltype(uc)::value] = rdd(uc); });
      l1b_for<32>([&](auto uc) __attribute__((always_inline)) {
        constexpr int u = decltype(uc)::value, h = u / 16, j = u % 16;
        const l1b_v4 bf = bd[u % DQD];
        if constexpr (u + DQD < 32) bd[u % DQD] = rdd(std::integral_constant<int, u + DQD>{});
        l1b_mfma_v<E>(acc[0][j], wds[0][h], bf);
        l1b_mfma_v<E>(acc[1][j], wds[1][h], bf);
      });
    }
    // asm MFMA results read by compiler code: 12 wait states (8-pass XDL)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 11" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    // the bias once per tile, for the accumulators' restart below
    f32x4 bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) bv[i] = l1b_ld<f32x4>(BA + 64 * i);

    // ---- epilogue: (+ residual) -> ReLU on packed bf16 -> 16-B stores: for
    // rows j, j + 1 one v_permlane16_swap per dword pairs lane row fg with its
    // neighbour row, so lane rows 0/2 hold 8 channels of pixel row j, 1/3 of j+1.
    // A store: the lane's OV (+ 32 i as the immediate), the rows' scalar offset
#pragma unroll
    for (int j = 0; j < TP; j += 2) {
      const int osj = o.obase + j * orow;  // uniform
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        f32x4 v0 = acc[i][j], v1 = acc[i][j + 1];
        const int rbi = i ? RB ^ 32 : RB;
        if constexpr (X3) {
          // residual hi + lo of logical channels cw + 16 i + 4 fg .. +3: split
          // columns 64 (cw / 32) + 16 i + 4 fg (hi) and + 32 (lo) -- 16-B chunk
          // ch (hi) / ch + 4 (lo), 8-B half fg & 1; then ReLU in fp32, hi =
          // bf16(v), lo = bf16(v - hi), 16-B stores of rows (j, j + 1) paired by
          // v_permlane16_swap
          if constexpr (RES) {
            const l1b_v2 h0 = l1b_ld<l1b_v2>(rbi + j * 4096);
            const l1b_v2 l0 = l1b_ld<l1b_v2>((rbi ^ 64) + j * 4096);
            const l1b_v2 h1 = l1b_ld<l1b_v2>(rbi + (j + 1) * 4096);
            const l1b_v2 l1 = l1b_ld<l1b_v2>((rbi ^ 64) + (j + 1) * 4096);
            v0[0] += __uint_as_float(h0.x << 16) + __uint_as_float(l0.x << 16);
            v0[1] += __uint_as_float(h0.x & 0xFFFF0000u) + __uint_as_float(l0.x & 0xFFFF0000u);
            v0[2] += __uint_as_float(h0.y << 16) + __uint_as_float(l0.y << 16);
            v0[3] += __uint_as_float(h0.y & 0xFFFF0000u) + __uint_as_float(l0.y & 0xFFFF0000u);
            v1[0] += __uint_as_float(h1.x << 16) + __uint_as_float(l1.x << 16);
            v1[1] += __uint_as_float(h1.x & 0xFFFF0000u) + __uint_as_float(l1.x & 0xFFFF0000u);
            v1[2] += __uint_as_float(h1.y << 16) + __uint_as_float(l1.y << 16);
            v1[3] += __uint_as_float(h1.y & 0xFFFF0000u) + __uint_as_float(l1.y & 0xFFFF0000u);
          }
          if (relu)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              v0[r] = fmaxf(v0[r], 0.f);
              v1[r] = fmaxf(v1[r], 0.f);
            }
          uint32_t qh[4] = {l1b_pk(v0[0], v0[1]), l1b_pk(v0[2], v0[3]), l1b_pk(v1[0], v1[1]), l1b_pk(v1[2], v1[3])};
          const float vv[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
          uint32_t ql[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            ql[e] = l1b_pk(vv[2 * e] - __uint_as_float(qh[e] << 16), vv[2 * e + 1] - __uint_as_float(qh[e] & 0xFFFF0000u));
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const auto rh = __builtin_amdgcn_permlane16_swap(qh[e], qh[e + 2], false, false);
            qh[e] = rh[0];
            qh[e + 2] = rh[1];
            const auto rl2 = __builtin_amdgcn_permlane16_swap(ql[e], ql[e + 2], false, false);
            ql[e] = rl2[0];
            ql[e + 2] = rl2[1];
          }
          __builtin_amdgcn_raw_buffer_store_b128((l1b_v4){qh[0], qh[1], qh[2], qh[3]}, ro, OV + 32 * i, osj, 0);
          __builtin_amdgcn_raw_buffer_store_b128((l1b_v4){ql[0], ql[1], ql[2], ql[3]}, ro, OV + 32 * i + 64, osj, 0);
          acc[i][j] = bv[i];
          acc[i][j + 1] = bv[i];
          continue;
        }
        if constexpr (RES) {
          // residual of channels cw + 16 i + 4 fg .. +3 of pixels (j, fr), (j + 1, fr)
          const l1b_v2 r0 = l1b_ld<l1b_v2>(rbi + j * 4096);
          const l1b_v2 r1 = l1b_ld<l1b_v2>(rbi + (j + 1) * 4096);
          v0[0] += lo16<E>(r0.x);
          v0[1] += hi16<E>(r0.x);
          v0[2] += lo16<E>(r0.y);
          v0[3] += hi16<E>(r0.y);
          v1[0] += lo16<E>(r1.x);
          v1[1] += hi16<E>(r1.x);
          v1[2] += lo16<E>(r1.y);
          v1[3] += hi16<E>(r1.y);
        }
        if constexpr (ST) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            st_s[i][e] += v0[e];
            st_s[i][e] += v1[e];
            st_q[i][e] = fmaf(v0[e], v0[e], st_q[i][e]);
            st_q[i][e] = fmaf(v1[e], v1[e], st_q[i][e]);
          }
        }
        uint32_t q[4] = {l1b_pk<E>(v0[0], v0[1]), l1b_pk<E>(v0[2], v0[3]), l1b_pk<E>(v1[0], v1[1]),
                         l1b_pk<E>(v1[2], v1[3])};
        if constexpr (!ST)  // (the statistics form is the raw conv: launch_l2conv requires !relu)
#pragma unroll
          for (int e = 0; e < 4; ++e) q[e] = l1b_relu2s(q[e], rl);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const auto r = __builtin_amdgcn_permlane16_swap(q[e], q[e + 2], false, false);
          q[e] = r[0];
          q[e + 2] = r[1];
        }
        if (!(ab & 8)) __builtin_amdgcn_raw_buffer_store_b128((l1b_v4){q[0], q[1], q[2], q[3]}, ro, OV + 32 * i, osj, 0);
        acc[i][j] = bv[i];
        acc[i][j + 1] = bv[i];
      }
    }
    ocur = ostep;
  }
  if constexpr (ST) {
    // across the 16 lanes (pixel columns) of each channel group, fixed order
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
          st_s[i][e] += __shfl_xor(st_s[i][e], off, 64);
          st_q[i][e] += __shfl_xor(st_q[i][e], off, 64);
        }
    if (fr == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = cw + 16 * i + 4 * fg + e;
          a.st_part[(int64_t)w * 256 + c] = st_s[i][e];
          a.st_part[(int64_t)w * 256 + 128 + c] = st_q[i][e];
        }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// the production kernels hold no ablation code; launch_l2conv picks the
// ablation twin (the bf16 inference forms only) when a.ablate != 0
template <bool RES, bool DS, bool X3 = false, bool ST = false, typename E = u16>
__global__ __launch_bounds__(256, 1) void l2conv_kernel(BlockConvArgs a) {
  l2conv_body<RES, DS, X3, ST, false, E>(a);
}
template <bool RES, bool DS>
__global__ __launch_bounds__(256, 1) void l2conv_ablate_kernel(BlockConvArgs a) {
  l2conv_body<RES, DS, false, false, true>(a);
}

// (x3: the split layout's bf16 channel counts / strides, as launch_block_conv
// passes them: Cin 128 = 64 logical, Cout and the bias logical 64)
int launch_l2conv(const BlockConvArgs& a, hipStream_t s, bool x3, bool h16) {
  using namespace l2c;
  SAD_REQUIRE(a.KH == 3 && a.KW == 3 && a.stride == 1 && a.pad == 1 && !a.pool_out,
              "variant 41/42: 3x3/s1/p1, no pool");
  SAD_REQUIRE(!h16 || (!x3 && !a.st_part && !a.ablate), "variant 41 in fp16: the plain inference forms");
  SAD_REQUIRE(!a.st_part || (!x3 && !a.in1 && !a.res && !a.relu && a.st_rows),
              "variant 41 statistics: the plain bf16 raw conv (no shortcut / residual / ReLU), st_rows set");
  if (x3) {
    SAD_REQUIRE(!a.in1 && a.Cin == 128 && a.Cout == 64 && a.H % 16 == 0 && a.W % 16 == 0 && a.Ho == a.H &&
                    a.Wo == a.W && a.wt_ld >= 9 * 128 && a.wt_ld % 8 == 0 && a.in0_pstride % 64 == 0 &&
                    a.in0_pstride >= 128 && a.out_pstride % 64 == 0 && a.out_pstride >= 128 &&
                    (!a.res || (a.res_pstride % 64 == 0 && a.res_pstride >= 128)) && a.out,
                "variant 42: split-bf16 64 -> 64 logical 3x3/s1/p1 (layer1), 16 x 16 tiles");
    const int64_t tiles = (int64_t)a.N * (a.H / 16) * (a.W / 16);
    if (tiles == 0) return SAD_OK;
    const int64_t g = std::min<int64_t>(tiles, 256);
    BlockConvArgs b = a;
    b.out_bytes = ((int64_t)a.N * a.H * a.W - 1) * a.out_pstride * 2 + 256;
    SAD_REQUIRE(b.out_bytes < (1ll << 31) - 65536, "variant 42: output passes the 32-bit buffer range");
    static bool attr[2] = {false, false};
    const void* kfn = a.res ? (const void*)l2conv_kernel<true, false, true> : (const void*)l2conv_kernel<false, false, true>;
    const int smem = (a.res ? SMEM_RES : OFF_RES) + TAIL;
    if (!attr[a.res ? 1 : 0]) {
      SAD_CHECK_HIP(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
      attr[a.res ? 1 : 0] = true;
    }
    if (a.res)
      hipLaunchKernelGGL((l2conv_kernel<true, false, true>), dim3((unsigned)g), dim3(256), smem, s, b);
    else
      hipLaunchKernelGGL((l2conv_kernel<false, false, true>), dim3((unsigned)g), dim3(256), smem, s, b);
    SAD_CHECK_HIP(hipGetLastError());
    return SAD_OK;
  }
  SAD_REQUIRE(!a.in1 || (!a.res && a.Cin1 == 64 && a.ss1 == 2 && a.H1 == 2 * a.H && a.W1 == 2 * a.W &&
                         a.in1_pstride % 8 == 0 && a.wt_ld >= 9 * 128 + 64),
              "variant 41: the shortcut is a 1x1/2 downsample of a 64-channel input at twice the size");
  SAD_REQUIRE(a.Cin == 128 && a.Cout == 128, "variant 41: Cin = Cout = 128");
  SAD_REQUIRE(a.H % 16 == 0 && a.W % 16 == 0 && a.Ho == a.H && a.Wo == a.W, "variant 41: image must tile by 16 x 16");
  SAD_REQUIRE(a.wt_ld >= 9 * 128 && a.wt_ld % 8 == 0, "variant 41: weight rows");
  SAD_REQUIRE(a.in0_pstride % 8 == 0 && a.out_pstride % 8 == 0 && (!a.res || a.res_pstride % 8 == 0) &&
                  a.in0_pstride >= 128 && a.out_pstride >= 128 && (!a.res || a.res_pstride >= 128),
              "variant 41: 16-B aligned pixel strides");
  SAD_REQUIRE(a.out, "null output");
  const int64_t tiles = (int64_t)a.N * (a.H / 16) * (a.W / 16);
  if (tiles == 0) return SAD_OK;
  const int64_t g = std::min<int64_t>(tiles, 256);
  BlockConvArgs b = a;
  b.out_bytes = ((int64_t)a.N * a.H * a.W - 1) * a.out_pstride * 2 + 256;
  SAD_REQUIRE(b.out_bytes < (1ll << 31) - 65536, "variant 41: output passes the 32-bit buffer range");
  // one launch path for every bf16 form: the kernel, its LDS size, and the
  // opt-in to that size once per kernel
  auto go = [&](auto kern, int smem, bool& attr) {
    if (!attr) {
      SAD_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem));
      attr = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(256), smem, s, b);
    return SAD_OK;
  };
  static bool attr[10] = {};
  int rc;
  if (h16) {
    rc = a.res   ? go(l2conv_kernel<true, false, false, false, f16>, SMEM_RES + TAIL, attr[7])
         : a.in1 ? go(l2conv_kernel<false, true, false, false, f16>, SMEM_RES + TAIL, attr[8])
                 : go(l2conv_kernel<false, false, false, false, f16>, OFF_RES + TAIL, attr[9]);
  } else if (a.st_part) {
    rc = go(l2conv_kernel<false, false, false, true>, OFF_RES + TAIL, attr[6]);
    if (rc == SAD_OK) *a.st_rows = (int)g;
  } else if (a.res) {
    rc = a.ablate ? go(l2conv_ablate_kernel<true, false>, SMEM_RES + TAIL, attr[3])
                  : go(l2conv_kernel<true, false>, SMEM_RES + TAIL, attr[0]);
  } else if (a.in1) {
    rc = a.ablate ? go(l2conv_ablate_kernel<false, true>, SMEM_RES + TAIL, attr[4])
                  : go(l2conv_kernel<false, true>, SMEM_RES + TAIL, attr[1]);
  } else {
    rc = a.ablate ? go(l2conv_ablate_kernel<false, false>, OFF_RES + TAIL, attr[5])
                  : go(l2conv_kernel<false, false>, OFF_RES + TAIL, attr[2]);
  }
  if (rc != SAD_OK) return rc;
  SAD_CHECK_HIP(hipGetLastError());
  return SAD_OK;
}

}  // namespace sad
