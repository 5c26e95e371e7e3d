// api.hip -- C ABI of libsad.so: runtime, backbone and heads plans.
// Declarations and the reference interfaces each entry replaces: include/sad.h.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace sad {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

}  // namespace sad

using namespace sad;

struct sad_backbone_plan {
  int dtype;
  int mh, mw;
  int device;
  void* stem_w = nullptr;
  float* stem_b = nullptr;
  float* stem_w3 = nullptr;  // distinct-channel stem (sad_backbone_run_img3)
  std::vector<BasicBlock> blocks;
};

struct sad_heads_plan {
  int n_heads, n_feat;
  int feat_dim;                    // backbone feature width (512: ResNet-18/34; 2048: Bottleneck ResNets)
  int device;
  std::vector<int> feat_index;
  std::vector<int> group_of;      // head -> group (== feat index order of appearance)
  std::vector<int> y1_col;        // head -> column offset in Y1
  std::vector<std::vector<int>> groups;  // feat -> heads
  std::vector<float*> w1;          // per group: [512*G][512] folded
  std::vector<float*> b1;          // per group: [512*G]
  float* w2 = nullptr;             // [N][256][512] folded
  float* b2 = nullptr;             // [N][256]
  float* w3 = nullptr;             // [N][2][256]
  float* b3 = nullptr;             // [N][2]
  // sad_heads_grad_run only, built on its first call (a plan that never explains allocates none of it)
  struct Grad {
    std::mutex mu;
    bool built = false;
    std::vector<float*> w1t;       // per head: [feat_dim][512] = folded W1 transposed
    float* w2t = nullptr;          // [N][512][256] = folded W2 transposed
    float* zero = nullptr;         // [max(512, feat_dim)] zero bias
    float* scratch = nullptr;      // [kGradRows][256 + 512]: one row range's masked operands
  };
  mutable Grad grad;
};

extern "C" const char* sad_last_error(void) { return g_err.c_str(); }
extern "C" const char* sad_version(void) { return "libsad 0.1 gfx950 (" __DATE__ " " __TIME__ ")"; }

extern "C" int sad_init(int device) {
  int n = 0;
  SAD_CHECK_HIP(hipGetDeviceCount(&n));
  SAD_REQUIRE(device >= 0 && device < n, "device index out of range");
  SAD_CHECK_HIP(hipSetDevice(device));
  return SAD_OK;
}

// ------------------------------------------------------------- folding ----
namespace sad {
void fold_bn(const float* g, const float* beta, const float* mu, const float* var, int c,
             std::vector<double>& scale, std::vector<double>& shift) {
  scale.resize(c);
  shift.resize(c);
  for (int i = 0; i < c; ++i) {
    scale[i] = (double)g[i] / sqrt((double)var[i] + 1e-5);
    shift[i] = (double)beta[i] - (double)mu[i] * scale[i];
  }
}

int upload_typed(void** dst, const std::vector<double>& v, int dtype, int64_t row_len) {
  if (dtype == SAD_BF16X3) {
    // split-bf16: each row's K axis in groups of 32 -> [hi 32 | lo 32] (the
    // activations' channel interleave, so one 128-B K-step pairs them up)
    if (row_len <= 0 || row_len % 32 != 0 || v.size() % (size_t)row_len != 0) {
      set_error("split-bf16 weights need rows of a multiple of 32 elements");
      return SAD_ERR_ARG;
    }
    std::vector<u16> h(2 * v.size());
    for (size_t i = 0; i < v.size(); ++i) {
      const float x = (float)v[i];
      const u16 hi = f2bf_host(x);
      float hf;
      const uint32_t hb = (uint32_t)hi << 16;
      memcpy(&hf, &hb, 4);
      const size_t g = i / 32, e = i % 32;
      h[g * 64 + e] = hi;
      h[g * 64 + 32 + e] = f2bf_host(x - hf);
    }
    return upload(dst, h);
  }
  if (dtype == SAD_BF16) {
    std::vector<u16> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = f2bf_host((float)v[i]);
    return upload(dst, h);
  }
  if (dtype == SAD_F16) {  // (the folds check the range first: check_f16_range)
    std::vector<u16> h(v.size());
    for (size_t i = 0; i < v.size(); ++i) h[i] = f2h_host((float)v[i]);
    return upload(dst, h);
  }
  std::vector<float> h(v.size());
  for (size_t i = 0; i < v.size(); ++i) h[i] = (float)v[i];
  return upload(dst, h);
}

int check_f16_range(const std::vector<double>& w, const std::vector<float>& b, const std::string& name) {
  for (size_t i = 0; i < w.size(); ++i)
    if (!(fabs(w[i]) <= (double)F16_MAX)) {  // (also NaN)
      set_error("argument check failed: fp16 plan: folded weight " + std::to_string(i) + " of " + name + " is " +
                std::to_string(w[i]) + ": not finite or beyond fp16's largest value 65504");
      return SAD_ERR_ARG;
    }
  for (size_t i = 0; i < b.size(); ++i)
    if (!std::isfinite(b[i])) {
      set_error("argument check failed: fp16 plan: folded bias " + std::to_string(i) + " of " + name +
                " is not finite");
      return SAD_ERR_ARG;
    }
  return SAD_OK;
}

// conv1 7x7/2 + bn1 folded for the stem kernel, the 3 identical input channels
// summed; k = ky*7+kx padded to 64 (params: conv weight, BN weight/bias/mean/var)
int fold_stem(const float* const* params, int dtype, void** w_out, float** b_out, float** w3_out) {
  const float* W = params[0];
  std::vector<double> sc, sh;
  fold_bn(params[1], params[2], params[3], params[4], 64, sc, sh);
  std::vector<double> w(64 * 64, 0.0);
  const int wdt = dtype == SAD_BF16X3 || dtype == SAD_F16 ? SAD_BF16 : dtype;  // split stem: bf16 layout, hi then lo; fp16: bf16's
  std::vector<float> b(64);
  for (int co = 0; co < 64; ++co) {
    for (int k = 0; k < 49; ++k) {
      double s = 0.0;
      for (int c = 0; c < 3; ++c) s += (double)W[(co * 3 + c) * 49 + k];
      // bf16 stem: (ky, kx) on an 8x8 grid; f32 stem: k = ky*7+kx, k=4q+g at g*16+q
      const int pos = wdt == SAD_BF16 ? (k / 7) * 8 + (k % 7) : ((k & 3) * 16 + (k >> 2));
      w[co * 64 + pos] = s * sc[co];
    }
    b[co] = (float)sh[co];
  }
  int rc;
  if (dtype == SAD_F16 && (rc = check_f16_range(w, b, "conv1"))) return rc;
  {  // [64 co][3 c][49 k] fp32, BN scale folded (distinct-channel stem)
    std::vector<float> w3(64 * 3 * 49);
    for (int co = 0; co < 64; ++co)
      for (int i = 0; i < 3 * 49; ++i) w3[co * 147 + i] = (float)((double)W[co * 147 + i] * sc[co]);
    if ((rc = upload((void**)w3_out, w3))) return rc;
  }
  if (dtype == SAD_BF16X3) {  // [64 co][64 k] hi, then [64][64] lo
    std::vector<u16> h(2 * 64 * 64);
    for (int i = 0; i < 64 * 64; ++i) {
      const float x = (float)w[i];
      h[i] = f2bf_host(x);
      float hf;
      const uint32_t hb = (uint32_t)h[i] << 16;
      memcpy(&hf, &hb, 4);
      h[64 * 64 + i] = f2bf_host(x - hf);
    }
    if ((rc = upload(w_out, h))) return rc;
  } else if ((rc = upload_typed(w_out, w, dtype))) {
    return rc;
  }
  return upload((void**)b_out, b);
}

int check_map_upsamples(int map_h, int map_w) {
  if (map_h > 512 || map_w > 512) {
    set_error("argument check failed: map shape " + std::to_string(map_h) + " x " + std::to_string(map_w) +
              " exceeds the limit of 512 per side (the stem's resize is upsampling only: no antialias filter)");
    return SAD_ERR_ARG;
  }
  return SAD_OK;
}
}  // namespace sad

extern "C" int sad_backbone_plan_create(const float* const* params, int32_t n_params, int32_t dtype,
                                        int32_t map_h, int32_t map_w, sad_backbone_plan** out) {
  SAD_REQUIRE(params && out, "null params/out");
  SAD_REQUIRE(n_params == 20 * 5, "n_params must be 100 (20 conv+BN groups)");
  SAD_REQUIRE(dtype == SAD_F32 || dtype == SAD_BF16 || dtype == SAD_BF16X3 || dtype == SAD_F16, "dtype");
  SAD_REQUIRE(map_h > 0 && map_w > 0, "map shape");
  if (int rc = check_map_upsamples(map_h, map_w)) return rc;
  for (int i = 0; i < n_params; ++i) SAD_REQUIRE(params[i] != nullptr, "null parameter pointer");
  {
    const char* env = getenv("SAD_BACKBONE_PATH");
    SAD_REQUIRE(!(env && strcmp(env, "igemm") == 0),
                "SAD_BACKBONE_PATH=igemm: the first-generation per-conv backbone path was removed (unset the variable)");
  }
  auto* p = new sad_backbone_plan();
  p->dtype = dtype;
  p->mh = map_h;
  p->mw = map_w;
  (void)hipGetDevice(&p->device);
  int rc;
  if ((rc = fold_stem(params, dtype, &p->stem_w, &p->stem_b, &p->stem_w3))) {
    sad_backbone_plan_destroy(p);  // (no device: the first upload fails)
    return rc;
  }
  // 20 conv+BN groups in timm state-dict order: the stem, then per block conv1,
  // conv2 and (the first blocks of layers 2-4) the downsample
  const float* const* q = params + 5;
  int inp = 64;
  for (int li = 0; li < 4; ++li) {
    for (int b = 0; b < 2; ++b) {
      const bool has_ds = b == 0 && li > 0;
      p->blocks.emplace_back();
      const std::string name = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      if ((rc = fold_basic_block(q, q + 5, has_ds ? q + 10 : nullptr, inp, 64 << li, has_ds ? 2 : 1, dtype,
                                 p->blocks.back(), name.c_str()))) {
        sad_backbone_plan_destroy(p);
        return rc;
      }
      q += has_ds ? 15 : 10;
      inp = 64 << li;
    }
  }
  *out = p;
  return SAD_OK;
}

extern "C" int sad_backbone_plan_destroy(sad_backbone_plan* p) {
  if (!p) return SAD_OK;
  (void)hipFree(p->stem_w);
  (void)hipFree(p->stem_b);
  (void)hipFree(p->stem_w3);
  for (auto& b : p->blocks) free_basic_block(b);
  delete p;
  return SAD_OK;
}

static constexpr int64_t kMaxActElems = 128ll * 128 * 64;  // per segment, layer1 map
static size_t act_bytes(const sad_backbone_plan* p, int64_t mb) {
  const size_t es = dtype_bytes(p->dtype);  // fp32 and split-bf16: 4 B per value
  return ((size_t)mb * kMaxActElems * es + 255) & ~(size_t)255;
}

extern "C" int sad_backbone_workspace_size(const sad_backbone_plan* p, int64_t mb, size_t* bytes) {
  SAD_REQUIRE(p && bytes && mb > 0, "bad args");
  *bytes = 4 * act_bytes(p, mb);
  return SAD_OK;
}

// ---- launch timing of the block-conv kernels (sad_profile_*): HIP events on
// the launch stream around each launch, keyed by tile variant, with the
// launch's algorithmic FLOPs (the identity shortcut's K columns excluded).
struct ProfRec {
  int variant;
  double flops;
  hipEvent_t e0, e1;
  int64_t kernels;  // kernel launches inside the bracket (image-range splits each count)
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;

int sad::timed_block_conv(const BlockConvArgs& a, int dtype, hipStream_t s, double flops) {
  if (!g_prof_on) return launch_block_conv(a, dtype, s);
  ProfRec r{a.x4 ? gemm_block_variant(a) : default_block_variant(a, dtype), flops, nullptr, nullptr, 0};
  SAD_CHECK_HIP(hipEventCreate(&r.e0));
  SAD_CHECK_HIP(hipEventCreate(&r.e1));
  SAD_CHECK_HIP(hipEventRecord(r.e0, s));
  const int64_t k0 = block_conv_kernel_launches();
  int rc = launch_block_conv(a, dtype, s);
  r.kernels = block_conv_kernel_launches() - k0;
  SAD_CHECK_HIP(hipEventRecord(r.e1, s));
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.push_back(r);
  return rc;
}

// SAD_L1_FUSED=0 runs layer1's blocks as two convs each (variant 25) instead of
// the fused BasicBlock kernel (variant 40; A/B switch).  Same box, 2 rounds:
// fused with 128-segment front sub-batches 52.5k seg/s vs 51.5k unfused at 32
bool sad::l1_fused() {
  static const bool v = env_int("SAD_L1_FUSED", 1) != 0;
  return v;
}
int sad::timed_l1block(const L1BlockArgs& a, hipStream_t s, double flops) {
  if (!g_prof_on) return launch_l1block(a, s);
  ProfRec r{40, flops, nullptr, nullptr, 1};
  SAD_CHECK_HIP(hipEventCreate(&r.e0));
  SAD_CHECK_HIP(hipEventCreate(&r.e1));
  SAD_CHECK_HIP(hipEventRecord(r.e0, s));
  int rc = launch_l1block(a, s);
  SAD_CHECK_HIP(hipEventRecord(r.e1, s));
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof.push_back(r);
  return rc;
}

extern "C" int sad_profile_begin(void) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  g_prof.clear();
  g_prof_on = true;
  return SAD_OK;
}

// sad_shutdown: release what the library itself holds (the launch-timing
// events of an unfinished sad_profile_begin) after the device has drained.
// Plans are caller-owned and destroyed by their *_destroy calls.
extern "C" int sad_shutdown(void) {
  SAD_CHECK_HIP(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& r : g_prof) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  g_prof.clear();
  g_prof_on = false;
  return SAD_OK;
}

extern "C" int sad_profile_end(int32_t variant, double* total_ms, int64_t* launches, double* flops) {
  SAD_REQUIRE(total_ms && launches && flops, "null outputs");
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on = false;
  double ms = 0.0, fl = 0.0;
  int64_t n = 0;
  for (auto& r : g_prof) {
    if (variant == 0 || r.variant == variant) {
      SAD_CHECK_HIP(hipEventSynchronize(r.e1));
      float t = 0.f;
      SAD_CHECK_HIP(hipEventElapsedTime(&t, r.e0, r.e1));
      ms += t;
      fl += r.flops;
      n += r.kernels;
    }
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
  }
  g_prof.clear();
  *total_ms = ms;
  *launches = n;
  *flops = fl;
  return SAD_OK;
}

// Blocks [b0, b1) on n segments: *in (NHWC, H x H x C) -> *in (the last
// output; the buffers *in and *alt swap per block, tmp holds conv1's output).
// pool_out (optional): fuse the global average pool into the last block's conv2
// when its kernel can (*pooled says whether it did; its NHWC output is not written)
static int run_blocks(const sad_backbone_plan* p, size_t b0, size_t b1, int64_t n, void** in, void** alt, void* tmp,
                      int& H, int& C, hipStream_t s, float* pool_out = nullptr, bool* pooled = nullptr) {
  for (size_t bi = b0; bi < b1; ++bi) {
    const BasicBlock& blk = p->blocks[bi];
    if (int rc = run_basic_block(blk, p->dtype, *in, tmp, *alt, n, H, s, bi + 1 == b1 ? pool_out : nullptr, pooled,
                                 true))
      return rc;
    std::swap(*in, *alt);
    H /= blk.stride;
    C = blk.cout;
  }
  return SAD_OK;
}

// Segments per sub-chunk for the stem and layer1 on the block path
// (SAD_FRONT_MB; 0 = the whole micro-batch).  At 32 segments a layer1
// activation is 64 MiB (bf16), so a conv's input, output and residual can stay
// in the 256 MiB Infinity Cache; layers 2-4 run on the whole micro-batch (their
// grids need the pixels, and bigger launches amortise the persistent kernels'
// ramp and tail).  Same-box sweeps (round 2, "front:micro-batch"):
// 32:512 46.9k seg/s vs 0:128 45.9k, 0:512 44.4-46.4k, 64:512 45.4k; 16 is 7%
// slower (layer2's grids underfill).  At 32:128 one box measured -1.1%.
// Round 2 at micro-batch 1024: 40 is 0.9 % and 48 1.4 % slower than 32 (same
// box, 3 rounds; profiles/r02s3_frontmb_ab.log).
// With layer1 fused (bf16, variant 40) only the block inputs/outputs pass
// through memory and the fused kernel's per-workgroup weight prologue wants
// more tiles: 128 segments (+1.8-2.1 % end to end vs fused at 32, same box;
// 64: +1.7-2 %).  With layer2 on variant 41 (round 3): 256 is +0.4-3 % over 128
// (same box, 3 rounds, tools/r03_sweep2.sh: 59.0-59.1k vs 57.3-58.9k seg/s;
// 512 with micro-batch 2048 within 0.2 % of 256).
static int front_sub_batch(int dtype) {
  static int v = env_int("SAD_FRONT_MB", -1);
  if (v >= 0) return v;
  // split-bf16 (layer1 on variant 42): 64, +0.8 % over 32 in the parity mode
  // (same box, 2 rounds; 128 and the whole micro-batch are slower,
  // profiles/r04_x3_frontmb_ab.log)
  return is16(dtype) && l1_fused() ? 256 : dtype == SAD_BF16X3 ? 64 : 32;
}

// Stem + layer1 of the block path on mb segments, per sub-chunk of
// front_sub_batch segments; layer1's output [mb, 128, 128, 64] is gathered in bufD.
static int run_front(const sad_backbone_plan* p, const float* map, const float* img, const float* img3, int64_t mb,
                     void* bufA, void* bufB, void* bufT, void* bufD, int& H, int& C, hipStream_t s) {
  int rc;
  const size_t es = dtype_bytes(p->dtype);
  const int64_t f = front_sub_batch(p->dtype) > 0 ? std::min<int64_t>(front_sub_batch(p->dtype), mb) : mb;
  // stem + layer1 per sub-chunk of f segments (Infinity-Cache-sized); layer1's
  // output ([f, 128, 128, 64] per sub-chunk) is gathered in bufD, then layers
  // 2-4 run on the whole micro-batch (layer2's halo grids underfill at f = 32:
  // its two convs took 218 + 201 vs 197 + 185 us per 128 segments).
  const size_t l1_elems = 128 * 128 * 64;
  for (int64_t i = 0; i < mb; i += f) {
    const int64_t n = std::min(f, mb - i);
    void* a0 = bufA;
    void* a1 = bufB;
    StemArgs st{map ? map + i * p->mh * p->mw : nullptr, img ? img + i * 512 * 512 : nullptr, p->mh, p->mw,
                p->stem_w, p->stem_b, a0, n, img3 ? img3 + i * 3 * 512 * 512 : nullptr, p->stem_w3};
    if ((rc = launch_stem(st, p->dtype, s))) return rc;
    H = 128;
    C = 64;
    if ((rc = run_blocks(p, 0, 1, n, &a0, &a1, bufT, H, C, s))) return rc;
    // layer1's second block writes straight into its slot of bufD
    void* slot = (char*)bufD + (size_t)i * l1_elems * es;
    void* dst = slot;
    void* src = a0;
    if ((rc = run_blocks(p, 1, 2, n, &src, &dst, bufT, H, C, s))) return rc;
    if (src != slot) {
      set_error("internal: layer1 output not in its bufD slot");
      return SAD_ERR_STATE;
    }
  }
  return SAD_OK;
}

static int run_chunk(const sad_backbone_plan* p, const float* map, const float* img, int64_t mb, float* feats,
                     void* layer4_out, char* ws, hipStream_t s, const float* img3 = nullptr) {
  const size_t ab = act_bytes(p, mb);
  void* bufA = ws;
  void* bufB = ws + ab;
  void* bufT = ws + 2 * ab;
  void* bufD = ws + 3 * ab;
  int rc;
  int H = 128, C = 64;
  bool pooled = false;  // the last conv wrote the pooled features itself
  if ((rc = run_front(p, map, img, img3, mb, bufA, bufB, bufT, bufD, H, C, s))) return rc;
  void* a0 = bufD;
  void* a1 = bufA;
  if ((rc = run_blocks(p, 2, p->blocks.size(), mb, &a0, &a1, bufB, H, C, s, layer4_out ? nullptr : feats, &pooled)))
    return rc;
  bufA = a0;
  if (layer4_out) {
    const size_t es = dtype_bytes(p->dtype);
    SAD_CHECK_HIP(hipMemcpyAsync(layer4_out, bufA, (size_t)mb * H * H * C * es, hipMemcpyDeviceToDevice, s));
  }
  if (pooled) return SAD_OK;
  return launch_avgpool(bufA, mb, H * H, C, feats, p->dtype, s);
}

// ---- shared-trunk ensembles: the backbone split after layer3.  The trunk
// (stem, layer1-3) and the tail (layer4 + average pool) issue exactly the
// launches run_chunk issues for their part, on the same micro-batch, so
// trunk + tail is bit-identical to sad_backbone_run*.
static constexpr int64_t kL3Elems = 32ll * 32 * 256;  // per segment, layer3 output
static size_t l3_bytes(const sad_backbone_plan* p, int64_t n) {
  return (size_t)n * kL3Elems * (dtype_bytes(p->dtype));
}

// stem .. layer3 on mb segments -> l3_out [mb, 32, 32, 256] (plan layout)
static int trunk_chunk(const sad_backbone_plan* p, const float* map, const float* img, int64_t mb, void* l3_out,
                       char* ws, hipStream_t s) {
  const size_t ab = act_bytes(p, mb);
  void* bufA = ws;
  void* bufB = ws + ab;
  void* bufT = ws + 2 * ab;
  void* bufD = ws + 3 * ab;
  int rc;
  int H = 128, C = 64;
  if ((rc = run_front(p, map, img, nullptr, mb, bufA, bufB, bufT, bufD, H, C, s))) return rc;
  void* a0 = bufD;
  void* a1 = bufA;
  if ((rc = run_blocks(p, 2, 5, mb, &a0, &a1, bufB, H, C, s))) return rc;
  // layer3's second block writes straight into l3_out
  void* src = a0;
  void* dst = l3_out;
  if ((rc = run_blocks(p, 5, 6, mb, &src, &dst, bufB, H, C, s))) return rc;
  if (src != l3_out || H != 32 || C != 256) {
    set_error("internal: layer3 output not in l3_out");
    return SAD_ERR_STATE;
  }
  return SAD_OK;
}

// layer4 + average pool on l3 [mb, 32, 32, 256] (read only) -> feats [mb, 512].
// The two blocks run as two calls so that the second writes a workspace
// buffer, not the first one's input.
static int tail_chunk(const sad_backbone_plan* p, const void* l3, int64_t mb, float* feats, char* ws,
                      hipStream_t s) {
  const size_t ab = act_bytes(p, mb);
  void* bufX = ws;
  void* bufY = ws + ab;
  void* bufT = ws + 2 * ab;
  int rc;
  int H = 32, C = 256;
  bool pooled = false;
  void* src = const_cast<void*>(l3);
  void* dst = bufX;
  if ((rc = run_blocks(p, 6, 7, mb, &src, &dst, bufT, H, C, s))) return rc;
  dst = bufY;
  if ((rc = run_blocks(p, 7, 8, mb, &src, &dst, bufT, H, C, s, feats, &pooled))) return rc;
  if (pooled) return SAD_OK;
  if (src != bufY) {
    set_error("internal: layer4 output not in its workspace buffer");
    return SAD_ERR_STATE;
  }
  return launch_avgpool(src, mb, H * H, C, feats, p->dtype, s);
}

extern "C" int sad_backbone_trunk_run(const sad_backbone_plan* p, const float* map, const float* img, int64_t B,
                                      int64_t mb, void* l3_out, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && l3_out && ws, "null args");
  SAD_REQUIRE((map != nullptr) != (img != nullptr), "exactly one of map and img must be given");
  SAD_REQUIRE(B >= 0 && mb > 0, "bad batch");
  SAD_REQUIRE(p->blocks.size() == 8, "not a ResNet-18 plan");
  size_t need = 0;
  sad_backbone_workspace_size(p, mb, &need);
  if (ws_bytes < need) {
    set_error("workspace too small");
    return SAD_ERR_NOMEM;
  }
  const int64_t plane = map ? (int64_t)p->mh * p->mw : 512 * 512;
  const float* x = map ? map : img;
  for (int64_t i = 0; i < B; i += mb) {
    const int64_t n = std::min(mb, B - i);
    const float* xi = x + i * plane;
    int rc = trunk_chunk(p, map ? xi : nullptr, map ? nullptr : xi, n, (char*)l3_out + l3_bytes(p, i), (char*)ws,
                         (hipStream_t)stream);
    if (rc) return rc;
  }
  return SAD_OK;
}

extern "C" int sad_backbone_tail_run(const sad_backbone_plan* p, const void* l3, int64_t B, int64_t mb,
                                     float* feats, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && l3 && feats && ws, "null args");
  SAD_REQUIRE(B >= 0 && mb > 0, "bad batch");
  SAD_REQUIRE(p->blocks.size() == 8, "not a ResNet-18 plan");
  size_t need = 0;
  sad_backbone_workspace_size(p, mb, &need);
  if (ws_bytes < need) {
    set_error("workspace too small");
    return SAD_ERR_NOMEM;
  }
  for (int64_t i = 0; i < B; i += mb) {
    const int64_t n = std::min(mb, B - i);
    int rc = tail_chunk(p, (const char*)l3 + l3_bytes(p, i), n, feats + i * 512, (char*)ws, (hipStream_t)stream);
    if (rc) return rc;
  }
  return SAD_OK;
}

extern "C" int sad_backbone_shared_workspace_size(const sad_backbone_plan* p, int64_t mb, size_t* bytes) {
  SAD_REQUIRE(p && bytes && mb > 0, "bad args");
  *bytes = 4 * act_bytes(p, mb) + ((l3_bytes(p, mb) + 255) & ~(size_t)255);
  return SAD_OK;
}

extern "C" int sad_backbone_shared_run(const sad_backbone_plan* trunk, const sad_backbone_plan* const* tails,
                                       int32_t n_tails, const float* map, const float* img, int64_t B, int64_t mb,
                                       float* const* feats, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(trunk && tails && feats && ws, "null args");
  SAD_REQUIRE(n_tails > 0, "n_tails must be positive");
  SAD_REQUIRE((map != nullptr) != (img != nullptr), "exactly one of map and img must be given");
  SAD_REQUIRE(B >= 0 && mb > 0, "bad batch");
  SAD_REQUIRE(trunk->blocks.size() == 8, "not a ResNet-18 plan");
  for (int t = 0; t < n_tails; ++t) {
    SAD_REQUIRE(tails[t] && feats[t], "null tail plan or feature pointer");
    SAD_REQUIRE(tails[t]->blocks.size() == 8, "tail is not a ResNet-18 plan");
    SAD_REQUIRE(tails[t]->dtype == trunk->dtype, "tail plan dtype differs from the trunk's");
    SAD_REQUIRE(tails[t]->mh == trunk->mh && tails[t]->mw == trunk->mw, "tail plan map size differs from the trunk's");
  }
  size_t need = 0;
  sad_backbone_shared_workspace_size(trunk, mb, &need);
  if (ws_bytes < need) {
    set_error("workspace too small");
    return SAD_ERR_NOMEM;
  }
  void* l3 = (char*)ws + 4 * act_bytes(trunk, mb);
  const int64_t plane = map ? (int64_t)trunk->mh * trunk->mw : 512 * 512;
  const float* x = map ? map : img;
  for (int64_t i = 0; i < B; i += mb) {
    const int64_t n = std::min(mb, B - i);
    const float* xi = x + i * plane;
    int rc = trunk_chunk(trunk, map ? xi : nullptr, map ? nullptr : xi, n, l3, (char*)ws, (hipStream_t)stream);
    if (rc) return rc;
    for (int t = 0; t < n_tails; ++t)
      if ((rc = tail_chunk(tails[t], l3, n, feats[t] + i * 512, (char*)ws, (hipStream_t)stream))) return rc;
  }
  return SAD_OK;
}

extern "C" int sad_backbone_run(const sad_backbone_plan* p, const float* map, int64_t B, int64_t mb,
                                float* feats, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && feats && ws, "null args");
  SAD_REQUIRE(B >= 0 && mb > 0, "bad batch");
  size_t need = 0;
  sad_backbone_workspace_size(p, mb, &need);
  if (ws_bytes < need) {
    set_error("workspace too small");
    return SAD_ERR_NOMEM;
  }
  const int64_t plane = (int64_t)p->mh * p->mw;
  for (int64_t i = 0; i < B; i += mb) {
    const int64_t n = std::min(mb, B - i);
    int rc = run_chunk(p, map + i * plane, nullptr, n, feats + i * 512, nullptr, (char*)ws, (hipStream_t)stream);
    if (rc) return rc;
  }
  return SAD_OK;
}

extern "C" int sad_backbone_run_debug(const sad_backbone_plan* p, const float* map, int64_t B, float* feats,
                                      void* layer4_out, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && feats && ws && layer4_out && B > 0, "null args");
  size_t need = 0;
  sad_backbone_workspace_size(p, B, &need);
  if (ws_bytes < need) {
    set_error("workspace too small (debug run needs micro_batch = B)");
    return SAD_ERR_NOMEM;
  }
  return run_chunk(p, map, nullptr, B, feats, layer4_out, (char*)ws, (hipStream_t)stream);
}

extern "C" int sad_backbone_run_keep(const sad_backbone_plan* p, const float* map, const float* img, int64_t B,
                                     float* feats, void* l4_out, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && feats && l4_out && ws, "run_keep: null plan, feats, l4_out or workspace");
  SAD_REQUIRE((map != nullptr) != (img != nullptr), "run_keep: exactly one of map and img must be given");
  SAD_REQUIRE(B >= 0, "run_keep: negative B");
  if (B == 0) return SAD_OK;
  size_t need = 0;
  sad_backbone_workspace_size(p, B, &need);
  if (ws_bytes < need) {
    set_error("workspace too small (run_keep takes one chunk: B <= the micro-batch the workspace was sized for)");
    return SAD_ERR_NOMEM;
  }
  return run_chunk(p, map, img, B, feats, l4_out, (char*)ws, (hipStream_t)stream);
}

extern "C" int sad_backbone_stem_run(const sad_backbone_plan* p, const float* map, int64_t B, void* out,
                                     void* stream) {
  SAD_REQUIRE(p && map && out && B >= 0, "null args");
  StemArgs st{map, nullptr, p->mh, p->mw, p->stem_w, p->stem_b, out, B};
  return launch_stem(st, p->dtype, (hipStream_t)stream);
}

extern "C" int sad_backbone_stem_run_img(const sad_backbone_plan* p, const float* img, const float* img3, int64_t B,
                                         void* out, void* stream) {
  SAD_REQUIRE(p && out && B >= 0, "null args");
  SAD_REQUIRE((img != nullptr) != (img3 != nullptr), "exactly one of img / img3");
  StemArgs st{nullptr, img, p->mh, p->mw, p->stem_w, p->stem_b, out, B, img3, p->stem_w3};
  return launch_stem(st, p->dtype, (hipStream_t)stream);
}

extern "C" int sad_backbone_run_img(const sad_backbone_plan* p, const float* img, int64_t B, int64_t mb,
                                    float* feats, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && img && feats && ws, "null args");
  SAD_REQUIRE(B >= 0 && mb > 0, "bad batch");
  size_t need = 0;
  sad_backbone_workspace_size(p, mb, &need);
  if (ws_bytes < need) {
    set_error("workspace too small");
    return SAD_ERR_NOMEM;
  }
  for (int64_t i = 0; i < B; i += mb) {
    const int64_t n = std::min(mb, B - i);
    int rc = run_chunk(p, nullptr, img + i * 512 * 512, n, feats + i * 512, nullptr, (char*)ws, (hipStream_t)stream);
    if (rc) return rc;
  }
  return SAD_OK;
}

extern "C" int sad_backbone_run_img3(const sad_backbone_plan* p, const float* img3, int64_t B, int64_t mb,
                                     float* feats, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && img3 && feats && ws, "null args");
  SAD_REQUIRE(B >= 0 && mb > 0, "bad batch");
  size_t need = 0;
  sad_backbone_workspace_size(p, mb, &need);
  if (ws_bytes < need) {
    set_error("workspace too small");
    return SAD_ERR_NOMEM;
  }
  for (int64_t i = 0; i < B; i += mb) {
    const int64_t n = std::min(mb, B - i);
    int rc = run_chunk(p, nullptr, nullptr, n, feats + i * 512, nullptr, (char*)ws, (hipStream_t)stream,
                       img3 + i * 3 * 512 * 512);
    if (rc) return rc;
  }
  return SAD_OK;
}

// ---------------------------------------------------------------- heads ----
extern "C" int sad_heads_plan_create(const float* const* params, int32_t n_heads, const int32_t* feat_index,
                                     int32_t n_feat, sad_heads_plan** out) {
  return sad_heads_plan_create_dim(params, n_heads, feat_index, n_feat, 512, out);
}

// Folds and uploads into *p; on an error the caller destroys p.
static int heads_plan_fill(sad_heads_plan* p, const float* const* params, int n_heads, const int32_t* feat_index,
                           int n_feat, int feat_dim) {
  p->n_heads = n_heads;
  p->n_feat = n_feat;
  p->feat_dim = feat_dim;
  const int D = feat_dim;
  (void)hipGetDevice(&p->device);
  p->groups.assign(n_feat, {});
  for (int h = 0; h < n_heads; ++h) {
    const int f = feat_index ? feat_index[h] : 0;
    p->feat_index.push_back(f);
    p->groups[f].push_back(h);
  }
  p->y1_col.assign(n_heads, 0);
  int col = 0, rc;
  std::vector<double> sc, sh;
  for (int f = 0; f < n_feat; ++f) {
    const auto& g = p->groups[f];
    std::vector<float> w1((size_t)g.size() * 512 * D), b1(g.size() * 512);
    for (size_t gi = 0; gi < g.size(); ++gi) {
      const float* const* hp = params + g[gi] * 14;
      fold_bn(hp[2], hp[3], hp[4], hp[5], 512, sc, sh);
      for (int o = 0; o < 512; ++o) {
        for (int i = 0; i < D; ++i)
          w1[(gi * 512 + o) * D + i] = (float)((double)hp[0][(size_t)o * D + i] * sc[o]);
        b1[gi * 512 + o] = (float)((double)hp[1][o] * sc[o] + sh[o]);
      }
      p->y1_col[g[gi]] = col;
      col += 512;
    }
    // the plan owns each pointer from its allocation on (an empty group keeps NULL)
    p->w1.push_back(nullptr);
    p->b1.push_back(nullptr);
    if (!g.empty()) {
      if ((rc = upload((void**)&p->w1.back(), w1))) return rc;
      if ((rc = upload((void**)&p->b1.back(), b1))) return rc;
    }
  }
  std::vector<float> w2((size_t)n_heads * 256 * 512), b2(n_heads * 256), w3(n_heads * 512), b3(n_heads * 2);
  for (int h = 0; h < n_heads; ++h) {
    const float* const* hp = params + h * 14;
    fold_bn(hp[8], hp[9], hp[10], hp[11], 256, sc, sh);
    for (int o = 0; o < 256; ++o) {
      for (int i = 0; i < 512; ++i) w2[((size_t)h * 256 + o) * 512 + i] = (float)((double)hp[6][o * 512 + i] * sc[o]);
      b2[h * 256 + o] = (float)((double)hp[7][o] * sc[o] + sh[o]);
    }
    memcpy(&w3[h * 512], hp[12], 512 * sizeof(float));
    memcpy(&b3[h * 2], hp[13], 2 * sizeof(float));
  }
  if ((rc = upload((void**)&p->w2, w2))) return rc;
  if ((rc = upload((void**)&p->b2, b2))) return rc;
  if ((rc = upload((void**)&p->w3, w3))) return rc;
  if ((rc = upload((void**)&p->b3, b3))) return rc;
  return SAD_OK;
}

extern "C" int sad_heads_plan_create_dim(const float* const* params, int32_t n_heads, const int32_t* feat_index,
                                         int32_t n_feat, int32_t feat_dim, sad_heads_plan** out) {
  SAD_REQUIRE(params && out && n_heads > 0 && n_feat > 0, "bad args");
  SAD_REQUIRE(feat_dim > 0 && feat_dim % 64 == 0, "feat_dim must be a positive multiple of 64");
  for (int i = 0; i < n_heads * 14; ++i) SAD_REQUIRE(params[i], "null head parameter");
  for (int h = 0; h < n_heads; ++h)
    SAD_REQUIRE(!feat_index || (feat_index[h] >= 0 && feat_index[h] < n_feat), "feat_index out of range");
  // every head of one backbone shares the first GEMM: its weights are one operand
  SAD_REQUIRE((int64_t)n_heads * 512 * feat_dim * 4 < (1ll << 31) && (int64_t)n_heads * 512 * 4 < (1ll << 31) - 64,
              "too many heads for one GEMM operand (2 GiB buffer range)");
  auto* p = new sad_heads_plan();
  const int rc = heads_plan_fill(p, params, n_heads, feat_index, n_feat, feat_dim);
  if (rc) {  // a failed upload: nothing of the half-built plan stays behind
    sad_heads_plan_destroy(p);
    return rc;
  }
  *out = p;
  return SAD_OK;
}

extern "C" int sad_heads_plan_destroy(sad_heads_plan* p) {
  if (!p) return SAD_OK;
  for (auto* w : p->w1) (void)hipFree(w);
  for (auto* b : p->b1) (void)hipFree(b);
  (void)hipFree(p->w2);
  (void)hipFree(p->b2);
  (void)hipFree(p->w3);
  (void)hipFree(p->b3);
  for (auto* w : p->grad.w1t) (void)hipFree(w);
  (void)hipFree(p->grad.w2t);
  (void)hipFree(p->grad.zero);
  (void)hipFree(p->grad.scratch);
  delete p;
  return SAD_OK;
}

extern "C" int sad_heads_workspace_size(const sad_heads_plan* p, int64_t B, size_t* bytes) {
  SAD_REQUIRE(p && bytes && B >= 0, "bad args");
  *bytes = (size_t)B * p->n_heads * (512 + 256) * sizeof(float) + 256;
  return SAD_OK;
}

// The second layer is one grouped launch when the heads' hidden columns are in
// head order (always for a shared backbone), otherwise one launch per head.
static bool heads_regular(const sad_heads_plan* p) {
  bool regular = true;
  for (int h = 0; h < p->n_heads; ++h) regular = regular && p->y1_col[h] == h * 512;
  return regular;
}

// Both GEMMs address their input with 32-bit byte offsets, so a batch runs as
// row ranges that keep each operand inside launch_conv's buffer range: the
// features are [rows][feat_dim], y1 is [rows][N*512] read 512 columns at a time.
static int64_t heads_row_range(const sad_heads_plan* p) {
  const int64_t range = std::min(conv_max_pixels(p->feat_dim, p->feat_dim, SAD_F32),
                                 conv_max_pixels((int64_t)p->n_heads * 512, 512, SAD_F32));
  return range >= 512 ? range - range % 512 : range;  // whole tiles of every variant
}

extern "C" int sad_heads_plan_info(const sad_heads_plan* p, int32_t* grouped, int64_t* row_range) {
  SAD_REQUIRE(p && grouped && row_range, "null args");
  *grouped = heads_regular(p) ? 1 : 0;
  *row_range = heads_row_range(p);
  return SAD_OK;
}

extern "C" int sad_heads_merge_run(const sad_heads_plan* p, const float* const* feats, int64_t B, float* logits,
                                   float* merged, void* ws, size_t ws_bytes, void* stream) {
  SAD_REQUIRE(p && feats && merged && ws, "null args");
  size_t need = 0;
  sad_heads_workspace_size(p, B, &need);
  if (ws_bytes < need) {
    set_error("heads workspace too small");
    return SAD_ERR_NOMEM;
  }
  // refusals come before the first launch: a used group's features must be there
  for (int f = 0; f < p->n_feat; ++f) SAD_REQUIRE(p->groups[f].empty() || feats[f], "null feature pointer");
  if (B == 0) return SAD_OK;
  hipStream_t s = (hipStream_t)stream;
  const int N = p->n_heads;
  float* y1 = (float*)ws;
  float* y2 = y1 + (size_t)B * N * 512;
  // Rows are independent (a row's K order does not depend on its position) and
  // every range writes its own rows of the one workspace layout (include/sad.h).
  const int64_t range = heads_row_range(p);
  SAD_REQUIRE(range >= 1, "heads: one row exceeds the 2 GiB buffer range");
  const bool regular = heads_regular(p);
  int rc;
  for (int64_t r0 = 0; r0 < B; r0 += range) {
    const int64_t rows = std::min(range, B - r0);
    int col = 0;
    for (int f = 0; f < p->n_feat; ++f) {
      const int G = (int)p->groups[f].size();
      if (!G) continue;
      ConvArgs a{};
      a.in = feats[f] + r0 * p->feat_dim;
      a.in_pstride = p->feat_dim;
      a.N = (int)rows;
      a.H = a.W = 1;
      a.Cin = p->feat_dim;
      a.wt = p->w1[f];
      a.bias = p->b1[f];
      a.out = y1 + r0 * N * 512 + col;
      a.out_pstride = (int64_t)N * 512;
      a.Ho = a.Wo = 1;
      a.Cout = 512 * G;
      a.KH = a.KW = 1;
      a.stride = 1;
      a.pad = 0;
      a.relu = 1;
      a.M = rows;
      if ((rc = launch_conv(a, SAD_F32, s))) return rc;
      col += 512 * G;
    }
    // the N heads' Linear(512, 256) + BN1d + ReLU (grouped or per head: heads_regular)
    for (int h = 0; h < (regular ? 1 : N); ++h) {
      ConvArgs a{};
      if (regular && N > 1) {
        a.groups = N;
        a.in_gstride = 512;
        a.wt_gstride = (int64_t)256 * 512;
        a.bias_gstride = 256;
        a.out_gstride = 256;
      }
      a.in = y1 + r0 * N * 512 + p->y1_col[h];
      a.in_pstride = (int64_t)N * 512;
      a.N = (int)rows;
      a.H = a.W = 1;
      a.Cin = 512;
      a.wt = p->w2 + (size_t)h * 256 * 512;
      a.bias = p->b2 + h * 256;
      a.out = y2 + r0 * N * 256 + h * 256;
      a.out_pstride = (int64_t)N * 256;
      a.Ho = a.Wo = 1;
      a.Cout = 256;
      a.KH = a.KW = 1;
      a.stride = 1;
      a.pad = 0;
      a.relu = 1;
      a.M = rows;
      if ((rc = launch_conv(a, SAD_F32, s))) return rc;
    }
  }
  return launch_heads_final(y2, B, N, p->w3, p->b3, logits, merged, s);
}

// ---- head gradient (evidence maps): g = W1^T (m1 * (W2^T (m2 * W3[cls]))) per
// head, as two GEMMs on the f32 implicit-GEMM kernel over the TRANSPOSED
// folded weights, the ReLU masks taken from y1 / y2 as merge_run left them.
static constexpr int64_t kGradRows = 4096;  // rows per range (whole tiles of every variant)

static void heads_grad_free(const sad_heads_plan* p) {
  auto& g = p->grad;
  for (auto* w : g.w1t) (void)hipFree(w);
  g.w1t.clear();
  (void)hipFree(g.w2t);
  (void)hipFree(g.zero);
  (void)hipFree(g.scratch);
  g.w2t = g.zero = g.scratch = nullptr;
}

static int heads_grad_build(const sad_heads_plan* p, hipStream_t s) {
  auto& g = p->grad;
  const int N = p->n_heads, D = p->feat_dim;
  int rc;
  const size_t nz = (size_t)std::max(512, D);
  SAD_CHECK_HIP(hipMalloc((void**)&g.zero, nz * sizeof(float)));
  SAD_CHECK_HIP(hipMemsetAsync(g.zero, 0, nz * sizeof(float), s));
  SAD_CHECK_HIP(hipMalloc((void**)&g.scratch, (size_t)kGradRows * (256 + 512) * sizeof(float)));
  SAD_CHECK_HIP(hipMalloc((void**)&g.w2t, (size_t)N * 512 * 256 * sizeof(float)));
  for (int h = 0; h < N; ++h) {
    if ((rc = launch_transpose(p->w2 + (size_t)h * 256 * 512, g.w2t + (size_t)h * 512 * 256, 256, 512, s))) return rc;
    const auto& grp = p->groups[p->feat_index[h]];
    size_t gi = 0;
    while (grp[gi] != h) ++gi;
    g.w1t.push_back(nullptr);
    SAD_CHECK_HIP(hipMalloc((void**)&g.w1t.back(), (size_t)D * 512 * sizeof(float)));
    if ((rc = launch_transpose(p->w1[p->feat_index[h]] + gi * 512 * D, g.w1t.back(), 512, D, s))) return rc;
  }
  // later calls may come on other streams: the transposes are complete when this returns
  SAD_CHECK_HIP(hipStreamSynchronize(s));
  return SAD_OK;
}

extern "C" int sad_heads_grad_run(const sad_heads_plan* p, const void* ws, int64_t B, int32_t cls, float* g_out,
                                  void* stream) {
  SAD_REQUIRE(p && ws && g_out, "heads grad: null plan, workspace or g_out");
  SAD_REQUIRE(cls == 0 || cls == 1, "heads grad: cls must be 0 (Real) or 1 (Synthetic)");
  SAD_REQUIRE(B >= 0, "heads grad: negative B");
  if (B == 0) return SAD_OK;
  hipStream_t s = (hipStream_t)stream;
  {
    std::lock_guard<std::mutex> lk(p->grad.mu);
    if (!p->grad.built) {
      if (int rc = heads_grad_build(p, s)) {
        heads_grad_free(p);
        return rc;
      }
      p->grad.built = true;
    }
  }
  const int N = p->n_heads, D = p->feat_dim;
  const float* y1 = (const float*)ws;
  const float* y2 = y1 + (size_t)B * N * 512;
  float* u2 = p->grad.scratch;
  float* t1 = u2 + kGradRows * 256;
  int rc;
  for (int64_t r0 = 0; r0 < B; r0 += kGradRows) {
    const int64_t rows = std::min(kGradRows, B - r0);
    for (int h = 0; h < N; ++h) {
      // u2 = m2 * W3[cls];  t1 = u2 W2;  t1 *= m1;  g = t1 W1
      if ((rc = launch_relu_mask(y2 + r0 * N * 256 + h * 256, (int64_t)N * 256, p->w3 + h * 512 + cls * 256, u2, rows,
                                 256, s)))
        return rc;
      ConvArgs a{};
      a.in = u2;
      a.in_pstride = 256;
      a.N = (int)rows;
      a.H = a.W = 1;
      a.Cin = 256;
      a.wt = p->grad.w2t + (size_t)h * 512 * 256;
      a.bias = p->grad.zero;
      a.out = t1;
      a.out_pstride = 512;
      a.Ho = a.Wo = 1;
      a.Cout = 512;
      a.KH = a.KW = 1;
      a.stride = 1;
      a.pad = 0;
      a.relu = 0;
      a.M = rows;
      if ((rc = launch_conv(a, SAD_F32, s))) return rc;
      if ((rc = launch_relu_mask(y1 + r0 * N * 512 + p->y1_col[h], (int64_t)N * 512, nullptr, t1, rows, 512, s)))
        return rc;
      a.in = t1;
      a.in_pstride = 512;
      a.Cin = 512;
      a.wt = p->grad.w1t[h];
      a.out = g_out + ((size_t)h * B + r0) * D;
      a.out_pstride = D;
      a.Cout = D;
      if ((rc = launch_conv(a, SAD_F32, s))) return rc;
    }
  }
  return SAD_OK;
}

// ------------------------------------------------------------- operators ----
extern "C" int sad_conv2d_run(const void* in, int64_t N, int32_t H, int32_t W, int32_t Cin, const void* wt,
                              const float* bias, const void* res, void* out, int32_t Cout, int32_t k,
                              int32_t stride, int32_t pad, int32_t relu, int32_t dtype, int32_t variant,
                              void* stream) {
  SAD_REQUIRE(in && wt && bias && out, "null tensor");
  SAD_REQUIRE(N >= 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, "bad shape");
  SAD_REQUIRE(dtype == SAD_F32 || dtype == SAD_BF16 || dtype == SAD_F16, "dtype");
  ConvArgs a{};
  a.in = in;
  a.in_pstride = Cin;
  a.N = (int)N;
  a.H = H;
  a.W = W;
  a.Cin = Cin;
  a.wt = wt;
  a.bias = bias;
  a.res = res;
  a.res_pstride = Cout;
  a.out = out;
  a.out_pstride = Cout;
  a.Ho = (H + 2 * pad - k) / stride + 1;
  a.Wo = (W + 2 * pad - k) / stride + 1;
  a.Cout = Cout;
  a.KH = a.KW = k;
  a.stride = stride;
  a.pad = pad;
  a.relu = relu;
  a.M = N * a.Ho * a.Wo;
  return launch_conv(a, dtype, (hipStream_t)stream, variant);
}

extern "C" int sad_l1_block_run(const void* x, int64_t N, int32_t H, int32_t W, const void* w1, int32_t w1_ld,
                                const float* b1, const void* w2, int32_t w2_ld, const float* b2, void* out,
                                int32_t ablate, void* stream) {
  SAD_REQUIRE(x && w1 && b1 && w2 && b2 && out, "null tensor");
  SAD_REQUIRE(N >= 0 && N < (1ll << 31) && H > 0 && W > 0, "bad shape");
  const int64_t bytes = N * H * W * 128;
  SAD_REQUIRE((const char*)out + bytes <= (const char*)x || (const char*)x + bytes <= (const char*)out,
              "fused layer1 block: out must not overlap x");
  L1BlockArgs a{};
  a.x = (const u16*)x;
  a.out = (u16*)out;
  a.N = (int)N;
  a.H = H;
  a.W = W;
  a.w1 = (const u16*)w1;
  a.w1_ld = w1_ld;
  a.b1 = b1;
  a.w2 = (const u16*)w2;
  a.w2_ld = w2_ld;
  a.b2 = b2;
  a.ablate = ablate & 0xFFFF;
  a.h16 = (ablate & SAD_L1_BLOCK_F16) != 0;
  return launch_l1block(a, (hipStream_t)stream);
}

extern "C" int sad_block_conv_run(const void* in0, int64_t N, int32_t H, int32_t W, int32_t Cin, const void* in1,
                                  int32_t H1, int32_t W1, int32_t Cin1, int32_t ss1, const void* wt,
                                  int32_t wt_ld, const float* bias, const void* res, void* out, int32_t Cout,
                                  int32_t k, int32_t stride, int32_t pad, int32_t relu, int32_t dtype,
                                  int32_t variant, void* stream) {
  SAD_REQUIRE(in0 && wt && bias && out, "null tensor");
  SAD_REQUIRE(N >= 0 && H > 0 && W > 0 && k > 0 && stride > 0 && pad >= 0, "bad shape");
  SAD_REQUIRE(dtype == SAD_F32 || dtype == SAD_BF16 || dtype == SAD_BF16X3 || dtype == SAD_F16, "dtype");
  BlockConvArgs a{};
  a.in0 = in0;
  a.in0_pstride = Cin;
  a.N = (int)N;
  a.H = H;
  a.W = W;
  a.Cin = Cin;
  a.KH = a.KW = k;
  a.stride = stride;
  a.pad = pad;
  a.in1 = in1;
  a.in1_pstride = Cin1;
  a.H1 = H1;
  a.W1 = W1;
  a.Cin1 = in1 ? Cin1 : 0;
  a.ss1 = ss1;
  a.wt = wt;
  a.wt_ld = wt_ld;
  a.bias = bias;
  a.res = res;
  a.res_pstride = Cout;
  a.out = out;
  a.out_pstride = Cout;
  a.Ho = (H + 2 * pad - k) / stride + 1;
  a.Wo = (W + 2 * pad - k) / stride + 1;
  if (in1) SAD_REQUIRE((a.Ho - 1) * ss1 < H1 && (a.Wo - 1) * ss1 < W1, "shortcut source too small");
  a.Cout = Cout;
  a.relu = relu;
  a.M = N * a.Ho * a.Wo;
  a.ablate = (variant >> 8) & 255;  // timing-only ablation bits (tools/convbench.py --ablate)
  a.x4 = (variant & SAD_CONV_FOUR_PRODUCTS) != 0;
  return launch_block_conv(a, dtype, (hipStream_t)stream, variant & 255);
}
