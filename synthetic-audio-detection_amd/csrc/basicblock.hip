// basicblock.hip -- one ResNet BasicBlock on the block-conv kernels: its fold
// and its launches, shared by the ResNet-18 plan (api.hip) and the generic
// BasicBlock plans (resnet.hip).  Host code only.
//   T = relu(conv3x3/s(X))
//   Y = relu(conv3x3(T) + shortcut)   the folded 1x1/s downsample as extra K
//       columns over X; the identity as an epilogue residual or as identity K
//       columns (identity_shortcut_is_res, block.hip)
//   bf16 / fp16 layer1 blocks (64 -> 64) as one fused kernel (variant 40, l1block.hip)
#include <vector>

#include "common.hpp"
#include "kernels.hpp"

namespace sad {

int fold_conv(const float* const* q, int cout, int cin, int k, int dtype, void** w_out, float** b_out, int* ld_out,
              const float* const* ds, int ds_cin, bool identity, const char* name) {
  std::vector<double> sc, sh, scd, shd;
  fold_bn(q[1], q[2], q[3], q[4], cout, sc, sh);
  if (ds) fold_bn(ds[1], ds[2], ds[3], ds[4], cout, scd, shd);
  const int kk = k * k * cin;
  const int extra = ds ? ds_cin : (identity ? cout : 0);
  const int ld = kk + extra;
  std::vector<double> w((size_t)cout * ld, 0.0);
  std::vector<float> b(cout);
  const float* W = q[0];
  for (int o = 0; o < cout; ++o) {
    for (int c = 0; c < cin; ++c)
      for (int t = 0; t < k * k; ++t)  // timm [Cout][Cin][KH][KW] -> [Cout][KH][KW][Cin]
        w[(size_t)o * ld + (size_t)t * cin + c] = (double)W[((size_t)o * cin + c) * k * k + t] * sc[o];
    double bias = sh[o];
    if (ds) {
      for (int c = 0; c < ds_cin; ++c) w[(size_t)o * ld + kk + c] = (double)ds[0][(size_t)o * ds_cin + c] * scd[o];
      bias += shd[o];
    } else if (identity) {
      w[(size_t)o * ld + kk + o] = 1.0;  // exact in bf16
    }
    b[o] = (float)bias;
  }
  *ld_out = ld;
  int rc;
  if (dtype == SAD_F16 && (rc = check_f16_range(w, b, name))) return rc;
  if ((rc = upload_typed(w_out, w, dtype, ld))) return rc;
  return upload((void**)b_out, b);
}

int fold_basic_block(const float* const* q1, const float* const* q2, const float* const* qd, int cin, int cout,
                     int stride, int dtype, BasicBlock& out, const char* name) {
  out.cin = cin;
  out.cout = cout;
  out.stride = stride;
  out.has_ds = qd != nullptr;
  int rc;
  const std::string n1 = std::string(name) + ".conv1", n2 = std::string(name) + (qd ? ".conv2 + downsample" : ".conv2");
  if ((rc = fold_conv(q1, cout, cin, 3, dtype, &out.w1, &out.b1, &out.w1_ld, nullptr, 0, false, n1.c_str()))) return rc;
  return fold_conv(q2, cout, cout, 3, dtype, &out.w2, &out.b2, &out.w2_ld, qd, cin, !qd, n2.c_str());
}

void free_basic_block(BasicBlock& b) {
  (void)hipFree(b.w1);
  (void)hipFree(b.b1);
  (void)hipFree(b.w2);
  (void)hipFree(b.b2);
  b.w1 = b.w2 = nullptr;
  b.b1 = b.b2 = nullptr;
}

int run_basic_block(const BasicBlock& blk, int dtype, const void* x, void* tmp, void* y, int64_t n, int H,
                    hipStream_t s, float* pool_out, bool* pooled, bool bracket) {
  const int C = blk.cin, Ho = H / blk.stride;
  if (is16(dtype) && blk.stride == 1 && !blk.has_ds && C == 64 && blk.cout == 64 && H % 16 == 0 && l1_fused()) {
    // layer1: the whole BasicBlock as one kernel (variant 40)
    L1BlockArgs f{};
    f.x = (const u16*)x;
    f.out = (u16*)y;
    f.N = (int)n;
    f.H = f.W = H;
    f.w1 = (const u16*)blk.w1;
    f.w1_ld = blk.w1_ld;
    f.b1 = blk.b1;
    f.w2 = (const u16*)blk.w2;
    f.w2_ld = blk.w2_ld;  // 576 + the identity's 64 K columns (not read: the residual is the patch centre)
    f.b2 = blk.b2;
    f.h16 = dtype == SAD_F16;
    return bracket ? timed_l1block(f, s, 2.0 * 2.0 * n * H * H * 64 * 576.0) : launch_l1block(f, s);
  }
  int rc;
  BlockConvArgs a{};
  a.in0 = x;
  a.in0_pstride = C;
  a.N = (int)n;
  a.H = a.W = H;
  a.Cin = C;
  a.KH = a.KW = 3;
  a.stride = blk.stride;
  a.pad = 1;
  a.wt = blk.w1;
  a.bias = blk.b1;
  a.out = tmp;
  a.out_pstride = blk.cout;
  a.Ho = a.Wo = Ho;
  a.Cout = blk.cout;
  a.relu = 1;
  a.M = n * Ho * Ho;
  const double fl1 = 2.0 * a.M * a.Cout * 9.0 * C;
  if ((rc = bracket ? timed_block_conv(a, dtype, s, fl1) : launch_block_conv(a, dtype, s))) return rc;
  BlockConvArgs b2 = a;
  b2.in0 = tmp;
  b2.in0_pstride = blk.cout;
  b2.H = b2.W = Ho;
  b2.Cin = blk.cout;
  b2.stride = 1;
  b2.wt_ld = blk.w2_ld;
  if (identity_shortcut_is_res(dtype, 0, C, blk.cout, blk.stride, blk.has_ds, Ho)) {
    b2.res = x;
    b2.res_pstride = C;
  } else {
    b2.in1 = x;
    b2.in1_pstride = C;
    b2.H1 = b2.W1 = H;
    b2.Cin1 = C;
    b2.ss1 = blk.stride;
  }
  b2.wt = blk.w2;
  b2.bias = blk.b2;
  b2.out = y;
  if (pool_out && block_conv_can_pool(b2, dtype)) {
    b2.pool_out = pool_out;
    b2.out = nullptr;
    *pooled = true;
  }
  // algorithmic work: conv2, plus the 1x1 downsample when there is one (not the identity)
  const double fl2 = 2.0 * b2.M * b2.Cout * (9.0 * blk.cout + (blk.stride != 1 ? (double)C : 0.0));
  return bracket ? timed_block_conv(b2, dtype, s, fl2) : launch_block_conv(b2, dtype, s);
}

}  // namespace sad
