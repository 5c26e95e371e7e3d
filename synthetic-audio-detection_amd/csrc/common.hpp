// common.hpp -- shared helpers for libsad (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <type_traits>

#include "../../include/sad.h"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;

namespace sad {

// thread-local last error (sad_last_error)
void set_error(const std::string& msg);

#define SAD_CHECK_HIP(expr)                                                        \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) {                                                        \
      ::sad::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));         \
      return SAD_ERR_HIP;                                                          \
    }                                                                              \
  } while (0)

#define SAD_REQUIRE(cond, msg)                                                     \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      ::sad::set_error(std::string("argument check failed: ") + (msg));            \
      return SAD_ERR_ARG;                                                          \
    }                                                                              \
  } while (0)

// an integer A/B switch from the environment (callers keep the value in a static)
inline int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}

// host fp32 -> bf16 round-to-nearest-even (no NaN inputs on this path)
inline u16 f2bf_host(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  u += 0x7FFF + ((u >> 16) & 1);
  return (u16)(u >> 16);
}

__device__ __forceinline__ u16 f2bf(float f) {
  __bf16 b = (__bf16)f;  // v_cvt_pk_bf16_f32, RNE
  return __builtin_bit_cast(u16, b);
}
__device__ __forceinline__ float bf2f(u16 h) { return __uint_as_float(((uint32_t)h) << 16); }

// ---- the 16-bit element formats.  The kernels' element type E (or T) is u16
// for bf16 and f16 for IEEE binary16 (SAD_F16): same bytes, same layouts, same
// MFMA shape; what differs is the MFMA's type, the packing and the unpacking.
typedef _Float16 f16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <typename E>
constexpr bool is_f16_v = std::is_same<E, f16>::value;
constexpr float F16_MAX = 65504.f;
inline bool is16(int dtype) { return dtype == SAD_BF16 || dtype == SAD_F16; }  // 2-byte plain layouts
inline int dtype_bytes(int dtype) { return is16(dtype) ? 2 : 4; }             // (split-bf16: 4 B per value)
// host fp32 -> fp16 round-to-nearest-even (the plans refuse what would overflow)
inline u16 f2h_host(float f) {
  const _Float16 h = (_Float16)f;
  u16 u;
  __builtin_memcpy(&u, &h, 2);
  return u;
}
// fp16 stores saturate: a finite value past +-65504 is stored as +-65504, never
// as inf.  Every kernel that stores fp16 sets the wave's fp16-overflow clamp
// mode (MODE.FP16_OVFL) once at entry: v_cvt_pk_f16_f32 / v_cvt_f16_f32 then
// clamp an overflowing result themselves, at no cost per value (a v_med3_f32
// per value in front of the conversion cost 1.0 % of the fp16 step:
// profiles/fp16_sat_ab.txt).  The mode keeps a true infinity: an
// fp32 value that is already inf or NaN is stored as such, which finite inputs
// and the plans' weight check rule out (65504^2 K is far inside fp32).
template <typename E>
__device__ __forceinline__ void f16_kernel_entry() {
  if constexpr (is_f16_v<E>) __builtin_amdgcn_s_setreg(1 | (23 << 6), 1);  // hwreg(HW_REG_MODE, 23, 1): FP16_OVFL
}
// float -> 16-bit element (RNE; fp16 saturating) and back
template <typename E>
__device__ __forceinline__ u16 to16(float f) {
  if constexpr (is_f16_v<E>)
    return __builtin_bit_cast(u16, (_Float16)f);
  else
    return f2bf(f);
}
template <typename E>
__device__ __forceinline__ float from16(u16 h) {
  if constexpr (is_f16_v<E>)
    return (float)__builtin_bit_cast(_Float16, h);
  else
    return bf2f(h);
}
// two floats -> one packed fp16 pair: v_cvt_pk_f16_f32 (RNE, saturating under f16_kernel_entry)
__device__ __forceinline__ uint32_t pk_f16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){lo, hi}, f16x2));
}
// the halves of a packed pair as floats, one VALU each: bf16 is a shift / a
// mask; fp16 is v_cvt_f32_f16 (the high half through SDWA WORD_1)
template <typename E>
__device__ __forceinline__ float lo16(uint32_t q) {
  if constexpr (is_f16_v<E>)
    return (float)__builtin_bit_cast(f16x2, q)[0];
  else
    return __uint_as_float(q << 16);
}
template <typename E>
__device__ __forceinline__ float hi16(uint32_t q) {
  if constexpr (is_f16_v<E>)
    return (float)__builtin_bit_cast(f16x2, q)[1];
  else
    return __uint_as_float(q & 0xFFFF0000u);
}

// torchvision bilinear sample (align_corners=False, source index clamped at 0;
// the antialias filter reduces to this for upsampling) of an `in`-long axis at
// output pixel o of an `on`-long axis: (i0, i1, weight of i1).  resize_kernel
// (frontend.hip) and crop_resize_kernel (train.hip) both go through bl_axis and
// bl_lerp, whose fused operations are spelled out: left to the compiler, the two
// kernels contracted the same expressions differently and Resize((512,512)) came
// out an ulp apart between them (tests/test_gpu_image_prep.py).
__device__ __forceinline__ void bl_axis(int o, int in, int on, int& i0, int& i1, float& l) {
  const float sc = (float)in / on;
  float f = __builtin_fmaf(sc, o + 0.5f, -0.5f);
  f = f < 0.f ? 0.f : f;
  i0 = min((int)floorf(f), in - 1);
  i1 = min(i0 + 1, in - 1);
  l = fminf(fmaxf(f - i0, 0.f), 1.f);
}
// (1 - ly) ((1 - lx) p00 + lx p01) + ly ((1 - lx) p10 + lx p11); exact for lx = ly = 0
__device__ __forceinline__ float bl_lerp(float p00, float p01, float p10, float p11, float lx, float ly) {
  const float ux = 1.f - lx, uy = 1.f - ly;
  const float top = __builtin_fmaf(lx, p01, ux * p00), bot = __builtin_fmaf(lx, p11, ux * p10);
  return __builtin_fmaf(ly, bot, uy * top);
}

// Bijective XCD-aware block remap (cdna_hip_programming.md 5, T1): consecutive
// logical tiles land on the same XCD (blocks b, b+8, ... share one).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

}  // namespace sad
