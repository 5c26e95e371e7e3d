// rwconv.hpp -- helpers of the resident-weight conv kernels (l1block.hip,
// l2conv.hip): weights held in AGPRs for a whole launch, so the MFMAs that read
// them are inline asm (hipcc only places MFMA A/B operands in VGPRs); packed
// bf16 conversion and ReLU; LDS access by byte address and the LDS-DMA piece
// with a pinned descriptor; compile-time loops.
#pragma once
#include <utility>

#include "common.hpp"

namespace sad {

typedef unsigned int l1b_v4 __attribute__((ext_vector_type(4)));
typedef unsigned int l1b_v2 __attribute__((ext_vector_type(2)));
// E: the element type (u16 = bf16, f16 = fp16, SAD_F16): the MFMA's type.
// acc (VGPR) [+]= w (AGPR) . b (VGPR).  hipcc places MFMA A/B operands only
// in VGPRs, and the 288 weight registers of both convs do not fit there next
// to the accumulators: the weights live in AGPRs, the MFMA is inline asm.
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_a0(f32x4& acc, const l1b_v4& w, const uint4& b) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "a"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  }
}
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_a(f32x4& acc, const l1b_v4& w, const uint4& b) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  }
}
// acc = c + w . b (the first K-step: C = the bias)
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_ac(f32x4& acc, const l1b_v4& w, const uint4& b, const f32x4& c) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3"
                 : "=&v"(acc)
                 : "a"(w), "v"(__builtin_bit_cast(l1b_v4, b)), "v"(c));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3"
                 : "=&v"(acc)
                 : "a"(w), "v"(__builtin_bit_cast(l1b_v4, b)), "v"(c));
  }
}
// the same with the weights in VGPRs (the AGPR file holds 256 of the 288)
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_v0(f32x4& acc, const l1b_v4& w, const uint4& b) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  }
}
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_v(f32x4& acc, const l1b_v4& w, const uint4& b) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(__builtin_bit_cast(l1b_v4, b)));
  }
}
// the same with the fragment as a native vector (HIP's uint4 is a struct)
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_a(f32x4& acc, const l1b_v4& w, const l1b_v4& b) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "a"(w), "v"(b));
  }
}
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_ac(f32x4& acc, const l1b_v4& w, const l1b_v4& b, const f32x4& c) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %3" : "=&v"(acc) : "a"(w), "v"(b), "v"(c));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %3" : "=&v"(acc) : "a"(w), "v"(b), "v"(c));
  }
}
template <typename E = u16>
__device__ __forceinline__ void l1b_mfma_v(f32x4& acc, const l1b_v4& w, const l1b_v4& b) {
  if constexpr (is_f16_v<E>) {
    asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
  } else {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
  }
}
// two floats -> packed bf16 pair (RNE), one v_cvt_pk_bf16_f32
typedef __bf16 l1b_bf2 __attribute__((ext_vector_type(2)));
typedef float l1b_f2 __attribute__((ext_vector_type(2)));
// relu of an asm MFMA result (fmaxf would first canonicalise it: one more VALU)
__device__ __forceinline__ float l1b_relu(float x) {
  float r;
  asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
  return r;
}
// ReLU of a packed bf16 pair: as int16, negative bf16 values (and -0) are
// negative, so max(x, 0) per half is relu (= relu before the rounding); fp16
// has the same sign-magnitude order, so the same instruction serves it
__device__ __forceinline__ uint32_t l1b_relu2(uint32_t x) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, 0" : "=v"(r) : "v"(x));
  return r;
}
// the same against a scalar floor per half: 0 = ReLU, 0x8000 (the least int16)
// = none, so a conv whose ReLU is a launch argument decides it once, in an SGPR
__device__ __forceinline__ uint32_t l1b_relu2s(uint32_t x, int floor2) {
  uint32_t r;
  asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(x), "s"(floor2));
  return r;
}
template <typename E = u16>
__device__ __forceinline__ uint32_t l1b_pk(float lo, float hi) {
  if constexpr (is_f16_v<E>) return pk_f16(lo, hi);  // v_cvt_pk_f16_f32, saturating
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((l1b_f2){lo, hi}, l1b_bf2));
}

// LDS access by byte address (the kernels' lane constants carry the LDS base, so
// no base is added in front of a read; a constant added to `ad` becomes the
// instruction's immediate offset)
// T: a native vector type (l1b_v4, l1b_v2, f32x4) -- HIP's uint4 / uint2 are
// structs, which the optimiser takes apart into 4-B accesses
template <typename T>
__device__ __forceinline__ T l1b_ld(int ad) {
  return *(const __attribute__((address_space(3))) T*)(unsigned)ad;
}
template <typename T>
__device__ __forceinline__ void l1b_st(int ad, const T& v) {
  *(__attribute__((address_space(3))) T*)(unsigned)ad = v;
}

// One LDS-DMA piece (16 B per lane from buffer offset voff to LDS [dst + OFF +
// 16 lane]) with M0 formed in the statement as a scalar base plus an
// immediate, and the descriptor passed as one 128-bit scalar value.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
template <int OFF>
__device__ __forceinline__ void l1b_dma16(const l1b_v4& rsrc, int voff, unsigned dst) {
  asm volatile(
      "s_add_u32 m0, %1, %3\n\t"
      "s_nop 0\n\t"
      "buffer_load_dwordx4 %0, %2, 0 offen lds"
      :
      : "v"(voff), "s"(dst), "s"(rsrc), "n"(OFF)
      : "memory", "m0", "scc");
}
#pragma clang diagnostic pop

template <typename F, int... I>
__device__ __forceinline__ void l1b_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void l1b_for(F&& f) {
  l1b_for_impl(f, std::make_integer_sequence<int, N>{});
}


}  // namespace sad
