// Device helpers shared by the two W8A16 decode GEMMs (gemm_decode_w8.hip and its grouped form
// gemm_decode_w8_grouped.hip): the LDS-DMA piece, the counted wait, the e4m3 -> bf16 fragment conversion and the
// SiLU * up epilogue. One definition, so the two kernels cannot drift apart. HIP device code only.
#pragma once

#include "common.h"

namespace die {
namespace gd {
namespace w8 {

constexpr int NTH = 256;  // threads per workgroup

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void global_cvoid;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f4;

template <int AUX>
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((global_cvoid*)src, (lds_void*)lds_wave_base, 16, 0, AUX);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// the high halves of two floats as a bf16 pair (a low): exact for e4m3 values
__device__ __forceinline__ uint32_t hi2(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}

// 8 e4m3 bytes (element i = byte i of lo, element 4 + i = byte i of hi) -> the 8 bf16 of a B fragment
__device__ __forceinline__ bf16x8 cvt8(uint32_t lo, uint32_t hi) {
  const f32x2_t a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2_t c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return __builtin_bit_cast(bf16x8, uint4{hi2(a[0], a[1]), hi2(b[0], b[1]), hi2(c[0], c[1]), hi2(d[0], d[1])});
}

// silu(v) * u = v / (1 + e^-v) * u; where the fast exp overflows (-v > 88.72) 1 + e^-v == e^-v in fp32 and the
// result is (v u) e^v with the exponent lifted by 64 and taken back by an exact power of two. COPIED from
// gemm_decode.hip's silu_mul (that file and its object stay as they are): keep the two in sync, both branches
__device__ __forceinline__ float silu_mul(float v, float u) {
  const float e = __expf(-v);
  float r = v / (1.f + e) * u;
  if (__float_as_uint(e) == 0x7f800000u)
    r = (v * u) * __builtin_amdgcn_exp2f(__builtin_fmaf(v, 0x1.715476p+0f, 64.f)) * 0x1p-64f;
  return r;
}

// the counted wait of the ring: `after` chunks (of per_wave pieces each) were issued after the one about to be read
// and stay in flight; S is the ring's depth
template <int S, int PER_WAVE>
__device__ __forceinline__ void wait_chunk(int after) {
  switch (after) {
    case 7: wait_vm<(S > 7 ? 7 : 0) * PER_WAVE>(); break;
    case 6: wait_vm<(S > 6 ? 6 : 0) * PER_WAVE>(); break;
    case 5: wait_vm<(S > 5 ? 5 : 0) * PER_WAVE>(); break;
    case 4: wait_vm<(S > 4 ? 4 : 0) * PER_WAVE>(); break;
    case 3: wait_vm<(S > 3 ? 3 : 0) * PER_WAVE>(); break;
    case 2: wait_vm<(S > 2 ? 2 : 0) * PER_WAVE>(); break;
    case 1: wait_vm<PER_WAVE>(); break;
    default: wait_vm<0>();
  }
}

}  // namespace w8
}  // namespace gd
}  // namespace die
