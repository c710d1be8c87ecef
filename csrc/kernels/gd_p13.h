// "P13": a lossless 13-bit layout of bf16 weights for the decode GEMM's (128, 128) tile (gemm_decode.hip, the
// P13 form of gd_body; packed by src/ops/p13.py). A bf16 s | e[7:0] | m[6:0] is kept as
//   low byte  (e & 1) << 7 | m                                     raw,
//   sign bit  s,
//   code      4 bits for h = e >> 1: 0 -> h = 0, c = 1..15 -> h = base7 + c   (base7: one per tensor),
// so a tensor whose exponents span <= 30 binades below its top pair (and zeros / denormals / e = 1) is exact.
//
// A K-chunk of a tile (128 image rows x 128 k) is three planes, each in the order the consumer loop reads it:
// wave w takes k in [32 w, 32 w + 32); its lane (fr = lane & 15, kg = lane >> 4) holds, for each of the 8
// 16-row MFMA tiles nt, the 8 weights of image row 16 nt + fr at k = 32 w + 8 kg + 0..7 (the B fragment).
//   low plane  16 KiB: [w][nt / 2][lane] 16 B  = the 8 low bytes of tile nt even, then of nt odd   (ds_read_b128)
//   code plane  8 KiB: [w][nt / 4][lane] 16 B  = one dword of 8 nibbles per tile nt & 3            (ds_read_b128)
//                      nibble 2 i = element i, nibble 2 i + 1 = element 4 + i (i < 4)
//   sign plane  2 KiB: [w][lane] 8 B           = dword nt / 4; element j of tile nt is bit
//                      8 (j & 3) + 7 - (2 (nt & 3) + j / 4): `dword << t & 0x80808080` drops 4 signs on 4 high bytes
// Plain C++17, no HIP constructs: the host compiler reads it too (csrc/kernels/tests/gd_p13_unpack.cpp).
#pragma once

#include <cstdint>

namespace die {
namespace gd {
namespace p13 {

constexpr int WR = 128, KC = 128;            // the one tile with a P13 form
constexpr int LOW_OFF = 0;                   // byte offsets of the planes in a chunk (and in its LDS slot)
constexpr int CODE_OFF = 16384;
constexpr int SIGN_OFF = 24576;
constexpr int CHUNK_BYTES = 26624;           // 13/16 of 128 x 128 x 2; the activation image follows in the slot
constexpr int W_PIECES = 32;                 // LDS-DMA pieces: 16 low + 8 code of 1 KiB (16 B per lane), then
constexpr int SIGN_PIECE0 = 24;              // 8 sign pieces of 256 B (4 B per lane)
constexpr int RING_SLOTS = 4;                // 4 x (26 + 8) KiB within the 144 KiB ring

// byte offset of LDS-DMA piece q (< W_PIECES) in the chunk; lanes follow at 16 B (4 B for the sign pieces)
constexpr int piece_off(int q) { return q < SIGN_PIECE0 ? q * 1024 : SIGN_OFF + (q - SIGN_PIECE0) * 256; }

// what lane `lane` of wave w reads: 16 B of low bytes for tiles (2 j, 2 j + 1), 16 B of codes for tiles
// 4 q .. 4 q + 3, 8 B of signs for all 8 tiles
constexpr int low_read_off(int w, int j, int lane) { return LOW_OFF + ((w * 4 + j) * 64 + lane) * 16; }
constexpr int code_read_off(int w, int q, int lane) { return CODE_OFF + ((w * 2 + q) * 64 + lane) * 16; }
constexpr int sign_read_off(int w, int lane) { return SIGN_OFF + (w * 64 + lane) * 8; }

// where the packer puts the weight at image row r, chunk column k
constexpr int frag_lane(int r, int k) { return ((k % 32) / 8) * 16 + r % 16; }
constexpr int low_byte(int r, int k) {
  return low_read_off(k / 32, r / 32, frag_lane(r, k)) + ((r / 16) & 1) * 8 + k % 8;
}
constexpr int code_dword(int r, int k) {  // byte offset of the dword; the nibble is at code_shift(k)
  return code_read_off(k / 32, r / 64, frag_lane(r, k)) + ((r / 16) & 3) * 4;
}
constexpr int code_shift(int k) { return k % 8 < 4 ? 8 * (k % 8) : 8 * (k % 8 - 4) + 4; }
constexpr int sign_t(int nt, int half) { return 2 * (nt & 3) + half; }  // the shift that aligns a quad of signs
constexpr int sign_dword(int r, int k) { return sign_read_off(k / 32, frag_lane(r, k)) + (r / 64) * 4; }
constexpr int sign_shift(int r, int k) { return 8 * (k % 4) + 7 - sign_t(r / 16, (k % 8) / 4); }

// Four high bytes s << 7 | h from four codes (one per byte, 0..15), the tensor's base7 and a sign dword already
// shifted so that the four signs sit on bits 7 / 15 / 23 / 31. h = c ? base7 + c : 0: per byte (c + 15) >> 4 is
// c != 0, and base7 + 15 <= 127 keeps every byte's sum inside the byte.
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t high4(uint32_t c, uint32_t base7, uint32_t sd) {
  const uint32_t nz = ((c + 0x0f0f0f0fu) >> 4) & 0x01010101u;
  const u16x2 b = {(unsigned short)base7, (unsigned short)base7};
  const uint32_t h = __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, nz) * b + __builtin_bit_cast(u16x2, c));
  return (sd & 0x80808080u) | h;
}
#else
inline uint32_t high4(uint32_t c, uint32_t base7, uint32_t sd) {
  const uint32_t nz = ((c + 0x0f0f0f0fu) >> 4) & 0x01010101u;
  return (sd & 0x80808080u) | (c + nz * base7);
}
#endif

// bytes (lo[i], hi[i]) interleaved: bf16 elements 0, 1 (out[0]) and 2, 3 (out[1]) of a quad
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void zip4(uint32_t lo, uint32_t hi, uint32_t& o0, uint32_t& o1) {
  o0 = __builtin_amdgcn_perm(hi, lo, 0x05010400u);
  o1 = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
}
#else
inline void zip4(uint32_t lo, uint32_t hi, uint32_t& o0, uint32_t& o1) {
  o0 = (lo & 0xffu) | (hi & 0xffu) << 8 | (lo & 0xff00u) << 8 | (hi & 0xff00u) << 16;
  o1 = (lo >> 16 & 0xffu) | (hi >> 16 & 0xffu) << 8 | (lo >> 24) << 16 | (hi >> 24) << 24;
}
#endif

// The B fragment of MFMA tile nt (8 bf16 as 4 dwords) from the lane's reads: lo0 / lo1 the tile's 8 low bytes,
// code its 8 nibbles, sd the sign dword nt / 4.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__
#else
inline
#endif
void unpack8(uint32_t lo0, uint32_t lo1, uint32_t code, uint32_t sd, int nt, uint32_t base7, uint32_t (&out)[4]) {
  const uint32_t h0 = high4(code & 0x0f0f0f0fu, base7, sd << sign_t(nt, 0));
  const uint32_t h1 = high4((code >> 4) & 0x0f0f0f0fu, base7, sd << sign_t(nt, 1));
  zip4(lo0, h0, out[0], out[1]);
  zip4(lo1, h1, out[2], out[3]);
}

}  // namespace p13
}  // namespace gd
}  // namespace die
