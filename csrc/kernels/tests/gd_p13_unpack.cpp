// Host replay of the P13 decode-GEMM consumer loop for tests/test_p13_cpu.py: reads packed K-chunks (gd_p13.h,
// CHUNK_BYTES each), makes every (wave, lane, MFMA tile) read at the offsets the kernel uses, unpacks with the
// kernel's own arithmetic and writes each chunk's image [128 rows][128 k] as bf16 bits.
//   gd_p13_unpack <packed.bin> <base7> <image.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../gd_p13.h"

int main(int argc, char** argv) {
  using namespace die::gd::p13;
  if (argc != 4) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<unsigned char> in;
  unsigned char buf[4096];
  for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + n);
  std::fclose(f);
  if (in.empty() || in.size() % CHUNK_BYTES) return 4;
  const uint32_t base7 = (uint32_t)std::atoi(argv[2]);
  const size_t chunks = in.size() / CHUNK_BYTES;
  std::vector<uint16_t> img(chunks * WR * KC);
  auto rd = [](const unsigned char* p) {
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
  };
  for (size_t c = 0; c < chunks; ++c) {
    const unsigned char* ch = in.data() + c * CHUNK_BYTES;
    for (int w = 0; w < 4; ++w)
      for (int lane = 0; lane < 64; ++lane) {
        const int fr = lane & 15, kg = lane >> 4;
        for (int nt = 0; nt < 8; ++nt) {
          const unsigned char* lo = ch + low_read_off(w, nt / 2, lane) + (nt & 1) * 8;
          const uint32_t code = rd(ch + code_read_off(w, nt / 4, lane) + (nt & 3) * 4);
          const uint32_t sd = rd(ch + sign_read_off(w, lane) + (nt / 4) * 4);
          uint32_t out[4];
          unpack8(rd(lo), rd(lo + 4), code, sd, nt, base7, out);
          uint16_t* dst = &img[(c * WR + 16 * nt + fr) * KC + 32 * w + 8 * kg];
          for (int i = 0; i < 4; ++i) {
            dst[2 * i] = (uint16_t)(out[i] & 0xffffu);
            dst[2 * i + 1] = (uint16_t)(out[i] >> 16);
          }
        }
      }
  }
  f = std::fopen(argv[3], "wb");
  if (!f) return 5;
  std::fwrite(img.data(), 2, img.size(), f);
  std::fclose(f);
  return 0;
}
