// Prints gd_w4.h's geometry for tests/test_w4_cpu.py: "G wr kc xr valid ring_slots lds_bytes slot_bytes" per (tile,
// image), then per tile "O wr kc ..." the byte offset in the chunk's record of every (image row, chunk column),
// row-major, "N wr kc ..." the nibble of each, and "S wr kc ..." the offset of every (image row, block)'s scale byte.
#include <cstdio>
#include <initializer_list>

#include "../gd_w4.h"

int main() {
  using namespace die::gd::w4;
  const int tiles[][2] = {
#define GD_W4_TILE(WR, KC) {WR, KC},
      GD_W4_TILES(GD_W4_TILE)
#undef GD_W4_TILE
  };
  for (const auto& t : tiles)
    for (int xr : {16, 32})
      std::printf("G %d %d %d %d %d %zu %d\n", t[0], t[1], xr, (int)valid(t[0], xr, t[1]), ring_slots(t[0], xr, t[1]),
                  lds_bytes(t[0], xr, t[1]), slot_bytes(t[0], xr, t[1]));
  for (const auto& t : tiles) {
    std::printf("O %d %d", t[0], t[1]);
    for (int r = 0; r < t[0]; ++r)
      for (int k = 0; k < t[1]; ++k) std::printf(" %d", byte_off(t[0], t[1], r, k));
    std::printf("\nN %d %d", t[0], t[1]);
    for (int r = 0; r < t[0]; ++r)
      for (int k = 0; k < t[1]; ++k) std::printf(" %d", nibble_of(k));
    std::printf("\nS %d %d", t[0], t[1]);
    for (int r = 0; r < t[0]; ++r)
      for (int b = 0; b < t[1] / BLOCK; ++b) std::printf(" %d", scale_off(t[0], t[1], r, b));
    std::printf("\n");
  }
}
