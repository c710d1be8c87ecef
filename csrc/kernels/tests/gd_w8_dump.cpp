// Prints gd_w8.h's geometry for tests/test_w8_cpu.py: "G wr kc xr valid ring_slots lds_bytes" per (tile, image), then
// "O wr kc off(0, 0) off(0, 1) ..." per tile: the byte offset of every (image row, chunk column), row-major.
#include <cstdio>
#include <initializer_list>

#include "../gd_w8.h"

int main() {
  using namespace die::gd::w8;
  const int tiles[][2] = {
#define GD_W8_TILE(WR, KC) {WR, KC},
      GD_W8_TILES(GD_W8_TILE)
#undef GD_W8_TILE
  };
  for (const auto& t : tiles)
    for (int xr : {16, 32})
      std::printf("G %d %d %d %d %d %zu\n", t[0], t[1], xr, (int)valid(t[0], xr, t[1]), ring_slots(t[0], xr, t[1]),
                  lds_bytes(t[0], xr, t[1]));
  for (const auto& t : tiles) {
    std::printf("O %d %d", t[0], t[1]);
    for (int r = 0; r < t[0]; ++r)
      for (int k = 0; k < t[1]; ++k) std::printf(" %d", byte_off(t[0], t[1], r, k));
    std::printf("\n");
  }
}
