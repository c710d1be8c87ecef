// Prints gd_tiles.h's tile list and geometry for tests/test_decode_tiles_cpu.py, one line per (tile, activation
// image): wr kc xr gd_valid ring_slots half_ring_slots gd_lds
#include <cstdio>

#include "../gd_tiles.h"

int main() {
  using namespace die::gd;
  const int tiles[][2] = {
#define GD_TILE(WR, KC) {WR, KC},
      GD_TILES(GD_TILE)
#undef GD_TILE
  };
  const int images[] = {16, 32, 64, 128};
  for (const auto& t : tiles)
    for (int xr : images) {
      const int s = ring_slots(t[0], xr, t[1]);
      std::printf("%d %d %d %d %d %d %zu\n", t[0], t[1], xr, (int)gd_valid(t[0], xr, t[1]), s,
                  half_ring_slots(t[0], xr, t[1]), gd_lds(t[0], xr, t[1], s));
    }
  return 0;
}
