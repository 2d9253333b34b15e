// The 4x4 tile map of the pair kernel's rank-M update (csrc/uwvk_tiles.hpp) on
// the CPU: every packed entry of the lower triangle is stored by exactly one
// (lane, u, v) under the store masks, nothing else is stored, every load stays
// inside the instance's LDS block, and the lane's block numbers put together
// from the bit masks are the map's.  Checked at the kernel's 26 DOFs and at
// other sizes (10, 4, 13, 28), so that the map is not right only at the shape
// it was written for.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../slam-uwv_kalman_filters_amd/csrc/uwvk_tiles.hpp"

namespace T = uwvk::tiles;

static int fails = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      fails++;                                 \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
    }                                          \
  } while (0)

// smem_doubles: the doubles of the instance's LDS block (PspSmem<dof>: the
// packed triangle, the stored mean, the staging area), from the caller
static void check(int dof, int smem_doubles) {
  const int np = T::tri(dof), nt = T::num_tiles(dof);
  CHECK(nt <= 32, "dof %d: %d tiles", dof, nt);
  CHECK(T::row_blocks(dof) <= (1 << T::block_bits(dof)), "dof %d: block bits", dof);
  std::vector<int> stored(np, 0);
  for (int l = 0; l < 32; l++) {
    // block numbers from the bit masks
    int rb = 0, cb = 0;
    for (int b = 0; b < T::block_bits(dof); b++) {
      rb |= (int)((T::block_bit_mask(dof, false, b) >> l) & 1) << b;
      cb |= (int)((T::block_bit_mask(dof, true, b) >> l) & 1) << b;
    }
    CHECK(rb == T::lane_rb(dof, l) && cb == T::lane_cb(dof, l), "dof %d lane %d: blocks (%d, %d)", dof, l, rb, cb);
    CHECK(cb <= rb && rb < T::row_blocks(dof), "dof %d lane %d: tile (%d, %d)", dof, l, rb, cb);
    if (l < nt) CHECK(T::tri(rb) + cb == l, "dof %d lane %d: tile order", dof, l);
    for (int u = 0; u < T::TB; u++)
      for (int v = 0; v < T::TB; v++) {
        const int e = T::entry_index(dof, l, u, v);
        const int i = T::TB * rb + u, j = T::TB * cb + v;
        CHECK(e == T::tri(i) + j, "dof %d lane %d (%d, %d): index %d", dof, l, u, v, e);
        CHECK(e >= 0 && e < smem_doubles, "dof %d lane %d (%d, %d): load index %d >= %d", dof, l, u, v, e, smem_doubles);
        CHECK(e <= T::max_load_index(dof), "dof %d: max_load_index", dof);
        const bool st = (T::store_mask(dof, u, v) >> l) & 1;
        CHECK(st == T::stores(dof, l, u, v), "dof %d lane %d (%d, %d): mask against predicate", dof, l, u, v);
        if (!st) continue;
        CHECK(l < nt, "dof %d: lane %d without a tile stores (%d, %d)", dof, l, u, v);
        CHECK(e < np, "dof %d lane %d (%d, %d): stores index %d >= NP %d", dof, l, u, v, e, np);
        CHECK(j <= i && i < dof, "dof %d lane %d: stores entry (%d, %d)", dof, l, i, j);
        if (e < np) stored[e]++;
      }
  }
  for (int u = 0; u < T::TB; u++)
    for (int v = 0; v < T::TB; v++)
      CHECK((T::store_mask(dof, u, v) >> 32) == 0, "dof %d (%d, %d): mask beyond 32 local lanes", dof, u, v);
  for (int i = 0; i < dof; i++)
    for (int j = 0; j <= i; j++)
      CHECK(stored[T::tri(i) + j] == 1, "dof %d: entry (%d, %d) stored %d times", dof, i, j, stored[T::tri(i) + j]);
}

int main() {
  // PspSmem<26>: 351 + 27 stored means + 115 staging doubles; smaller layouts
  // with the triangle and the staging area alone
  check(26, 351 + 27 + 115);
  check(10, T::tri(10) + 115);
  check(4, T::tri(4) + 115);
  check(13, T::tri(13) + 115);
  check(28, T::tri(28) + 115);
  // compile-time use, as the kernel's
  static_assert(T::num_tiles(26) == 28 && T::row_blocks(26) == 7, "26 DOFs: 28 tiles");
  static_assert(T::max_load_index(26) == T::tri(27) + 27, "the last row block's rows 26 and 27 are loaded");
  static_assert(T::store_mask(26, 0, 0) == 0x0FFFFFFFull, "lanes 28..31 store nothing");
  static_assert(T::tile_rb(27) == 6 && T::tile_cb(27) == 6 && T::tile_rb(0) == 0, "tile order");
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("tiles ok\n");
  return 0;
}
