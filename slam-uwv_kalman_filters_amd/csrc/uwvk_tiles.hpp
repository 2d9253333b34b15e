// uwvk_tiles.hpp — the 4x4 tile map of the pair kernel's rank-M update
// Sigma~ -= C~ K~^T (uwvk_psp_dev.hpp rankm_tiles), as constexpr functions of
// integers (plain C++17, no HIP): which tile of the packed lower triangle a
// local lane of a 32-lane half owns, where its entries lie, and which lanes
// store which tile position.  tests/cpp/tiles_test.cpp checks this file on the
// CPU.
//
// The DOF x DOF lower triangle in blocks of TB = 4 rows and columns is
// NB (NB + 1) / 2 tiles with NB = ceil(DOF / 4) (26 DOFs: 7 row blocks, 28
// tiles).  Local lane t < NT owns tile (rb, cb), cb <= rb, in row-major order
// of the block triangle: t = rb (rb + 1) / 2 + cb.  Its entry at tile
// position (u, v) is (i, j) = (4 rb + u, 4 cb + v) at packed index
// i (i + 1) / 2 + j: the four entries of a tile row are contiguous.  Lanes
// >= NT take tile 0 for their loads and store nothing.
#pragma once
#include <cstdint>

namespace uwvk {
namespace tiles {

constexpr int TB = 4;  // tile edge

constexpr int tri(int n) { return n * (n + 1) / 2; }
constexpr int row_blocks(int dof) { return (dof + TB - 1) / TB; }
constexpr int num_tiles(int dof) { return tri(row_blocks(dof)); }

// tile t's row and column block
constexpr int tile_rb(int t) {
  int rb = 0;
  while (tri(rb + 1) <= t) rb++;
  return rb;
}
constexpr int tile_cb(int t) { return t - tri(tile_rb(t)); }

// the tile whose entries local lane l loads
constexpr int lane_tile(int dof, int l) { return l < num_tiles(dof) ? l : 0; }
constexpr int lane_rb(int dof, int l) { return tile_rb(lane_tile(dof, l)); }
constexpr int lane_cb(int dof, int l) { return tile_cb(lane_tile(dof, l)); }

// packed index of lane l's tile position (u, v).  Above the diagonal (diagonal
// tiles, v > u) and in rows >= dof (the last row block) this is a later entry
// of the triangle or lies past it: loaded, never stored.
constexpr int entry_index(int dof, int l, int u, int v) {
  return tri(TB * lane_rb(dof, l) + u) + TB * lane_cb(dof, l) + v;
}
// the largest index any lane loads
constexpr int max_load_index(int dof) {
  int m = 0;
  for (int l = 0; l < 32; l++)
    if (entry_index(dof, l, TB - 1, TB - 1) > m) m = entry_index(dof, l, TB - 1, TB - 1);
  return m;
}

// lane l stores its tile position (u, v): a lane with a tile, a row of the
// matrix, on or below the diagonal
constexpr bool stores(int dof, int l, int u, int v) {
  return l < num_tiles(dof) && TB * tile_rb(l) + u < dof && TB * tile_cb(l) + v <= TB * tile_rb(l) + u;
}
// the local lanes (bits 0..31) that store tile position (u, v)
constexpr uint64_t store_mask(int dof, int u, int v) {
  uint64_t m = 0;
  for (int l = 0; l < 32; l++)
    if (stores(dof, l, u, v)) m |= uint64_t(1) << l;
  return m;
}
// the local lanes whose row block (col = false) or column block (col = true)
// has bit b set: the lane's block numbers are put together from these masks
constexpr uint64_t block_bit_mask(int dof, bool col, int b) {
  uint64_t m = 0;
  for (int l = 0; l < 32; l++)
    if (((col ? lane_cb(dof, l) : lane_rb(dof, l)) >> b) & 1) m |= uint64_t(1) << l;
  return m;
}
// bits needed for a block number
constexpr int block_bits(int dof) {
  int n = 0;
  while ((1 << n) < row_blocks(dof)) n++;
  return n;
}

}  // namespace tiles
}  // namespace uwvk
