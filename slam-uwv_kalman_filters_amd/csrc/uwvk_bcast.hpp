// uwvk_bcast.hpp — the lane map of the pair kernel's fused half-wide
// broadcasts (uwvk_psp_dev.hpp rep16 / fmac_bc), as constexpr functions of
// integers and a host model of the two instructions involved (plain C++17, no
// HIP).  tests/cpp/bcast_test.cpp checks this file on the CPU.
//
// An instance owns a 32-lane half of the wave: two DPP rows of 16 lanes.  A
// DPP row_newbcast:N operand gives every lane of a row its own row's lane N, so
// a value of local lane s < 32 reaches all 32 lanes of its half only from a
// register in which the source's row stands in BOTH rows of the half.  rep16
// makes the two such registers with one v_permlane16_swap_b32 per dword
// (x.row1 <-> y.row0, x.row3 <-> y.row2, with x = y = a copy of v):
//   lo = [v.row0, v.row0, v.row2, v.row2]   (each half's lower row, twice)
//   hi = [v.row1, v.row1, v.row3, v.row3]   (each half's upper row, twice)
// and local lane s is read as row_newbcast:(s & 15) of lo (s < 16) or hi.
#pragma once

namespace uwvk {
namespace bcast {

constexpr int kRow = 16;   // lanes of a DPP row
constexpr int kHalf = 32;  // lanes of an instance
constexpr int kWave = 64;

// where local lane s of a half is read from: copy 0 = rep16's lo, 1 = its hi;
// n = the row_newbcast lane
struct Src {
  int copy, n;
};
constexpr Src src_of(int s) { return Src{(s / kRow) & 1, s % kRow}; }
constexpr int copy_of(int s) { return src_of(s).copy; }
constexpr int n_of(int s) { return src_of(s).n; }
// sources of a strided list (lane s0 + stride k, k < count) that need the hi copy
constexpr bool needs_hi(int s0, int stride, int count) {
  for (int k = 0; k < count; k++)
    if (copy_of(s0 + stride * k)) return true;
  return false;
}

// ---- host model of a 64-lane register (one T per lane) ----
// v_permlane16_swap_b32 x, y: x.row1 <-> y.row0 and x.row3 <-> y.row2; a lane
// outside exec keeps its value (both lanes of an exchange lie in one half)
template <class T>
void permlane16_swap(T (&x)[kWave], T (&y)[kWave], unsigned long long exec = ~0ull) {
  for (int pass = 0; pass < 2; pass++)
    for (int i = 0; i < kRow; i++) {
      const int lx = pass * kHalf + kRow + i, ly = pass * kHalf + i;
      if (!((exec >> lx) & 1) || !((exec >> ly) & 1)) continue;
      const T t = x[lx];
      x[lx] = y[ly];
      y[ly] = t;
    }
}
template <class T>
void rep16(const T (&v)[kWave], T (&lo)[kWave], T (&hi)[kWave], unsigned long long exec = ~0ull) {
  for (int l = 0; l < kWave; l++) lo[l] = hi[l] = v[l];
  permlane16_swap(lo, hi, exec);
}
// the value lane l sees through row_newbcast:n of src
template <class T>
T row_newbcast(const T (&src)[kWave], int l, int n) {
  return src[(l / kRow) * kRow + n];
}

}  // namespace bcast
}  // namespace uwvk
