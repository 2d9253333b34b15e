// bcast_test.cpp — csrc/uwvk_bcast.hpp on the CPU: a 64-lane wave emulated on
// the host.  rep16's row algebra (one v_permlane16_swap_b32 per dword) and the
// (copy, N) map of a source lane: for every source lane s < 32, every lane of
// either half must receive the value of lane s of ITS OWN half through
// row_newbcast:N of the copy the map names -- with all 64 lanes active and with
// one half masked off (the other half's lanes then keep their registers).
// Then each site's actual source lists (the Cholesky columns' too: their fused
// form was measured and not kept).  Plain C++17, no HIP.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../slam-uwv_kalman_filters_amd/csrc/uwvk_bcast.hpp"

using namespace uwvk::bcast;

static int fails = 0;
#define EXPECT(c, ...)                  \
  do {                                  \
    if (!(c)) {                         \
      fails++;                          \
      if (fails < 20) {                 \
        std::printf("FAIL %s: ", #c);   \
        std::printf(__VA_ARGS__);       \
        std::printf("\n");              \
      }                                 \
    }                                   \
  } while (0)

// the map at compile time, as the kernel uses it
static_assert(copy_of(0) == 0 && n_of(0) == 0, "lane 0");
static_assert(copy_of(15) == 0 && n_of(15) == 15, "lane 15");
static_assert(copy_of(16) == 1 && n_of(16) == 0, "lane 16");
static_assert(copy_of(17) == 1 && n_of(17) == 1, "lane 17");
static_assert(copy_of(28) == 1 && n_of(28) == 12, "lane 28");
static_assert(copy_of(31) == 1 && n_of(31) == 15, "lane 31");
static_assert(!needs_hi(0, 1, 15) && !needs_hi(0, 1, 6), "Cholesky columns: lower row only");
static_assert(needs_hi(0, 2, 15) && !needs_hi(0, 2, 6), "Delta_j spans both rows, Dz_j does not");
static_assert(needs_hi(0, 1, 18) && !needs_hi(0, 1, 12), "P: M K = 18 reaches lanes 16, 17; 12 does not");

// lane l's value: distinct per lane and per register, so a wrong lane, row or half shows
static uint64_t val(int l, int tag) { return 0x1000u * (uint64_t)tag + 0x10u * (uint64_t)l + 7u; }

static void check_source(int s, unsigned long long exec, const char* what) {
  uint64_t v[kWave], lo[kWave], hi[kWave];
  for (int l = 0; l < kWave; l++) v[l] = val(l, 1);
  rep16(v, lo, hi, exec);
  const Src m = src_of(s);
  EXPECT(m.n >= 0 && m.n < kRow && (m.copy == 0 || m.copy == 1), "%s: s = %d -> (%d, %d)", what, s, m.copy, m.n);
  for (int l = 0; l < kWave; l++) {
    if (!((exec >> l) & 1)) continue;  // a lane outside exec executes nothing
    const uint64_t got = row_newbcast(m.copy ? hi : lo, l, m.n);
    const uint64_t want = v[(l / kHalf) * kHalf + s];
    EXPECT(got == want, "%s: s = %d, lane %d got %llx want %llx", what, s, l, (unsigned long long)got,
           (unsigned long long)want);
  }
}

int main() {
  // rep16's row algebra, all lanes active
  {
    uint64_t v[kWave], lo[kWave], hi[kWave];
    for (int l = 0; l < kWave; l++) v[l] = val(l, 2);
    rep16(v, lo, hi);
    for (int l = 0; l < kWave; l++) {
      const int h = l / kHalf, i = l % kRow;
      EXPECT(lo[l] == v[h * kHalf + i], "lo lane %d", l);          // [row0, row0, row2, row2]
      EXPECT(hi[l] == v[h * kHalf + kRow + i], "hi lane %d", l);   // [row1, row1, row3, row3]
    }
  }
  // one half masked off: its registers stay what they were (copies of v), the active half is whole
  const unsigned long long masks[3] = {~0ull, 0x00000000FFFFFFFFull, 0xFFFFFFFF00000000ull};
  for (unsigned long long exec : masks) {
    uint64_t v[kWave], lo[kWave], hi[kWave];
    for (int l = 0; l < kWave; l++) v[l] = val(l, 3);
    rep16(v, lo, hi, exec);
    for (int l = 0; l < kWave; l++)
      if (!((exec >> l) & 1)) EXPECT(lo[l] == v[l] && hi[l] == v[l], "masked lane %d changed", l);
    // every source lane of a half, every destination lane
    for (int s = 0; s < kHalf; s++) check_source(s, exec, "all sources");
  }
  // the sites' source lists (uwvk_psp_dev.hpp)
  for (unsigned long long exec : masks) {
    for (int c = 0; c < 15; c++) check_source(c, exec, "pchol K = 15: L[c][J] in lane c");
    for (int c = 0; c < 6; c++) check_source(c, exec, "pchol K = 6");
    for (int j = 0; j < 15; j++) check_source(2 * j, exec, "predict: Delta_j in lane 2j");
    for (int j = 0; j < 6; j++) check_source(2 * j, exec, "update: Dz_j in lane 2j");
    for (int M : {3, 2})
      for (int i = 0; i < M; i++)
        for (int j = 0; j < 6; j++) check_source(i * 6 + j, exec, "update: P[i][j] in lane i K + j");
  }
  // the lists that need only the lower row's copy stay below lane 16
  for (int c = 0; c < 15; c++) EXPECT(copy_of(c) == 0 && n_of(c) == c, "column %d", c);
  for (int j = 0; j < 6; j++) EXPECT(copy_of(2 * j) == 0, "Dz %d", j);
  EXPECT(copy_of(16) == 1 && copy_of(17) == 1, "P lanes 16, 17 from the upper row's copy");
  // a wrong map must fail this emulation (the check has teeth): read lane 17 from the lower copy
  {
    uint64_t v[kWave], lo[kWave], hi[kWave];
    for (int l = 0; l < kWave; l++) v[l] = val(l, 4);
    rep16(v, lo, hi);
    EXPECT(row_newbcast(lo, 40, 1) != v[32 + 17], "lower copy must not hold lane 17");
    EXPECT(row_newbcast(hi, 40, 1) == v[32 + 17], "upper copy holds lane 17 of the lane's own half");
    EXPECT(row_newbcast(v, 56, 1) != v[32 + 1], "without rep16 the upper row reads its own lane 1");
  }
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("bcast map ok\n");
  return 0;
}
