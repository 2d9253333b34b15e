// track_plan_test.cpp — the record cuts of uwvk_pose_run_log_track (plan_run's
// RECORD launches / track_records, csrc/uwvk_plan.hpp) on the CPU, over fixed
// and seeded random (first, count, every) on an all-IMU log: the pieces between
// records tile the range in order, each but possibly the last ends at a record
// epoch, their number is the closed form, and a range split anywhere gives the
// two halves' records one after the other.  Exit 0 = all checks hold.
#include <cstdio>
#include <random>

#include "../../slam-uwv_kalman_filters_amd/csrc/uwvk_plan.hpp"

using namespace uwvk;

static int g_fail = 0;
#define CHECK(c)                                                                                              \
  do {                                                                                                        \
    if (!(c)) {                                                                                               \
      std::printf("FAIL %s:%d: %s (first %lld count %lld every %lld)\n", __FILE__, __LINE__, #c,              \
                  (long long)first, (long long)count, (long long)every);                                      \
      g_fail++;                                                                                               \
    }                                                                                                         \
  } while (0)

// [first, first + count) as plan_run cuts it for the track alone: the epochs
// its launches cover up to and including each RECORD (record), then what is
// left at the range's end without one
struct Piece {
  int64_t first, count;
  bool record;
};
static std::vector<Piece> record_pieces(int64_t first, int64_t count, int64_t every) {
  const std::vector<uint32_t> imu((size_t)count, UWVK_EV_ACC);
  const EpochPlan p = plan_run(imu.data(), nullptr, nullptr, every, first, count,
                               {53, 63, 1, 0, 1, 0, false, true, true, true});  // no pair kernel: one launch per piece
  std::vector<Piece> s;
  int64_t e = first, next = first;  // the open piece is [e, next)
  for (const Launch& l : p.launches) {
    if (l.kind == RECORD) {
      if (l.first != next - 1 || next == e) return {};  // a record not at the end of what ran: no valid cut
      s.push_back({e, next - e, true});
      e = next;
    } else {
      if (l.first != next || l.count <= 0 || (l.kind != EPOCH_ONE && l.kind != EPOCH_PAIR)) return {};
      next += l.count;
    }
  }
  if (next > e) s.push_back({e, next - e, false});
  return s;
}

// the record epochs of a range, from its segments
static std::vector<int64_t> records(int64_t first, int64_t count, int64_t every) {
  std::vector<int64_t> r;
  for (const Piece& s : record_pieces(first, count, every))
    if (s.record) r.push_back(s.first + s.count - 1);
  return r;
}

static void check_case(int64_t first, int64_t count, int64_t every) {
  const std::vector<Piece> segs = record_pieces(first, count, every);
  int64_t e = first, nrec = 0;
  for (size_t k = 0; k < segs.size(); k++) {
    const Piece& s = segs[k];
    CHECK(s.first == e && s.count > 0);  // in order, no gap, no empty segment
    e = s.first + s.count;
    if (s.record) nrec++;
    // every segment ends at a record epoch, the last possibly at the range's end
    CHECK(s.record == (e % every == 0));
    CHECK(s.record || k + 1 == segs.size());
    // no record epoch inside a segment
    for (int64_t q = s.first; q + 1 < e; q++) CHECK((q + 1) % every != 0);
  }
  CHECK(e == first + count);
  CHECK(count > 0 || segs.empty());
  CHECK(nrec == track_records(first, count, every));
  CHECK(nrec == (first + count) / every - first / every);
  // naive count
  int64_t naive = 0;
  for (int64_t q = first; q < first + count; q++) naive += (q + 1) % every == 0;
  CHECK(nrec == naive);
  // composition: the records of [first, cut) then [cut, first + count)
  const std::vector<int64_t> whole = records(first, count, every);
  for (int64_t cut = first; cut <= first + count; cut++) {
    std::vector<int64_t> two = records(first, cut - first, every);
    for (int64_t r : records(cut, first + count - cut, every)) two.push_back(r);
    CHECK(two == whole);
  }
}

int main() {
  // every = 1, every > count, first not a multiple of every, count = 0, a range
  // that ends on / one short of / one past a record epoch
  const int64_t fixed[][3] = {{0, 120, 25}, {0, 10, 1},  {7, 10, 1},  {0, 5, 9},   {3, 5, 9},  {4, 5, 9},
                              {13, 40, 7},  {13, 0, 7},  {0, 0, 1},   {70, 50, 25}, {0, 24, 25}, {0, 25, 25},
                              {0, 26, 25},  {24, 1, 25}, {25, 1, 25}, {1999, 1, 1000}};
  for (const auto& c : fixed) check_case(c[0], c[1], c[2]);
  std::mt19937_64 rng(20240611);
  for (int k = 0; k < 3000; k++) {
    const int64_t first = (int64_t)(rng() % 300), count = (int64_t)(rng() % 200);
    const int64_t every = 1 + (int64_t)(rng() % (k % 3 == 0 ? 8 : 260));
    check_case(first, count, every);
  }
  // large epochs: no 32-bit arithmetic
  {
    const int64_t first = (int64_t(1) << 33) + 5, count = 1000, every = 300;
    const std::vector<Piece> segs = record_pieces(first, count, every);
    CHECK(!segs.empty() && segs.front().first == first && segs.back().first + segs.back().count == first + count);
    CHECK((int64_t)records(first, count, every).size() == track_records(first, count, every));
  }
  // track_args_valid, the track argument check of every run_log entry point: a
  // stride <= 0, no output array, and the capacity one below / exactly at the
  // records of a range that does not start at 0 ([13, 53) with every 7: after epochs 13, 20, .. 48)
  {
    const int64_t first = 13, count = 40, every = 7, need = track_records(first, count, every);
    CHECK(need == 6);
    CHECK(!track_args_valid(0, need, true, first, count));
    CHECK(!track_args_valid(-every, need, true, first, count));
    CHECK(!track_args_valid(every, need, false, first, count));
    CHECK(!track_args_valid(every, need - 1, true, first, count));
    CHECK(track_args_valid(every, need, true, first, count));
    CHECK(track_args_valid(every, 0, true, first, 0));  // an empty range needs no room
  }
  std::printf("track plan: %s\n", g_fail ? "FAILED" : "ok");
  return g_fail ? 1 : 0;
}
