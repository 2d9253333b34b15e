// visual_plan_test.cpp — the launch plan of uwvk_pose_run_log_visual (plan_run
// with visual flags, csrc/uwvk_plan.hpp) on the CPU: an epoch with a visual row
// ends a launch; its VISUAL launch comes after the epoch's FIX launch and
// before its LATCH launch, a track record last; pdec is false from the first
// VISUAL launch on (no pair or pd launch after it); without visual flags the
// plan is today's plan_run, launch for launch; calls over adjacent ranges
// concatenate; a dense handle gets the same event launches after its per-epoch
// launches; a per-epoch restatement over seeded random flag sets.
// Exit 0 = all checks hold.
#include <random>

#include "plan_check.hpp"

// plan_check.hpp's show() with the VISUAL launch as "VIS(e)"
static std::string vshow(const EpochPlan& p) {
  std::string s;
  EpochPlan one;
  one.pdec = false;
  for (const Launch& l : p.launches) {
    if (l.kind == VISUAL) {
      s += "VIS(" + std::to_string(l.first) + ") ";
    } else {
      one.launches.assign(1, l);
      s += show_launches(one);
    }
  }
  return s + "pdec=" + std::to_string((int)p.pdec);
}
static std::string vshow_launches(const EpochPlan& p) {
  const std::string t = vshow(p);
  return t.substr(0, t.rfind("pdec="));
}

static void expect(const EpochPlan& p, const char* want, int line) {
  const std::string got = vshow(p);
  if (got != want) {
    std::printf("FAIL line %d:\n  got  %s\n  want %s\n", line, got.c_str(), want);
    g_fail++;
  }
}
#define EXPECT(p, want) expect(p, want, __LINE__)

static void test_cases() {
  const EpochFacts d = defaults();
  const auto plain = flags(120, IMU), none = flags(120, 0);
  // appended: the earlier kinds keep their values
  CHECK(EPOCH_ONE == 0 && EPOCH_PAIR == 1 && EPOCH_DENSE == 2 && EFFORTS == 3 && FIX == 4 && LATCH == 5 &&
        RECORD == 6 && VISUAL == 7);
  // a fix, an arrival, a visual row, a latch and a record on one epoch: FIX, VISUAL, LATCH, RECORD
  EXPECT(plan_run(plain.data(), flags(120, 0, {{59, XY}}).data(), flags(120, 0, {{59, ARR | LAT}}).data(), 60, 0, 120,
                  d, flags(120, 0, {{59, 1}}).data()),
         "PAIR[0,60)pd FIX(59,m=9) VIS(59) LATCH(59) REC(59) ONE[60,120) REC(119) pdec=0");
  // a visual row alone; pdec false from it on: the general kernel afterwards
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 120, d, flags(120, 0, {{59, 1}}).data()),
         "PAIR[0,60)pd VIS(59) ONE[60,120) pdec=0");
  // the flag is "has a row": any non-zero value
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 120, d, flags(120, 0, {{59, 7}}).data()),
         "PAIR[0,60)pd VIS(59) ONE[60,120) pdec=0");
  // adjacent visual epochs
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 120, d, flags(120, 0, {{11, 1}, {12, 1}}).data()),
         "PAIR[0,12)pd VIS(11) ONE[12,13) VIS(12) ONE[13,120) pdec=0");
  // a visual row on the first and on the last epoch of the range
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 120, d, flags(120, 0, {{0, 1}}).data()),
         "PAIR[0,1)pd VIS(0) ONE[1,120) pdec=0");
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 120, d, flags(120, 0, {{119, 1}}).data()),
         "PAIR[0,120)pd VIS(119) pdec=0");
  // on a BodyEfforts epoch: EFFORTS, FIX, VISUAL; the velocity-only form leaves pdec, the visual row ends it
  EXPECT(plan_run(flags(120, IMU, {{59, E | VO}}).data(), flags(120, 0, {{59, Z}}).data(), nullptr, 0, 0, 120, d,
                  flags(120, 0, {{59, 1}}).data()),
         "PAIR[0,60)pd EFFORTS(59,vo=1) FIX(59,m=2) VIS(59) ONE[60,120) pdec=0");
  // a later fix, arrival and latch run on the general kernel
  EXPECT(plan_run(plain.data(), flags(120, 0, {{80, GEO}}).data(), flags(120, 0, {{70, LAT}, {90, ARR}}).data(), 0, 0,
                  120, d, flags(120, 0, {{30, 1}}).data()),
         "PAIR[0,31)pd VIS(30) ONE[31,71) LATCH(70) ONE[71,81) FIX(80,m=4) ONE[81,91) FIX(90,m=8) ONE[91,120) pdec=0");
  // dof 26: its pair kernel does not depend on pdec
  EpochFacts f = d;
  f.dof = 26, f.q_params_diag = false;
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 120, f, flags(120, 0, {{30, 1}}).data()),
         "PAIR[0,31) VIS(30) PAIR[31,120) pdec=0");
  // an odd batch: the one-instance kernel, pd until the first row
  f = d, f.batch = 3;
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 0, 24, f, flags(24, 0, {{5, 1}, {11, 1}, {12, 1}, {23, 1}}).data()),
         "ONE[0,6)pd VIS(5) ONE[6,12) VIS(11) ONE[12,13) VIS(12) ONE[13,24) VIS(23) pdec=0");
  // first > 0: absolute epochs, the visual array read at k - first
  EXPECT(plan_run(plain.data(), nullptr, nullptr, 0, 1000, 100, d, flags(100, 0, {{48, 1}}).data()),
         "PAIR[1000,1049)pd VIS(1048) ONE[1049,1100) pdec=0");
  // an empty range keeps pdec
  EXPECT(plan_run(nullptr, nullptr, nullptr, 0, 7, 0, d, nullptr), "pdec=1");
  (void)none;
}

// no VISUAL flag: today's plan_run, launch for launch (null and all-zero
// arrays), over the seeded random logs of delayed_plan_test.cpp; random visual
// flags: the plan is that of the same log cut after every visual epoch, each
// piece planned without visual flags, pdec false after the first VISUAL
static void test_properties() {
  std::mt19937_64 rng(20262);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  EpochFacts variants[6];
  for (EpochFacts& f : variants) f = defaults();
  variants[1].batch = 7;
  variants[2].pdec = false;
  variants[3].dof = 26, variants[3].q_params_diag = false;
  variants[4].persist = 0;
  variants[5].dense = true;
  const double dens[] = {0.0, 0.002, 0.01, 0.05, 0.3};
  int plans = 0, visuals = 0, after = 0;
  for (const EpochFacts& f : variants)
    for (int it = 0; it < 300; it++, plans++) {
      const int64_t n = 1 + (int64_t)(rng() % 300), first = (it % 3) ? (int64_t)(rng() % 5000) : 0;
      const double dp = dens[rng() % 5], de = dens[rng() % 5], df = dens[rng() % 5], dd = dens[rng() % 5];
      std::vector<uint32_t> fl((size_t)n, IMU), fx((size_t)n, 0u), dl((size_t)n, 0u), vs((size_t)n, 0u);
      for (uint32_t& w : fl) {
        if (u01(rng) < dp) w |= P;
        if (u01(rng) < de) w |= (u01(rng) < 0.5) ? E : (E | VO);
      }
      for (uint32_t& w : fx)
        if (u01(rng) < df) w = 1u + (uint32_t)(rng() % 7);
      for (uint32_t& w : dl) {
        if (u01(rng) < dd) w |= ARR;
        if (u01(rng) < dd) w |= LAT;
      }
      const int64_t every = (it % 4 == 0) ? 0 : 1 + (int64_t)(rng() % 70);
      const EpochPlan base = plan_run(fl.data(), fx.data(), dl.data(), every, first, n, f);
      if (!same(plan_run(fl.data(), fx.data(), dl.data(), every, first, n, f, nullptr), base) ||
          !same(plan_run(fl.data(), fx.data(), dl.data(), every, first, n, f, vs.data()), base)) {
        std::printf("FAIL zero visual flags, variant %d iteration %d\n", (int)(&f - variants), it);
        g_fail++;
      }
      const double dv = dens[1 + rng() % 4];
      for (uint32_t& w : vs)
        if (u01(rng) < dv) w = 1u;
      const EpochPlan p = plan_run(fl.data(), fx.data(), dl.data(), every, first, n, f, vs.data());
      // the restatement: the cut run's calls, the VISUAL launch put in after the piece's FIX
      EpochPlan want;
      EpochFacts g = f;
      if (g.dense) g.pdec = false;
      want.pdec = g.pdec;
      for (int64_t a = 0; a < n;) {
        int64_t b = a;
        while (b < n && !vs[(size_t)b]) b++;
        const bool cut = b < n;
        if (cut) b++;
        EpochPlan piece = plan_run(fl.data() + a, fx.data() + a, dl.data() + a, every, first + a, b - a, g);
        if (cut) {
          // the event launches of the piece's last epoch: LATCH and RECORD come after the VISUAL launch
          size_t at = piece.launches.size();
          while (at > 0 && (piece.launches[at - 1].kind == LATCH || piece.launches[at - 1].kind == RECORD) &&
                 piece.launches[at - 1].first == first + b - 1)
            at--;
          piece.launches.insert(piece.launches.begin() + (std::ptrdiff_t)at, Launch{VISUAL, first + b - 1, 1, 0, 0, 0});
          piece.pdec = false;
          visuals++;
        }
        want.launches.insert(want.launches.end(), piece.launches.begin(), piece.launches.end());
        g.pdec = want.pdec = piece.pdec;
        a = b;
      }
      bool ok = same(p, want);
      // nothing parameter-decoupled and no 53-DOF pair launch after the first VISUAL
      bool seen = false;
      for (const Launch& l : p.launches) {
        if (seen && (l.pd || (l.kind == EPOCH_PAIR && f.dof == 53))) ok = false;
        if (seen && (l.kind == EPOCH_ONE || l.kind == EPOCH_PAIR)) after++;
        seen = seen || l.kind == VISUAL;
      }
      if (seen && p.pdec) ok = false;
      if (!ok) {
        std::printf("FAIL visual plan property, variant %d iteration %d (every %lld):\n  got  %s\n  want %s\n",
                    (int)(&f - variants), it, (long long)every, vshow(p).c_str(), vshow(want).c_str());
        g_fail++;
      }
    }
  CHECK(plans >= 1800 && visuals > 2000 && after > 2000);
}

// calls over adjacent ranges (the first ending on an event epoch, so that no
// epoch launch is split) give the concatenation of their launches
static void test_split() {
  const EpochFacts d = defaults();
  const auto fl = flags(120, IMU, {{59, E | VO}});
  const auto fx = flags(120, 0, {{59, XY}});
  const auto dl = flags(120, 0, {{58, LAT}, {60, ARR}, {89, LAT}});
  const auto vs = flags(120, 0, {{20, 1}, {59, 1}, {60, 1}, {119, 1}});
  for (int64_t every : {0, 30, 45})
    for (int64_t cut : {21, 59, 60, 61}) {  // after an event epoch: no epoch launch is split
      EpochFacts g = d;
      auto part = [&](int64_t a, int64_t n) {
        const EpochPlan p = plan_run(fl.data() + a, fx.data() + a, dl.data() + a, every, a, n, g, vs.data() + a);
        g.pdec = p.pdec;  // the handle carries pdec from call to call
        return vshow_launches(p);
      };
      std::string parts = part(0, cut);
      parts += part(cut, 120 - cut);
      g = d;
      CHECK(parts == part(0, 120));
    }
}

// A dense handle: its per-epoch launches, then the same event launches
static void test_dense() {
  EpochFacts d = defaults();
  d.dense = true;
  const auto fx = flags(8, 0, {{5, XY | Z | GEO}});
  const auto dl = flags(8, 0, {{5, ARR | LAT}});
  const auto vs = flags(8, 0, {{2, 1}, {5, 1}, {7, 1}});
  EXPECT(plan_run(nullptr, fx.data(), dl.data(), 6, 0, 8, d, vs.data()),
         "DENSE[0,1) DENSE[1,2) DENSE[2,3) VIS(2) DENSE[3,4) DENSE[4,5) DENSE[5,6) FIX(5,m=15) VIS(5) LATCH(5) REC(5) "
         "DENSE[6,7) DENSE[7,8) VIS(7) pdec=0");
}

int main() {
  test_cases();
  test_properties();
  test_split();
  test_dense();
  if (g_fail) std::printf("%d checks failed\n", g_fail);
  else std::printf("visual_plan_test: ok\n");
  return g_fail ? 1 : 0;
}
