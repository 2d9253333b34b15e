// delayed_plan_test.cpp — the launch plan of uwvk_pose_run_log_delayed
// (plan_run with delayed flags, csrc/uwvk_plan.hpp) on the CPU: without delayed
// or fix flags it is plan_epochs' plan; an arrival or a latch ends a launch; the
// epoch's FIX launch (fixes and the arrival, one launch) comes after its EFFORTS
// launch and before its LATCH launch, a track record last; pdec is carried from
// piece to piece; a per-epoch restatement of the rule over seeded random flag
// sets and track strides; the plan of a dense handle; and the argument check
// delayed_events.  Exit 0 = all checks hold.
#include <random>

#include "plan_check.hpp"

static void expect(const std::vector<uint32_t>& f, const std::vector<uint32_t>& fx, const std::vector<uint32_t>& dl,
                   const EpochFacts& facts, const char* want, int line) {
  expect_plan(plan_run(f.data(), fx.data(), dl.data(), 0, 0, (int64_t)f.size(), facts), want, line);
}
#define EXPECT(f, fx, dl, facts, want) expect(f, fx, dl, facts, want, __LINE__)

static void test_cases() {
  const EpochFacts d = defaults();
  const auto plain = flags(120, IMU), nofix = flags(120, 0);
  // the internal bits lie outside UWVK_FIX_*: a FIX launch's mask holds both
  CHECK((ARR & (XY | Z | GEO)) == 0 && (LAT & (XY | Z | GEO)) == 0 && ARR != LAT && ARR && LAT);
  EXPECT(plain, nofix, flags(120, 0), d, "PAIR[0,120)pd pdec=1");
  // a latch on the first and on the last epoch
  EXPECT(plain, nofix, flags(120, 0, {{0, LAT}}), d, "PAIR[0,1)pd LATCH(0) PAIR[1,120)pd pdec=1");
  EXPECT(plain, nofix, flags(120, 0, {{119, LAT}}), d, "PAIR[0,120)pd LATCH(119) pdec=1");
  // a latch one epoch before an arrival
  EXPECT(plain, nofix, flags(120, 0, {{58, LAT}, {59, ARR}}), d,
         "PAIR[0,59)pd LATCH(58) PAIR[59,60)pd FIX(59,m=8) PAIR[60,120)pd pdec=1");
  // a latch and an arrival of different rows in one epoch: the arrival first
  EXPECT(plain, nofix, flags(120, 0, {{9, LAT}, {30, ARR | LAT}, {70, ARR}}), d,
         "PAIR[0,10)pd LATCH(9) PAIR[10,31)pd FIX(30,m=8) LATCH(30) PAIR[31,71)pd FIX(70,m=8) PAIR[71,120)pd pdec=1");
  // an arrival on a fix epoch is part of that epoch's one FIX launch
  EXPECT(plain, flags(120, 0, {{59, XY | Z | GEO}}), flags(120, 0, {{59, ARR}}), d,
         "PAIR[0,60)pd FIX(59,m=15) PAIR[60,120)pd pdec=1");
  // a latch on a fix epoch: FIX before LATCH
  EXPECT(plain, flags(120, 0, {{59, XY}}), flags(120, 0, {{59, LAT}}), d,
         "PAIR[0,60)pd FIX(59,m=1) LATCH(59) PAIR[60,120)pd pdec=1");
  // a latch on a BodyEfforts epoch: EFFORTS, (FIX,) LATCH; pdec after the full model
  EXPECT(flags(120, IMU, {{59, E}}), nofix, flags(120, 0, {{59, LAT}, {90, ARR}}), d,
         "PAIR[0,60)pd EFFORTS(59,vo=0) LATCH(59) ONE[60,91) FIX(90,m=8) ONE[91,120) pdec=0");
  EXPECT(flags(120, IMU, {{59, E}}), flags(120, 0, {{59, Z}}), flags(120, 0, {{59, LAT | ARR}}), d,
         "PAIR[0,60)pd EFFORTS(59,vo=0) FIX(59,m=10) LATCH(59) ONE[60,120) pdec=0");
  EXPECT(flags(120, IMU, {{59, E | VO}}), nofix, flags(120, 0, {{59, LAT}, {90, ARR}}), d,
         "PAIR[0,60)pd EFFORTS(59,vo=1) LATCH(59) PAIR[60,91)pd FIX(90,m=8) PAIR[91,120)pd pdec=1");
  // a full BodyEfforts in an earlier piece than the latch: pdec is carried
  EXPECT(flags(120, IMU, {{20, E}}), nofix, flags(120, 0, {{10, LAT}, {59, ARR}}), d,
         "PAIR[0,11)pd LATCH(10) PAIR[11,21)pd EFFORTS(20,vo=0) ONE[21,60) FIX(59,m=8) ONE[60,120) pdec=0");
  // a latch on a pressure epoch
  EXPECT(flags(200, IMU, {{100, P}}), flags(200, 0), flags(200, 0, {{100, LAT}}), d,
         "PAIR[0,100)pd ONE[100,101)pd LATCH(100) PAIR[101,200)pd pdec=1");
  // dof 26 and a handle without the pair kernel
  EpochFacts f = d;
  f.dof = 26, f.q_params_diag = false;
  EXPECT(plain, nofix, flags(120, 0, {{30, LAT}}), f, "PAIR[0,31) LATCH(30) PAIR[31,120) pdec=1");
  f = d, f.batch = 5;
  EXPECT(plain, nofix, flags(120, 0, {{30, ARR}}), f, "ONE[0,31)pd FIX(30,m=8) ONE[31,120)pd pdec=1");
  // first > 0: absolute epochs, the three arrays read at k - first; null arrays
  {
    const auto dl = flags(100, 0, {{48, LAT}, {60, ARR}});
    const auto fx = flags(100, 0, {{60, GEO}});
    const auto fl = flags(100, IMU);
    CHECK(show(plan_run(fl.data(), fx.data(), dl.data(), 0, 1000, 100, d)) ==
          "PAIR[1000,1049)pd LATCH(1048) PAIR[1049,1061)pd FIX(1060,m=12) PAIR[1061,1100)pd pdec=1");
    CHECK(show(plan_run(fl.data(), nullptr, dl.data(), 0, 1000, 100, d)) ==
          "PAIR[1000,1049)pd LATCH(1048) PAIR[1049,1061)pd FIX(1060,m=8) PAIR[1061,1100)pd pdec=1");
    CHECK(show(plan_run(fl.data(), fx.data(), nullptr, 0, 1000, 100, d)) ==
          "PAIR[1000,1061)pd FIX(1060,m=4) PAIR[1061,1100)pd pdec=1");
    CHECK(same(plan_run(fl.data(), nullptr, nullptr, 0, 1000, 100, d), plan_epochs(fl.data(), 1000, 100, d)));
    CHECK(show(plan_run(nullptr, nullptr, nullptr, 0, 7, 0, d)) == "pdec=1");
    EpochFacts g = d;
    g.pdec = false;
    CHECK(show(plan_run(nullptr, nullptr, nullptr, 0, 7, 0, g)) == "pdec=0");
  }
  // calls over adjacent ranges concatenate (a row latched in one, arriving in the next)
  {
    const auto fl = flags(120, IMU, {{59, E | VO}});
    const auto fx = flags(120, 0, {{59, XY}});
    const auto dl = flags(120, 0, {{58, LAT}, {60, ARR}, {89, LAT}});
    for (int64_t every : {0, 30, 45}) {  // with a track too: record epochs 29, 59, ... / 44, 89
      auto part = [&](int64_t a, int64_t n) {
        return show_launches(plan_run(fl.data() + a, fx.data() + a, dl.data() + a, every, a, n, d));
      };
      CHECK(part(0, 60) + part(60, 60) == part(0, 120));
    }
  }
}

// The rule once more, per epoch: an epoch's range ends with a BodyEfforts
// epoch, a fix epoch, an arrival, a latch or a record epoch ((e + 1) % every ==
// 0; every 0: no track); its kernel is plan_epochs' (pair: no pressure, and a
// stretch of kPairMinRun such epochs or the whole range); pd from the state's
// decoupling when the epoch runs; EFFORTS, FIX, LATCH, RECORD after it.
static EpochPlan naive_plan(const std::vector<uint32_t>& fl, const std::vector<uint32_t>& fx,
                            const std::vector<uint32_t>& dl, int64_t every, int64_t first, EpochFacts f) {
  EpochPlan p;
  const int64_t n = (int64_t)fl.size();
  auto rec = [&](int64_t k) { return every > 0 && (first + k + 1) % every == 0; };
  std::vector<int> range_of((size_t)n);
  for (int64_t k = 0, r = 0; k < n; k++) {
    range_of[(size_t)k] = (int)r;
    if ((fl[(size_t)k] & E) || fx[(size_t)k] || dl[(size_t)k] || rec(k)) r++;
  }
  auto in_range = [&](int64_t a, int64_t k) { return a >= 0 && a < n && range_of[(size_t)a] == range_of[(size_t)k]; };
  std::vector<LaunchKind> label((size_t)n, EPOCH_ONE);
  std::vector<int> pd((size_t)n, 0);
  for (int64_t k = 0; k < n; k++) {
    pd[(size_t)k] = runs_pd(f);
    if (runs_pair(f) && !(fl[(size_t)k] & P)) {
      int64_t lo = k, hi = k;
      while (in_range(lo - 1, k) && !(fl[(size_t)lo - 1] & P)) lo--;
      while (in_range(hi + 1, k) && !(fl[(size_t)hi + 1] & P)) hi++;
      const bool whole = !in_range(lo - 1, k) && !in_range(hi + 1, k);
      if (hi - lo + 1 >= 48 || whole) label[(size_t)k] = EPOCH_PAIR;
    }
    if ((fl[(size_t)k] & E) && !(fl[(size_t)k] & VO)) f.pdec = false;
  }
  for (int64_t k = 0; k < n; k++) {
    const size_t i = (size_t)k;
    if (k > 0 && in_range(k - 1, k) && label[i - 1] == label[i]) {
      p.launches.back().count++;
      p.launches.back().ev_any |= fl[i];
    } else {
      p.launches.push_back({label[i], first + k, 1, pd[i], 0, fl[i]});
    }
    if (fl[i] & E) p.launches.push_back({EFFORTS, first + k, 1, 0, (fl[i] & VO) ? 1 : 0, fl[i]});
    if (fx[i] || (dl[i] & ARR)) p.launches.push_back({FIX, first + k, 1, 0, 0, fx[i] | (dl[i] & ARR)});
    if (dl[i] & LAT) p.launches.push_back({LATCH, first + k, 1, 0, 0, LAT});
    if (rec(k)) p.launches.push_back({RECORD, first + k, 1, 0, 0, 0});
  }
  p.pdec = f.pdec;
  return p;
}

// the seeded random logs of plan_test.cpp: zero or null delayed flags change
// nothing, and with zero fix flags too the plan is plan_epochs' exactly; random
// ones, with and without a track, give the per-epoch restatement's
static void test_properties() {
  std::mt19937_64 rng(20261);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  EpochFacts variants[6];
  for (EpochFacts& f : variants) f = defaults();
  variants[1].batch = 7;
  variants[2].pdec = false;
  variants[3].dof = 26, variants[3].q_params_diag = false;
  variants[4].persist = 0;
  variants[5].dof = 26, variants[5].q_simple = false, variants[5].q_params_diag = false;
  const double dens[] = {0.0, 0.002, 0.01, 0.05, 0.3};
  int plans = 0, fixes = 0, latches = 0, records = 0, pairs = 0;
  for (const EpochFacts& f : variants)
    for (int it = 0; it < 400; it++, plans++) {
      const int64_t n = 1 + (int64_t)(rng() % 400), first = (it % 3) ? (int64_t)(rng() % 5000) : 0;
      const double dp = dens[rng() % 5], da = dens[rng() % 5], de = dens[rng() % 5], df = dens[rng() % 5];
      std::vector<uint32_t> fl((size_t)n, IMU), fx((size_t)n, 0u), dl((size_t)n, 0u);
      for (uint32_t& w : fl) {
        if (u01(rng) < dp) w |= P;
        if (u01(rng) < da) w |= A;
        if (u01(rng) < de) w |= (u01(rng) < 0.5) ? E : (E | VO);
      }
      for (uint32_t& w : fx)
        if (u01(rng) < df) w = 1u + (uint32_t)(rng() % 7);
      const EpochPlan base = plan_run(fl.data(), fx.data(), nullptr, 0, first, n, f);
      if (!same(plan_run(fl.data(), fx.data(), dl.data(), 0, first, n, f), base) ||
          !same(plan_run(fl.data(), nullptr, dl.data(), 0, first, n, f), plan_epochs(fl.data(), first, n, f)) ||
          !same(base, naive_plan(fl, fx, dl, 0, first, f))) {
        std::printf("FAIL zero delayed flags, variant %d iteration %d\n", (int)(&f - variants), it);
        g_fail++;
      }
      const double dd = dens[1 + rng() % 4];
      for (uint32_t& w : dl) {
        if (u01(rng) < dd) w |= ARR;
        if (u01(rng) < dd) w |= LAT;
      }
      const int64_t every = (it % 4 == 0) ? 0 : 1 + (int64_t)(rng() % 70);  // no track, or a stride of 1 .. 70
      const EpochPlan p = plan_run(fl.data(), fx.data(), dl.data(), every, first, n, f);
      auto rec = [&](int64_t e) { return every > 0 && (e + 1) % every == 0; };
      // structure: the epoch launches tile the range once in order; per event
      // epoch at most one FIX, one LATCH and one RECORD, in the order EFFORTS, FIX, LATCH, RECORD
      int64_t next = first;
      bool ok = true;
      size_t nfix = 0, nlatch = 0, nrec = 0;
      for (size_t i = 0; i < p.launches.size() && ok; i++) {
        const Launch& l = p.launches[i];
        const size_t k = (size_t)(l.first - first);
        if (l.kind == FIX) {
          nfix++;
          ok = i > 0 && p.launches[i - 1].kind != FIX && p.launches[i - 1].kind != LATCH &&
               p.launches[i - 1].kind != RECORD && l.first == next - 1 && l.count == 1 &&
               l.ev_any == (fx[k] | (dl[k] & ARR)) && l.ev_any != 0 &&
               ((fl[k] & E) != 0) == (p.launches[i - 1].kind == EFFORTS);
        } else if (l.kind == LATCH) {
          nlatch++;
          const LaunchKind before = i > 0 ? p.launches[i - 1].kind : LATCH;
          ok = i > 0 && before != LATCH && before != RECORD && l.first == next - 1 && l.count == 1 && (dl[k] & LAT) &&
               (before == FIX) == ((fx[k] | (dl[k] & ARR)) != 0) && p.launches[i - 1].first + p.launches[i - 1].count - 1 == l.first;
        } else if (l.kind == RECORD) {
          nrec++;
          // the last launch of its epoch: after its LATCH, else its FIX, else its EFFORTS, else the epoch launch
          const LaunchKind before = i > 0 ? p.launches[i - 1].kind : RECORD;
          const LaunchKind want = (dl[k] & LAT) ? LATCH : (fx[k] | (dl[k] & ARR)) ? FIX : (fl[k] & E) ? EFFORTS : EPOCH_ONE;
          ok = i > 0 && l.first == next - 1 && l.count == 1 && rec(l.first) &&
               (want == EPOCH_ONE ? (before == EPOCH_ONE || before == EPOCH_PAIR) : before == want) &&
               p.launches[i - 1].first + p.launches[i - 1].count - 1 == l.first &&
               (i + 1 == p.launches.size() || p.launches[i + 1].kind == EPOCH_ONE || p.launches[i + 1].kind == EPOCH_PAIR);
        } else if (l.kind == EFFORTS) {
          ok = l.first == next - 1;
        } else {
          ok = l.first == next && l.count > 0 && l.kind != EPOCH_DENSE;
          for (int64_t e = l.first; e + 1 < l.first + l.count; e++)
            ok = ok && !fx[(size_t)(e - first)] && !dl[(size_t)(e - first)] && !rec(e);
          next = l.first + l.count;
          pairs += l.kind == EPOCH_PAIR;
        }
      }
      size_t want_fix = 0, want_latch = 0;
      for (size_t k = 0; k < (size_t)n; k++) {
        want_fix += (fx[k] || (dl[k] & ARR)) ? 1 : 0;
        want_latch += (dl[k] & LAT) ? 1 : 0;
      }
      fixes += (int)nfix;
      latches += (int)nlatch;
      records += (int)nrec;
      ok = ok && next == first + n && nfix == want_fix && nlatch == want_latch &&
           (int64_t)nrec == (every > 0 ? track_records(first, n, every) : 0);
      if (!ok || !same(p, naive_plan(fl, fx, dl, every, first, f))) {
        std::printf("FAIL delayed plan property, variant %d iteration %d (every %lld):\n  got   %s\n  naive %s\n",
                    (int)(&f - variants), it, (long long)every, show(p).c_str(),
                    show(naive_plan(fl, fx, dl, every, first, f)).c_str());
        g_fail++;
      }
    }
  CHECK(plans >= 2000 && fixes > 2000 && latches > 2000 && records > 2000 && pairs > 200);
}

// A dense handle (the literal kernels): one fused launch per epoch, then the
// epoch's events in the same order; no EFFORTS launch (the fused epoch holds
// it), host_flags not read, never parameter-decoupled afterwards
static void test_dense() {
  EpochFacts d = defaults();
  d.dense = true;
  const auto fl = flags(12, IMU, {{3, E}, {5, E | VO}, {8, P}});
  const auto fx = flags(12, 0, {{5, XY | Z | GEO}, {11, GEO}});
  const auto dl = flags(12, 0, {{5, ARR | LAT}});
  const char* want =
      "DENSE[0,1) DENSE[1,2) DENSE[2,3) DENSE[3,4) DENSE[4,5) DENSE[5,6) FIX(5,m=15) LATCH(5) REC(5) "
      "DENSE[6,7) DENSE[7,8) DENSE[8,9) DENSE[9,10) DENSE[10,11) DENSE[11,12) FIX(11,m=4) REC(11) pdec=0";
  const EpochPlan p = plan_run(fl.data(), fx.data(), dl.data(), 6, 0, 12, d);
  expect_plan(p, want, __LINE__);
  CHECK(!p.pdec);
  for (const Launch& l : p.launches) CHECK(l.kind != EFFORTS && l.kind != EPOCH_ONE && l.kind != EPOCH_PAIR && l.count == 1);
  expect_plan(plan_run(nullptr, fx.data(), dl.data(), 6, 0, 12, d), want, __LINE__);
  // no events: the epochs alone; first > 0; an empty range
  expect_plan(plan_run(nullptr, nullptr, nullptr, 0, 0, 3, d), "DENSE[0,1) DENSE[1,2) DENSE[2,3) pdec=0", __LINE__);
  expect_plan(plan_run(nullptr, fx.data() + 4, dl.data() + 4, 6, 4, 3, d),
              "DENSE[4,5) DENSE[5,6) FIX(5,m=15) LATCH(5) REC(5) DENSE[6,7) pdec=0", __LINE__);
  expect_plan(plan_run(nullptr, nullptr, nullptr, 6, 7, 0, d), "pdec=0", __LINE__);
  // the same log on a PSP handle: the efforts epochs end launches and have their EFFORTS launch
  expect_plan(plan_run(fl.data(), fx.data(), dl.data(), 6, 0, 12, defaults()),
              "PAIR[0,4)pd EFFORTS(3,vo=0) ONE[4,6) EFFORTS(5,vo=1) FIX(5,m=15) LATCH(5) REC(5) ONE[6,12) FIX(11,m=4) "
              "REC(11) pdec=0",
              __LINE__);
}

// delayed_events on a 10-epoch log with 3 rows, over the range [3, 8): the
// example's flag array and latch list, then each defect alone
static void test_delayed_events() {
  // row r latches after epoch L[r] and arrives at the epoch e with index[e] = r
  const std::vector<int32_t> L = {6, 1, 4}, index = {-1, -1, -1, 1, -1, -1, -1, 2, -1, 0};
  double rows[1] = {0.0};  // stands for the device arrays: tested for null, never read
  uwvk_pose_delayed ok{};
  ok.index = index.data(), ok.latch_epoch = L.data(), ok.xy = rows, ok.latched = rows, ok.n = 3;
  DelayedEvents ev;
  CHECK(delayed_events(&ok, 10, 3, 5, &ev));
  // row 1's latch (epoch 1) and row 0's arrival (epoch 9) lie outside the range
  CHECK((ev.flags == std::vector<uint32_t>{ARR, LAT, 0, LAT, ARR}));
  CHECK((ev.latches == std::vector<std::pair<int64_t, int32_t>>{{4, 2}, {6, 0}}));
  CHECK(delayed_events(&ok, 10, 0, 10, &ev));
  CHECK((ev.flags == std::vector<uint32_t>{0, LAT, 0, ARR, LAT, 0, LAT, ARR, 0, ARR}));
  CHECK((ev.latches == std::vector<std::pair<int64_t, int32_t>>{{1, 1}, {4, 2}, {6, 0}}));
  CHECK(delayed_events(&ok, 10, 8, 0, &ev) && ev.flags.empty() && ev.latches.empty());
  auto with = [](std::vector<int32_t> v, int64_t e, int32_t x) {
    v[(size_t)e] = x;
    return v;
  };
  auto rejected = [&](const uwvk_pose_delayed& d, int64_t first, int64_t count) {
    DelayedEvents out;
    return !delayed_events(&d, 10, first, count, &out);
  };
  uwvk_pose_delayed d = ok;
  // an index below -1 or >= n, at an epoch of the range only
  for (int32_t v : {-2, 3, 1 << 20}) {
    const auto bad = with(index, 5, v);
    d = ok, d.index = bad.data();
    CHECK(rejected(d, 3, 5) && rejected(d, 5, 1) && !rejected(d, 6, 2) && !rejected(d, 3, 2));
  }
  d = ok, d.n = 2;  // row 2, arriving at epoch 7, is gone
  CHECK(rejected(d, 3, 5) && !rejected(d, 3, 4));
  // a latch epoch below -1 or >= epochs, whatever the range; -1 is a caller-filled row
  for (int32_t v : {-2, 10, 1 << 20}) {
    const auto bad = with(L, 2, v);
    d = ok, d.latch_epoch = bad.data();
    CHECK(rejected(d, 3, 5) && rejected(d, 0, 0));
  }
  {
    const auto filled = with(L, 2, -1);
    d = ok, d.latch_epoch = filled.data();
    CHECK(delayed_events(&d, 10, 3, 5, &ev) && (ev.flags == std::vector<uint32_t>{ARR, 0, 0, LAT, ARR}));
  }
  // an arrival at or before its row's latch (row 2 arrives at epoch 7), when the arrival is in the range
  for (int32_t v : {7, 8}) {
    const auto bad = with(L, 2, v);
    d = ok, d.latch_epoch = bad.data();
    CHECK(rejected(d, 3, 5) && rejected(d, 7, 1) && !rejected(d, 3, 4));
  }
  d = ok, d.n = -1;
  CHECK(rejected(d, 3, 5) && rejected(d, 0, 0));
  // n > 0 and a null array, each of the four
  d = ok, d.index = nullptr;
  CHECK(rejected(d, 3, 5) && rejected(d, 0, 0));
  d = ok, d.latch_epoch = nullptr;
  CHECK(rejected(d, 3, 5));
  d = ok, d.xy = nullptr;
  CHECK(rejected(d, 3, 5));
  d = ok, d.latched = nullptr;
  CHECK(rejected(d, 3, 5));
  // n == 0: no arrays needed, no events; an index array is still checked
  d = uwvk_pose_delayed{};
  CHECK(delayed_events(&d, 10, 3, 5, &ev) && (ev.flags == std::vector<uint32_t>(5, 0u)) && ev.latches.empty());
  const std::vector<int32_t> none(10, -1);
  d.index = none.data();
  CHECK(!rejected(d, 0, 10));
  d.index = index.data();
  CHECK(rejected(d, 0, 10));
}

int main() {
  test_cases();
  test_properties();
  test_dense();
  test_delayed_events();
  if (g_fail) std::printf("%d checks failed\n", g_fail);
  else std::printf("delayed_plan_test: ok\n");
  return g_fail ? 1 : 0;
}
