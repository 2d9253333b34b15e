// fix_plan_test.cpp — the launch plan of uwvk_pose_run_log_fixes (plan_run with
// fix flags, csrc/uwvk_plan.hpp) on the CPU: without fix flags it is
// plan_epochs' plan; a fix epoch ends a launch and is followed by one FIX
// launch, after the epoch's EFFORTS launch; a fix leaves pd / pair on; track
// records compose with fixes; a per-epoch restatement of the rule over seeded
// random flag sets; and the argument check fixes_valid.  Exit 0 = all checks hold.
#include <random>

#include "plan_check.hpp"

static void expect(const std::vector<uint32_t>& f, const std::vector<uint32_t>& fx, const EpochFacts& facts,
                   const char* want, int line) {
  expect_plan(plan_run(f.data(), fx.data(), nullptr, 0, 0, (int64_t)f.size(), facts), want, line);
}
#define EXPECT(f, fx, facts, want) expect(f, fx, facts, want, __LINE__)

static void test_cases() {
  const EpochFacts d = defaults();
  const auto plain = flags(120, IMU);
  EXPECT(plain, flags(120, 0), d, "PAIR[0,120)pd pdec=1");
  // the first epoch, the last epoch, two adjacent epochs
  EXPECT(plain, flags(120, 0, {{0, XY}}), d, "PAIR[0,1)pd FIX(0,m=1) PAIR[1,120)pd pdec=1");
  EXPECT(plain, flags(120, 0, {{119, GEO}}), d, "PAIR[0,120)pd FIX(119,m=4) pdec=1");
  EXPECT(plain, flags(120, 0, {{59, XY | Z | GEO}, {60, Z}}), d,
         "PAIR[0,60)pd FIX(59,m=7) PAIR[60,61)pd FIX(60,m=2) PAIR[61,120)pd pdec=1");
  // on a BodyEfforts epoch: EFFORTS before FIX; the full model turns pd off for
  // the pieces after it, the fix does not
  EXPECT(flags(120, IMU, {{59, E}}), flags(120, 0, {{59, XY}, {90, Z}}), d,
         "PAIR[0,60)pd EFFORTS(59,vo=0) FIX(59,m=1) ONE[60,91) FIX(90,m=2) ONE[91,120) pdec=0");
  EXPECT(flags(120, IMU, {{59, E | VO}}), flags(120, 0, {{59, XY}, {90, Z}}), d,
         "PAIR[0,60)pd EFFORTS(59,vo=1) FIX(59,m=1) PAIR[60,91)pd FIX(90,m=2) PAIR[91,120)pd pdec=1");
  // efforts in an earlier piece than the fix: pdec is carried from piece to piece
  EXPECT(flags(120, IMU, {{20, E}}), flags(120, 0, {{10, XY}, {59, XY}}), d,
         "PAIR[0,11)pd FIX(10,m=1) PAIR[11,21)pd EFFORTS(20,vo=0) ONE[21,60) FIX(59,m=1) ONE[60,120) pdec=0");
  // on a pressure epoch: the piece [0, 101) has the runs [0, 100) and the pressure epoch
  EXPECT(flags(200, IMU, {{100, P}}), flags(200, 0, {{100, Z}}), d,
         "PAIR[0,100)pd ONE[100,101)pd FIX(100,m=2) PAIR[101,200)pd pdec=1");
  // dof 26 and a handle without the pair kernel
  EpochFacts f = d;
  f.dof = 26, f.q_params_diag = false;
  EXPECT(plain, flags(120, 0, {{30, XY}}), f, "PAIR[0,31) FIX(30,m=1) PAIR[31,120) pdec=1");
  f = d, f.batch = 5;
  EXPECT(plain, flags(120, 0, {{30, XY}}), f, "ONE[0,31)pd FIX(30,m=1) ONE[31,120)pd pdec=1");
  // first > 0: absolute epochs, both flag arrays read at k - first; a null fix array
  {
    const auto fx = flags(100, 0, {{48, GEO}});
    const auto fl = flags(100, IMU);
    CHECK(show(plan_run(fl.data(), fx.data(), nullptr, 0, 1000, 100, d)) ==
          "PAIR[1000,1049)pd FIX(1048,m=4) PAIR[1049,1100)pd pdec=1");
    CHECK(same(plan_run(fl.data(), nullptr, nullptr, 0, 1000, 100, d), plan_epochs(fl.data(), 1000, 100, d)));
    CHECK(show(plan_run(nullptr, nullptr, nullptr, 0, 7, 0, d)) == "pdec=1");
    EpochFacts g = d;
    g.pdec = false;
    CHECK(show(plan_run(nullptr, nullptr, nullptr, 0, 7, 0, g)) == "pdec=0");
  }
}

// the launches of a tracked run with fixes, as run_log queues them: the
// record ("REC(e)") after its epoch's launches
static std::string tracked(const std::vector<uint32_t>& fl, const std::vector<uint32_t>& fx, int64_t first,
                           int64_t count, int64_t every, EpochFacts f) {
  return show_launches(plan_run(fl.data() + first, fx.data() + first, nullptr, every, first, count, f));
}

static void test_track() {
  const EpochFacts d = defaults();
  const auto fl = flags(120, IMU, {{59, E | VO}});
  const auto fx = flags(120, 0, {{29, XY}, {59, XY | Z}, {60, Z}});
  // the fix of a record epoch comes before its record, after the EFFORTS launch
  CHECK(tracked(fl, fx, 0, 120, 30, d) ==
        "PAIR[0,30)pd FIX(29,m=1) REC(29) PAIR[30,60)pd EFFORTS(59,vo=1) FIX(59,m=3) REC(59) "
        "PAIR[60,61)pd FIX(60,m=2) PAIR[61,90)pd REC(89) PAIR[90,120)pd REC(119) ");
  // calls over adjacent ranges concatenate
  CHECK(tracked(fl, fx, 0, 60, 30, d) + tracked(fl, fx, 60, 60, 30, d) == tracked(fl, fx, 0, 120, 30, d));
}

// The rule once more, per epoch: an epoch's range ends with a BodyEfforts epoch
// or a fix epoch; its kernel is plan_epochs' (pair: no pressure, and a stretch
// of kPairMinRun such epochs or the whole range); pd from the state's
// decoupling when the epoch runs; EFFORTS then FIX after the epoch.
static EpochPlan naive_plan(const std::vector<uint32_t>& fl, const std::vector<uint32_t>& fx, int64_t first,
                            EpochFacts f) {
  EpochPlan p;
  const int64_t n = (int64_t)fl.size();
  std::vector<int> range_of((size_t)n);
  for (int64_t k = 0, r = 0; k < n; k++) {
    range_of[(size_t)k] = (int)r;
    if ((fl[(size_t)k] & E) || fx[(size_t)k]) r++;
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
    if (k > 0 && in_range(k - 1, k) && label[(size_t)k - 1] == label[(size_t)k]) {
      p.launches.back().count++;
      p.launches.back().ev_any |= fl[(size_t)k];
    } else {
      p.launches.push_back({label[(size_t)k], first + k, 1, pd[(size_t)k], 0, fl[(size_t)k]});
    }
    if (fl[(size_t)k] & E) p.launches.push_back({EFFORTS, first + k, 1, 0, (fl[(size_t)k] & VO) ? 1 : 0, fl[(size_t)k]});
    if (fx[(size_t)k]) p.launches.push_back({FIX, first + k, 1, 0, 0, fx[(size_t)k]});
  }
  p.pdec = f.pdec;
  return p;
}

// the seeded random logs of plan_test.cpp: zero fix flags give plan_epochs'
// plan exactly; random fix flags give the per-epoch restatement's
static void test_properties() {
  std::mt19937_64 rng(20260);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  EpochFacts variants[6];
  for (EpochFacts& f : variants) f = defaults();
  variants[1].batch = 7;
  variants[2].pdec = false;
  variants[3].dof = 26, variants[3].q_params_diag = false;
  variants[4].persist = 0;
  variants[5].dof = 26, variants[5].q_simple = false, variants[5].q_params_diag = false;
  const double dens[] = {0.0, 0.002, 0.01, 0.05, 0.3};
  int plans = 0, fixes = 0, pairs = 0;
  for (const EpochFacts& f : variants)
    for (int it = 0; it < 400; it++, plans++) {
      const int64_t n = 1 + (int64_t)(rng() % 400), first = (it % 3) ? (int64_t)(rng() % 5000) : 0;
      const double dp = dens[rng() % 5], da = dens[rng() % 5], de = dens[rng() % 5];
      std::vector<uint32_t> fl((size_t)n, IMU);
      for (uint32_t& w : fl) {
        if (u01(rng) < dp) w |= P;
        if (u01(rng) < da) w |= A;
        if (u01(rng) < de) w |= (u01(rng) < 0.5) ? E : (E | VO);
      }
      const EpochPlan base = plan_epochs(fl.data(), first, n, f);
      const std::vector<uint32_t> none((size_t)n, 0u);
      if (!same(plan_run(fl.data(), none.data(), nullptr, 0, first, n, f), base) ||
          !same(plan_run(fl.data(), nullptr, nullptr, 0, first, n, f), base)) {
        std::printf("FAIL zero fix flags, variant %d iteration %d\n", (int)(&f - variants), it);
        g_fail++;
      }
      const double df = dens[1 + rng() % 4];
      std::vector<uint32_t> fx((size_t)n, 0u);
      for (uint32_t& w : fx)
        if (u01(rng) < df) w = 1u + (uint32_t)(rng() % 7);
      const EpochPlan p = plan_run(fl.data(), fx.data(), nullptr, 0, first, n, f);
      // structure: the epoch launches tile the range once in order; a FIX entry
      // per flagged epoch, right after the launch that ends with it (or its EFFORTS)
      int64_t next = first;
      bool ok = true;
      size_t nfix = 0;
      for (size_t i = 0; i < p.launches.size() && ok; i++) {
        const Launch& l = p.launches[i];
        if (l.kind == FIX) {
          nfix++;
          ok = i > 0 && p.launches[i - 1].kind != FIX && l.first == next - 1 && l.count == 1 &&
               l.ev_any == fx[(size_t)(l.first - first)] && l.ev_any != 0 &&
               ((fl[(size_t)(l.first - first)] & E) != 0) == (p.launches[i - 1].kind == EFFORTS);
        } else if (l.kind == EFFORTS) {
          ok = l.first == next - 1;
        } else {
          ok = l.first == next && l.count > 0;
          for (int64_t k = l.first; k + 1 < l.first + l.count; k++) ok = ok && !fx[(size_t)(k - first)];
          next = l.first + l.count;
          pairs += l.kind == EPOCH_PAIR;
        }
      }
      size_t want = 0;
      for (uint32_t w : fx) want += w != 0;
      fixes += (int)nfix;
      ok = ok && next == first + n && nfix == want;
      if (!ok || !same(p, naive_plan(fl, fx, first, f))) {
        std::printf("FAIL fix plan property, variant %d iteration %d:\n  got   %s\n  naive %s\n", (int)(&f - variants), it,
                    show(p).c_str(), show(naive_plan(fl, fx, first, f)).c_str());
        g_fail++;
      }
    }
  CHECK(plans >= 2000 && fixes > 2000 && pairs > 200);
}

// fixes_valid on a 10-epoch log with 3 rows per kind: the example is accepted,
// each defect alone is rejected, and only inside [first, first + count)
static void test_fixes_valid() {
  const auto fl = flags(10, 0, {{2, XY}, {5, XY | Z | GEO}, {9, GEO}});
  const std::vector<int32_t> xi = {-1, -1, 0, -1, -1, 2, -1, -1, -1, -1}, zi = {-1, -1, -1, -1, -1, 1, -1, -1, -1, -1},
                             gi = {-1, -1, -1, -1, -1, 0, -1, -1, -1, 2};
  const double rows[1] = {0.0};  // stands for the device arrays: tested for null, never read
  uwvk_pose_fixes ok{};
  ok.host_flags = fl.data();
  ok.xy_index = xi.data(), ok.xy = rows, ok.n_xy = 3;
  ok.z_index = zi.data(), ok.z = rows, ok.n_z = 3;
  ok.geo_index = gi.data(), ok.geo = rows, ok.n_geo = 3;
  CHECK(fixes_valid(&ok, 0, 10) && fixes_valid(&ok, 3, 4) && fixes_valid(&ok, 10, 0));
  // the epoch whose entry is changed, the changed struct
  auto bad = [&](int64_t e, const uwvk_pose_fixes& f) {
    // rejected over every range that holds the epoch, accepted beside it
    return !fixes_valid(&f, 0, 10) && !fixes_valid(&f, e, 1) && fixes_valid(&f, 0, e) && fixes_valid(&f, e + 1, 9 - e);
  };
  auto with = [](std::vector<int32_t> v, int64_t e, int32_t x) {
    v[(size_t)e] = x;
    return v;
  };
  uwvk_pose_fixes f = ok;
  const auto neg = with(xi, 2, -1), past = with(gi, 9, 3), far = with(zi, 5, 1 << 20);
  f.xy_index = neg.data();  // a negative index at a flagged epoch
  CHECK(bad(2, f));
  f = ok, f.geo_index = past.data();  // an index >= n
  CHECK(bad(9, f));
  f = ok, f.z_index = far.data();
  CHECK(bad(5, f));
  f = ok, f.n_xy = 2;  // row 2 is gone
  CHECK(bad(5, f));
  f = ok, f.z_index = nullptr;  // a flagged kind without its index array
  CHECK(bad(5, f));
  f = ok, f.z = nullptr;  // ... without its rows
  CHECK(bad(5, f));
  f = ok, f.xy = nullptr;  // (flagged at epochs 2 and 5)
  CHECK(!fixes_valid(&f, 0, 10) && !fixes_valid(&f, 2, 1) && !fixes_valid(&f, 5, 1) && fixes_valid(&f, 6, 4));
  const auto outside = flags(10, 0, {{2, XY}, {5, XY | Z | GEO}, {7, 0x8u}, {9, GEO}});
  f = ok, f.host_flags = outside.data();  // a flag bit outside UWVK_FIX_*
  CHECK(bad(7, f));
  f = ok, f.host_flags = nullptr;
  CHECK(!fixes_valid(&f, 0, 10) && !fixes_valid(&f, 0, 0));
  // an unflagged kind needs no arrays, an unflagged epoch no valid index
  const auto only_z = flags(10, 0, {{5, Z}});
  f = ok, f.host_flags = only_z.data(), f.xy_index = nullptr, f.xy = nullptr, f.geo = nullptr, f.n_geo = 0;
  CHECK(fixes_valid(&f, 0, 10));
}

int main() {
  test_cases();
  test_track();
  test_properties();
  test_fixes_valid();
  if (g_fail) std::printf("%d checks failed\n", g_fail);
  else std::printf("fix_plan_test: ok\n");
  return g_fail ? 1 : 0;
}
