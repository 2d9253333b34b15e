// plan_test.cpp — the host planner of uwvk_pose_run_log (csrc/uwvk_plan.hpp) on
// the CPU: the kernel choice and the split of a log into launches (fixed cases
// and a property check against a naive restatement of the rule), the grid /
// tail geometry, the process-noise tables and the parameter-block scan.
// Exit 0 = all checks hold.
#include <random>

#include "plan_check.hpp"
#include "../../slam-uwv_kalman_filters_amd/csrc/uwvk_host.hpp"

// an all-IMU log of n epochs, ev's bits ORed in
static std::vector<uint32_t> flags(int64_t n, Ev ev = {}) { return flags(n, IMU, ev); }

static void expect(const std::vector<uint32_t>& f, const EpochFacts& facts, const char* want, int line) {
  expect_plan(plan_epochs(f.data(), 0, (int64_t)f.size(), facts), want, line);
  // a call without events is plan_epochs' plan
  expect_plan(plan_run(f.data(), nullptr, nullptr, 0, 0, (int64_t)f.size(), facts), want, line);
}
#define EXPECT(f, facts, want) expect(f, facts, want, __LINE__)

static void test_plan_cases() {
  const EpochFacts d = defaults();
  EXPECT(flags(200), d, "PAIR[0,200)pd pdec=1");
  EXPECT(flags(200, {{100, P}}), d, "PAIR[0,100)pd ONE[100,101)pd PAIR[101,200)pd pdec=1");
  EXPECT(flags(100, {{47, P}}), d, "ONE[0,48)pd PAIR[48,100)pd pdec=1");
  EXPECT(flags(100, {{48, P}}), d, "PAIR[0,48)pd ONE[48,49)pd PAIR[49,100)pd pdec=1");
  EXPECT(flags(60, {{10, P}, {30, P}}), d, "ONE[0,60)pd pdec=1");  // no run reaches 48 epochs
  EXPECT(flags(120, {{59, E}}), d, "PAIR[0,60)pd EFFORTS(59,vo=0) ONE[60,120) pdec=0");
  EXPECT(flags(120, {{59, E | VO}}), d, "PAIR[0,60)pd EFFORTS(59,vo=1) PAIR[60,120)pd pdec=1");
  EXPECT(flags(120, {{119, E}}), d, "PAIR[0,120)pd EFFORTS(119,vo=0) pdec=0");
  EXPECT(flags(0), d, "pdec=1");
  // no pair kernel: the efforts split alone, still parameter-decoupled
  const auto mixed = flags(120, {{20, P}, {59, E | VO}, {90, A}});
  const char* one_pd = "ONE[0,60)pd EFFORTS(59,vo=1) ONE[60,120)pd pdec=1";
  EpochFacts f = d;
  EXPECT(mixed, d, "ONE[0,60)pd EFFORTS(59,vo=1) PAIR[60,120)pd pdec=1");
  f = d, f.batch = 63;
  EXPECT(mixed, f, one_pd);
  f = d, f.pair_opt = 0;
  EXPECT(mixed, f, one_pd);
  f = d, f.persist = 0;
  EXPECT(mixed, f, one_pd);
  f = d, f.lds_pad = 1024;
  EXPECT(mixed, f, one_pd);
  // not parameter-decoupled: the general kernel, never a pair
  const char* one = "ONE[0,60) EFFORTS(59,vo=1) ONE[60,120) pdec=";
  f = d, f.pd_opt = 0;
  EXPECT(mixed, f, (std::string(one) + "1").c_str());
  f = d, f.pdec = false;
  EXPECT(mixed, f, (std::string(one) + "0").c_str());
  f = d, f.q_params_diag = false;
  EXPECT(mixed, f, (std::string(one) + "1").c_str());
  f = d, f.q_simple = false;
  EXPECT(mixed, f, (std::string(one) + "1").c_str());
  // dof 26: a pair whenever Q is simple, whatever pdec is, never pd
  for (bool pdec : {false, true}) {
    f = d, f.dof = 26, f.pdec = pdec, f.q_params_diag = false;
    EXPECT(flags(120, {{59, E}}), f, "PAIR[0,60) EFFORTS(59,vo=0) PAIR[60,120) pdec=0");
    f.q_simple = false;
    EXPECT(flags(120, {{59, E | VO}}), f, (std::string(one) + (pdec ? "1" : "0")).c_str());
  }
  // first > 0: absolute epochs, flags read at k - first
  {
    const auto fl = flags(100, {{48, P}});
    const EpochPlan p = plan_epochs(fl.data(), 1000, 100, d);
    const std::string got = show(p);
    CHECK(got == "PAIR[1000,1048)pd ONE[1048,1049)pd PAIR[1049,1100)pd pdec=1");
    CHECK(p.launches.size() == 3 && p.launches[1].ev_any == (IMU | P) && p.launches[0].ev_any == IMU);
  }
  // the predicates' remaining inputs
  f = d, f.dense = true;
  CHECK(!runs_pair(f) && runs_pd(f));
  f = d, f.dof = 26;
  CHECK(runs_pair(f) && !runs_pd(f));
}

// The rule once more, per epoch: label every epoch with the kernel it runs on,
// then merge equal neighbours.  A range ends with its BodyEfforts epoch; inside
// a pair-eligible range an epoch runs on the pair kernel when it has no
// pressure update and the stretch of such epochs around it is kPairMinRun long
// or the whole range.
static EpochPlan naive_plan(const std::vector<uint32_t>& fl, int64_t first, EpochFacts f) {
  EpochPlan p;
  const int64_t n = (int64_t)fl.size();
  std::vector<int> range_of((size_t)n);  // index of the efforts-bounded range
  for (int64_t k = 0, r = 0; k < n; k++) {
    range_of[(size_t)k] = (int)r;
    if (fl[(size_t)k] & E) r++;
  }
  std::vector<LaunchKind> label((size_t)n, EPOCH_ONE);
  std::vector<int> pd((size_t)n, 0);
  for (int64_t k = 0; k < n; k++) {
    pd[(size_t)k] = runs_pd(f);
    if (runs_pair(f) && !(fl[(size_t)k] & P)) {
      int64_t lo = k, hi = k;  // the stretch [lo, hi] without pressure in k's range
      while (lo > 0 && range_of[(size_t)lo - 1] == range_of[(size_t)k] && !(fl[(size_t)lo - 1] & P)) lo--;
      while (hi + 1 < n && range_of[(size_t)hi + 1] == range_of[(size_t)k] && !(fl[(size_t)hi + 1] & P)) hi++;
      const bool whole = (lo == 0 || range_of[(size_t)lo - 1] != range_of[(size_t)k]) &&
                         (hi + 1 == n || range_of[(size_t)hi + 1] != range_of[(size_t)k]);
      if (hi - lo + 1 >= 48 || whole) label[(size_t)k] = EPOCH_PAIR;
    }
    if ((fl[(size_t)k] & E) && !(fl[(size_t)k] & VO)) f.pdec = false;
  }
  for (int64_t k = 0; k < n; k++) {
    const bool merge = k > 0 && range_of[(size_t)k - 1] == range_of[(size_t)k] && label[(size_t)k - 1] == label[(size_t)k];
    if (merge) {
      Launch& l = p.launches.back();
      l.count++;
      l.ev_any |= fl[(size_t)k];
    } else {
      p.launches.push_back({label[(size_t)k], first + k, 1, pd[(size_t)k], 0, fl[(size_t)k]});
    }
    if (fl[(size_t)k] & E) p.launches.push_back({EFFORTS, first + k, 1, 0, (fl[(size_t)k] & VO) ? 1 : 0, fl[(size_t)k]});
  }
  p.pdec = f.pdec;
  return p;
}

static void test_plan_properties() {
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
  int plans = 0, pairs = 0;
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
      const EpochPlan p = plan_epochs(fl.data(), first, n, f);
      auto fk = [&](int64_t k) { return fl[(size_t)(k - first)]; };
      int64_t next = first, range0 = first;  // the next epoch to cover; the start of the efforts-bounded range
      bool ok = true;
      for (size_t i = 0; i < p.launches.size() && ok; i++) {
        const Launch& l = p.launches[i];
        if (l.kind == EFFORTS) {
          // right after the epoch launch that ends with this efforts epoch
          ok = i > 0 && p.launches[i - 1].kind != EFFORTS && l.first == next - 1 && l.count == 1 && (fk(l.first) & E) &&
               l.vo == ((fk(l.first) & VO) ? 1 : 0);
          range0 = next;
          continue;
        }
        ok = l.first == next && l.count > 0 && l.first + l.count <= first + n;  // tiles the range once, in order
        if (!ok) break;
        uint32_t ev = 0;
        for (int64_t k = l.first; k < l.first + l.count; k++) {
          ev |= fk(k);
          // an efforts epoch only as the last epoch of a launch, followed by its EFFORTS entry
          if (fk(k) & E)
            ok = ok && k == l.first + l.count - 1 && i + 1 < p.launches.size() && p.launches[i + 1].kind == EFFORTS;
        }
        ok = ok && ev == l.ev_any;
        next = l.first + l.count;
        if (l.kind == EPOCH_PAIR) {
          pairs++;
          const bool whole = l.first == range0 && (next == first + n || (fk(next - 1) & E));
          ok = ok && !(ev & P) && (l.count >= 48 || whole);
        }
      }
      ok = ok && next == first + n;
      if (!ok || !same(p, naive_plan(fl, first, f)) || !same(p, plan_run(fl.data(), nullptr, nullptr, 0, first, n, f))) {
        std::printf("FAIL plan property, variant %d iteration %d:\n  got  %s\n  naive %s\n", (int)(&f - variants), it,
                    show(p).c_str(), show(naive_plan(fl, first, f)).c_str());
        g_fail++;
      }
    }
  CHECK(plans >= 2000 && pairs > 200);
}

static void test_geometry() {
  Geometry g = persist_geometry(65536, 3072, 0, 0, 0, 200, 0, -1);
  CHECK(g.chunks == 4 && g.tail0 == 53248 && g.r_x == 12288 && g.units == 102400 && g.grid == 3072 &&
        g.wait_bound == 1074176 && g.tail_need == 12288 && g.tail_cap == 8 * 3072 && g.n_x == 0);
  // the pair kernel does not spread unless asked
  g = persist_geometry(32768, 3072, 0, 0, 0, 200, 1, -1);
  CHECK(g.chunks == 1 && g.tail0 == 32768 && g.r_x == 0 && g.units == 32768 && g.grid == 3072 && g.tail_need == 0);
  g = persist_geometry(1000, 3072, 0, 0, 0, 200, 1, -1);
  CHECK(g.chunks == 1 && g.units == 1000 && g.grid == 1000);
  g = persist_geometry(32768, 3072, 384, 0, 0, 200, 1, -1);  // UWVK_OPT_TAIL_SLOTS > 0
  CHECK(g.chunks == 4 && g.r_x == 4 * 3072);
  g = persist_geometry(32768, 3072, 0, 2, 0, 200, 1, 5);  // UWVK_OPT_TAIL_CHUNKS, UWVK_OPT_WAIT_BOUND
  CHECK(g.chunks == 2 && g.tail0 == 32768 - 2 * 3072 && g.units == 32768 + 2 * 3072 && g.wait_bound == 5);
  CHECK(persist_geometry(65536, 3072, -1, 0, 0, 200, 0, -1).chunks == 1);
  CHECK(persist_geometry(65536, 3072, 0, 0, 4096, 200, 0, -1).chunks == 1);
  CHECK(persist_geometry(65536, 3072, -1, 3, 0, 200, 0, -1).chunks == 1);
  CHECK(persist_geometry(65536, 3072, 0, 3, 0, 200, 0, -1).chunks == 3);
  CHECK(persist_geometry(9000, 3072, 0, 3, 0, 200, 0, -1).chunks == 1);   // 3 x 3072 instances are not there
  CHECK(persist_geometry(65536, 3072, 0, 3, 0, 2, 0, -1).chunks == 1);    // fewer epochs than chunks
  CHECK(persist_geometry(65536, 3072, 0, 8, 0, 200, 0, -1).chunks == 8);
  g = persist_geometry(40, 3072, 3, 3, 0, 20, 0, -1);  // slots per XCD given: 8 x 3 units per chunk
  CHECK(g.chunks == 1);
  g = persist_geometry(80, 3072, 3, 3, 0, 20, 0, -1);
  CHECK(g.chunks == 3 && g.r_x == 72 && g.tail0 == 8 && g.units == 8 + 3 * 72 && g.grid == g.units);

  g = static_geometry(65536, 384, 0, 0, 0, 200, -1);
  CHECK(g.chunks == 4 && g.n_x == 8192 && g.tail0 == 6656 && g.r_x == 1536 && g.grid == 102400 &&
        g.wait_bound == 1061376 && g.tail_need == 12288 && g.tail_cap == 24576);
  for (const Geometry& u : {static_geometry(65532, 384, 0, 0, 0, 200, -1), static_geometry(65536, 384, -1, 0, 0, 200, -1),
                            static_geometry(65536, 384, 0, 0, 64, 200, -1), static_geometry(65536, 0, 0, 0, 0, 200, -1),
                            static_geometry(65536, 384, 0, 0, 0, 3, -1)})
    CHECK(u.chunks == 1 && u.grid == 0 && u.tail_need == 0);
  g = static_geometry(96, 384, 3, 3, 0, 20, 7);  // 12 per XCD over 3 slots, 3 chunks forced
  CHECK(g.chunks == 3 && g.n_x == 12 && g.r_x == 9 && g.tail0 == 3 && g.grid == 8 * (12 + 2 * 9) && g.wait_bound == 7 &&
        g.tail_need == 72 && g.tail_cap == 8 * 24);
  CHECK(static_geometry(96, 384, 3, 5, 0, 20, -1).chunks == 1);  // 5 x 3 > 12
  CHECK(plan_tail(8192, 384, 20) == 2 && plan_tail(8192, 384, 200) == 4 && plan_tail(700, 384, 200) == 1);
}

static uwvk_pose_config example_config() {
  uwvk_pose_config c{};
  for (int i = 0; i < 3; i++) {
    c.acceleration.randomwalk[i] = 1e-3, c.acceleration.bias_instability[i] = 1e-4;
    c.rotation_rate.randomwalk[i] = 1e-4, c.rotation_rate.bias_instability[i] = 1e-5;
    c.max_jerk[i] = 0.5;
  }
  c.acceleration.bias_tau = c.rotation_rate.bias_tau = 600;
  uwvk_model_noise& m = c.model_noise_parameters;
  for (int i = 0; i < 9; i++)
    m.inertia_instability[i] = 10, m.lin_damping_instability[i] = 5, m.quad_damping_instability[i] = 5;
  m.inertia_tau = m.lin_damping_tau = m.quad_damping_tau = 3600;
  c.water_velocity.tau = 900, c.water_velocity.limits = 0.1;
  c.water_velocity.adcp_bias_tau = 900, c.water_velocity.adcp_bias_limits = 0.05;
  c.hydrostatics.water_density = 1025, c.hydrostatics.water_density_limits = 2, c.hydrostatics.water_density_tau = 3600;
  return c;
}

static void test_q_tables() {
  const uwvk_pose_config cfg = example_config();
  const double dt = 0.01, q_imu[4] = {0.8, 0.2, -0.4, 0.4};  // a rotated IMU: full 3 x 3 blocks
  const double ntau[8] = {-1. / 600, -1. / 600, -1. / 3600, -1. / 3600, -1. / 3600, -1. / 900, -1. / 900, -1. / 3600};
  for (int n : {53, 26}) {
    std::vector<double> Q((size_t)n * n);
    host::pose_process_noise(n, cfg, dt, q_imu, Q.data());
    const QTables t = build_q_tables(n, Q, ntau, dt);
    CHECK(t.q_simple == 1 && t.q_bw == 2 && t.q_band == 1 && q_is_simple(n, Q));
    CHECK(q_params_diag(n, Q) == (n == 53));
    CHECK((int)t.qp.size() == n * (n + 1) && (int)t.band.size() == kQBand && (int)t.qpd.size() == 2 * kQpdEntries);
    // A_ii of a Markov block 1 + dt (-1 / tau), of any other DOF 1
    auto a = [&](int d) {
      if (d >= 12 && d < 18) return 1.0 + dt * ntau[d < 15 ? 0 : 1];
      if (n == 53 && d >= 19 && d < 46) return 1.0 + dt * ntau[2 + (d - 19) / 9];
      const int w = n == 53 ? 46 : 19;  // water velocity (4), ADCP bias (2), density (1)
      if (d >= w) return 1.0 + dt * ntau[d < w + 4 ? 5 : d < w + 6 ? 6 : 7];
      return 1.0;
    };
    int stored = 0;
    for (int i = 0, k = 0; i < n; i++) {
      CHECK(t.qlo[i] >= (i >= 9 ? 9 : i + 1) && t.qlo[i] <= i + 1 && t.qoff[i] == stored);
      for (int j = 0; j <= i; j++, k++) {
        CHECK(t.qp[2 * k] == ((i < 9 || j < 9) ? 0.0 : a(i) * a(j)));
        CHECK(t.qp[2 * k + 1] == dt * dt * Q[(size_t)i * n + j]);
        if (j >= t.qlo[i]) {
          CHECK(t.band[t.qoff[i] + j - t.qlo[i]] == dt * dt * Q[(size_t)i * n + j]);
          stored++;
        } else if (i >= 9 && j >= 9) {
          CHECK(Q[(size_t)i * n + j] == 0.0);  // left of the band
        }
      }
    }
    CHECK(stored > n - 9 && stored <= kQBand);
    if (n == 53) {
      for (int i = 0, k = 0; i < 26; i++)
        for (int j = 0; j <= i; j++, k++) {
          const int I = pd_dof(i), J = pd_dof(j), k53 = I * (I + 1) / 2 + J;
          CHECK(t.qpd[2 * k] == t.qp[2 * k53] && t.qpd[2 * k + 1] == t.qp[2 * k53 + 1]);
        }
      for (int p = 0; p < 27; p++) {
        const int d = 19 + p, k53 = d * (d + 1) / 2 + d;
        CHECK(t.qpd[2 * (351 + p)] == t.qp[2 * k53] && t.qpd[2 * (351 + p) + 1] == dt * dt * Q[(size_t)d * 53 + d]);
        CHECK(t.qpd[2 * (351 + p) + 1] > 0.0);
      }
      CHECK(pd_dof(18) == 18 && pd_dof(19) == 46 && pd_dof(25) == 52);
    } else {
      for (double v : t.qpd) CHECK(v == 0.0);
    }
  }
  std::vector<double> Q(53 * 53, 0.0);
  Q[20 * 53 + 3] = 1e-6;  // a parameter row coupled with the orientation
  CHECK(!q_is_simple(53, Q) && !q_params_diag(53, Q) && build_q_tables(53, Q, ntau, dt).q_simple == 0);
  Q.assign(53 * 53, 0.0);
  Q[50 * 53 + 46] = 1e-6;  // a band of 4 below the diagonal
  QTables t = build_q_tables(53, Q, ntau, dt);
  CHECK(!q_is_simple(53, Q) && q_params_diag(53, Q) && t.q_simple == 0 && t.q_bw == 4 && t.qlo[50] == 46);
  Q.assign(53 * 53, 0.0);
  Q[30 * 53 + 29] = 1e-6;  // inside the band, but a parameter off its diagonal
  CHECK(q_is_simple(53, Q) && !q_params_diag(53, Q));
  t = build_q_tables(53, {}, ntau, dt);  // no process noise set
  CHECK(t.q_simple == 1 && t.q_bw == 0 && t.q_band == 1 && q_is_simple(53, {}) && q_params_diag(53, {}));
  for (double v : t.band) CHECK(v == 0.0);
  for (size_t k = 0; k < t.qp.size() / 2; k++) CHECK(t.qp[2 * k + 1] == 0.0);
  for (int i = 0; i < 53; i++) CHECK(t.qlo[i] == i + 1 && t.qoff[i] == 0);
  // a dense Q: the band does not fit its 128 entries
  Q.assign(53 * 53, 1e-6);
  t = build_q_tables(53, Q, ntau, dt);
  CHECK(t.q_band == 0 && t.q_simple == 0 && t.q_bw == 43);
}

static void test_param_block() {
  const int tn = 53 * 54 / 2;
  auto at = [&](int i, int j) { return i * (i + 1) / 2 + j; };
  // the constructor's shape: 3 x 3 blocks in position .. biases, a diagonal below
  std::vector<double> Pp((size_t)3 * tn, 0.0);
  for (int b = 0; b < 3; b++) {
    for (int i = 0; i < 53; i++) Pp[(size_t)b * tn + at(i, i)] = 1.0 + i;
    for (int blk : {0, 3, 12, 15}) Pp[(size_t)b * tn + at(blk + 1, blk)] = Pp[(size_t)b * tn + at(blk + 2, blk)] = 0.01;
  }
  CHECK(param_block_decoupled(53, 3, Pp.data()));
  std::vector<double> c = Pp;
  c[(size_t)1 * tn + at(30, 2)] = 1e-9;
  CHECK(!param_block_decoupled(53, 3, c.data()) && param_block_decoupled(53, 1, c.data()));
  c = Pp;
  c[(size_t)2 * tn + at(48, 47)] = 1e-3;  // water velocity: not a parameter row or column
  CHECK(param_block_decoupled(53, 3, c.data()));
  c = Pp;
  c[at(47, 45)] = 1e-9;  // a parameter column under the block
  CHECK(!param_block_decoupled(53, 3, c.data()));
  c = Pp;
  c[at(45, 44)] = 1e-9;  // inside the block
  CHECK(!param_block_decoupled(53, 3, c.data()));
  CHECK(!param_block_decoupled(26, 3, Pp.data()));
}

int main() {
  test_plan_cases();
  test_plan_properties();
  test_geometry();
  test_q_tables();
  test_param_block();
  if (g_fail) std::printf("%d checks failed\n", g_fail);
  else std::printf("plan_test: ok\n");
  return g_fail ? 1 : 0;
}
