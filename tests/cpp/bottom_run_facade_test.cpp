// bottom_run_facade_test.cpp — BottomUKF::runLog through the C++ facade: a
// 20-epoch log at batch 11 (4 beams, one range per epoch, a normal every fifth)
// must be bitwise the facade's own setVelocity / predictionStep /
// integrateMeasurement sequence on a second filter.  Exit 0 = equal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "uwv_kalman_filters_amd/BottomUKF.hpp"

namespace U = uwv_kalman_filters_amd;

// a device copy of a host array (at least one element)
template <class T>
static T* upload(const std::vector<T>& v) {
  void* d = nullptr;
  const size_t bytes = (v.empty() ? 1 : v.size()) * sizeof(T);
  U::check(uwvk_device_malloc(0, bytes, &d), "uwvk_device_malloc");
  if (!v.empty()) U::check(uwvk_memcpy_h2d(d, v.data(), bytes), "uwvk_memcpy_h2d");
  return (T*)d;
}

int main() {
  const int64_t B = 11, E = 20;
  const int beams = 4;
  const double dt = 0.2;
  std::mt19937_64 rng(7);
  std::normal_distribution<double> n01;
  std::vector<double> x0(B * 4), P0(B * 9, 0.0);
  for (int64_t i = 0; i < B; i++) {
    x0[i * 4] = 10.0 + 0.5 * n01(rng);
    x0[i * 4 + 1] = 0.05 * n01(rng);
    x0[i * 4 + 2] = 0.05 * n01(rng);
    x0[i * 4 + 3] = 1.0;
    P0[i * 9] = 0.2;
    P0[i * 9 + 4] = P0[i * 9 + 8] = 0.01;
  }
  const std::array<double, 9> Q = {0.02, 0, 0, 0, 0.001, 0, 0, 0, 0.001};
  const std::array<double, 4> ncov = {4e-4, 0, 0, 4e-4};
  const double s = std::sqrt(0.25 + 0.866 * 0.866);
  const double dirs[4][3] = {{0.5 / s, 0, -0.866 / s}, {-0.5 / s, 0, -0.866 / s}, {0, 0.5 / s, -0.866 / s},
                             {0, -0.5 / s, -0.866 / s}};
  const double orgs[4][3] = {{0.1, 0, 0}, {-0.1, 0, 0}, {0, 0.1, 0}, {0, -0.1, 0}};

  std::vector<uint32_t> flags(E);
  std::vector<int32_t> ri(E), ni(E, 0);
  std::vector<double> vel(E * B * 3), range(E * beams * B, 0.0), var(E * beams * B, 1.0), normal;
  for (int64_t e = 0; e < E; e++) {
    const int b = (int)(e % beams);
    flags[e] = UWVK_BEV_BEAM(b);
    ri[e] = (int32_t)e;
    for (int64_t i = 0; i < B; i++) {
      vel[(e * B + i) * 3] = 0.5 + 0.1 * n01(rng);
      vel[(e * B + i) * 3 + 1] = 0.1 * n01(rng);
      vel[(e * B + i) * 3 + 2] = 0.05 * n01(rng);
      range[(e * beams + b) * B + i] = 10.0 / 0.866 + 0.05 * n01(rng);
      var[(e * beams + b) * B + i] = 0.02 + 0.001 * (double)i;
    }
    if (e % 5 == 4) {
      flags[e] |= UWVK_BEV_NORMAL;
      ni[e] = (int32_t)(normal.size() / (B * 3));
      for (int64_t i = 0; i < B; i++) {
        normal.push_back(0.03 * n01(rng));
        normal.push_back(0.03 * n01(rng));
        normal.push_back(1.0);
      }
    }
  }
  uwvk_bottom_log log{};
  log.epochs = E;
  log.dt = dt;
  log.flags = flags.data();
  log.velocity = upload(vel);
  log.beams = beams;
  std::memcpy(log.beam_direction, dirs, sizeof(dirs));
  std::memcpy(log.beam_origin, orgs, sizeof(orgs));
  log.range_index = ri.data();
  log.range = upload(range);
  log.range_var = upload(var);
  log.n_range = E;
  log.range_cov = 0.02;
  log.normal_index = ni.data();
  log.normal = upload(normal);
  log.n_normal = (int64_t)(normal.size() / (B * 3));
  std::memcpy(log.normal_cov, ncov.data(), sizeof(log.normal_cov));

  U::BottomUKF run(B, x0, P0), step(B, x0, P0);
  run.setProcessNoiseCovariance(Q);
  step.setProcessNoiseCovariance(Q);
  run.runLog(log, 0, 8);
  run.runLog(log, 8, E - 8);
  run.synchronize();
  for (int64_t e = 0; e < E; e++) {
    step.setVelocity(std::vector<double>(vel.begin() + e * B * 3, vel.begin() + (e + 1) * B * 3));
    step.predictionStep(dt);
    const int b = (int)(e % beams);
    U::RangeMeasurement r;
    r.mu.assign(range.begin() + (e * beams + b) * B, range.begin() + (e * beams + b + 1) * B);
    r.cov.assign(var.begin() + (e * beams + b) * B, var.begin() + (e * beams + b + 1) * B);
    step.integrateMeasurement(r, {dirs[b][0], dirs[b][1], dirs[b][2]}, {orgs[b][0], orgs[b][1], orgs[b][2]});
    if (flags[e] & UWVK_BEV_NORMAL) {
      U::NormalMeasurement nm;
      nm.mu.assign(normal.begin() + ni[e] * B * 3, normal.begin() + (ni[e] + 1) * B * 3);
      step.integrateMeasurement(nm, ncov);
    }
  }
  std::vector<double> xa, Pa, xb, Pb;
  run.getState(xa, &Pa);
  step.getState(xb, &Pb);
  const bool same_x = std::memcmp(xa.data(), xb.data(), xa.size() * 8) == 0;
  const bool same_P = std::memcmp(Pa.data(), Pb.data(), Pa.size() * 8) == 0;
  const bool moved = std::memcmp(xa.data(), x0.data(), 8) != 0;
  // an invalid range throws (UWVK_EINVAL) and leaves the state alone
  bool threw = false;
  try {
    run.runLog(log, 0, E + 1);
  } catch (const U::Error& e) {
    threw = e.code == UWVK_EINVAL;
  }
  std::vector<double> x2;
  run.getState(x2);
  std::printf("bottom run facade: mean %d, covariance %d, moved %d, einval %d, untouched %d\n", (int)same_x,
              (int)same_P, (int)moved, (int)threw, (int)(x2 == xa));
  for (const void* p : {(const void*)log.velocity, (const void*)log.range, (const void*)log.range_var,
                        (const void*)log.normal})
    uwvk_device_free(const_cast<void*>(p));
  return (same_x && same_P && moved && threw && x2 == xa) ? 0 : 1;
}
