// fix_facade_test.cpp — PoseUKF::runLogFixes through the C++ facade: 60 IMU
// epochs at batch 4 with an XY fix after epoch 19, a Z fix after 39 and both
// after 59, against a second filter that runs runLog cut there with
// uwvk_pose_update_xy / _z at the cuts.  The states must be bitwise equal, the
// fix accept counts complete, and a row index out of range must throw
// (UWVK_EINVAL) and leave the state alone.  Exit 0 = all of that.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "uwv_kalman_filters_amd/PoseUKF.hpp"

namespace U = uwv_kalman_filters_amd;

static void fill(double* d, std::initializer_list<double> v) {
  int i = 0;
  for (double x : v) d[i++] = x;
}

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
  const int64_t B = 4, E = 60;
  const double dt = 1e-3;
  uwvk_pose_config cfg{};
  fill(cfg.acceleration.randomwalk, {1e-3, 1e-3, 1e-3});
  fill(cfg.acceleration.bias_instability, {1e-4, 1e-4, 1e-4});
  cfg.acceleration.bias_tau = 600;
  fill(cfg.rotation_rate.randomwalk, {1e-4, 1e-4, 1e-4});
  fill(cfg.rotation_rate.bias_instability, {1e-5, 1e-5, 1e-5});
  cfg.rotation_rate.bias_tau = 600;
  auto& m = cfg.model_noise_parameters;
  fill(m.body_efforts_std, {5, 5, 5, 1, 1, 1});
  for (int i = 0; i < 9; i++) m.inertia_instability[i] = 10, m.lin_damping_instability[i] = 5,
                              m.quad_damping_instability[i] = 5;
  m.inertia_tau = m.lin_damping_tau = m.quad_damping_tau = 3600;
  cfg.water_velocity.tau = 900; cfg.water_velocity.limits = 0.1; cfg.water_velocity.scale = 1e-3;
  fill(cfg.water_velocity.measurement_std, {0.05, 0.05, 0.05});
  cfg.water_velocity.adcp_bias_tau = 900; cfg.water_velocity.adcp_bias_limits = 0.05;
  cfg.location = {0.9, 0.15, 0.0};
  cfg.hydrostatics = {1025, 2, 3600, 101325, 100};
  uwvk_uwv_params uwv{};
  const double Md[6] = {200, 250, 300, 20, 30, 30}, Dl[6] = {20, 30, 40, 5, 5, 5}, Dq[6] = {50, 80, 100, 10, 10, 10};
  for (int i = 0; i < 6; i++) {
    uwv.inertia_matrix[i * 7] = Md[i];
    uwv.damping_matrices[0][i * 7] = Dl[i];
    uwv.damping_matrices[1][i * 7] = Dq[i];
  }
  uwv.weight = uwv.buoyancy = 2000;
  uwv.distance_body2centerofbuoyancy[2] = 0.05;

  std::mt19937_64 rng(11);
  std::normal_distribution<double> n01;
  std::vector<double> pos(B * 3), pos_cov(B * 9, 0), rot(B * 4, 0), rot_cov(B * 9, 0);
  for (int64_t b = 0; b < B; b++) {
    rot[b * 4] = 1.0;
    for (int i = 0; i < 3; i++) {
      pos[b * 3 + i] = 5 * n01(rng);
      pos_cov[b * 9 + i * 4] = 0.1;
      rot_cov[b * 9 + i * 4] = 1e-3;
    }
  }
  U::PoseUKF fa(B, pos, pos_cov, rot, rot_cov, cfg, uwv), fb(B, pos, pos_cov, rot, rot_cov, cfg, uwv);
  fa.setProcessNoiseFromConfig(cfg, dt);
  fb.setProcessNoiseFromConfig(cfg, dt);

  // an IMU-only log: no DVL / pressure / ADCP / efforts sample
  std::vector<uint32_t> flags(E, UWVK_EV_ACC);
  std::vector<int32_t> none(E, -1);
  std::vector<double> gyro(E * B * 3), acc(E * B * 3), empty;
  for (size_t k = 0; k < gyro.size(); k++) {
    gyro[k] = 0.01 * n01(rng);
    acc[k] = (k % 3 == 2 ? 9.81 : 0.0) + 0.02 * n01(rng);
  }
  uwvk_pose_log log{};
  log.epochs = E;
  log.dt = dt;
  log.flags = upload(flags);
  log.host_flags = flags.data();
  log.gyro = upload(gyro);
  log.acc = upload(acc);
  log.dvl_index = log.pressure_index = log.adcp_index = log.efforts_index = upload(none);
  log.dvl = log.pressure = log.adcp = log.efforts = upload(empty);
  log.adcp_cells = 1;
  for (int i = 0; i < 3; i++) log.acc_cov[i * 4] = 1e-4, log.dvl_cov[i * 4] = 1e-4;
  log.pressure_cov = 1e4;
  log.adcp_cov[0] = log.adcp_cov[3] = 2.5e-3;
  for (int i = 0; i < 6; i++) log.efforts_cov[i * 7] = 25;

  // XY after epochs 19 and 59 (rows 0, 1), Z after 39 and 59 (rows 0, 1)
  std::vector<uint32_t> fix_flags(E, 0u);
  std::vector<int32_t> xy_index(E, -1), z_index(E, -1);
  fix_flags[19] = UWVK_FIX_XY, fix_flags[39] = UWVK_FIX_Z, fix_flags[59] = UWVK_FIX_XY | UWVK_FIX_Z;
  xy_index[19] = 0, xy_index[59] = 1, z_index[39] = 0, z_index[59] = 1;
  std::vector<double> xy(2 * B * 2), z(2 * B);
  for (int r = 0; r < 2; r++)
    for (int64_t b = 0; b < B; b++) {
      xy[(r * B + b) * 2] = pos[b * 3] + 0.1 * n01(rng);
      xy[(r * B + b) * 2 + 1] = pos[b * 3 + 1] + 0.1 * n01(rng);
      z[r * B + b] = pos[b * 3 + 2] + 0.1 * n01(rng);
    }
  uwvk_pose_fixes fx{};
  fx.host_flags = fix_flags.data();
  fx.xy_index = xy_index.data();
  fx.z_index = z_index.data();
  fx.xy = upload(xy);
  fx.z = upload(z);
  fx.n_xy = fx.n_z = 2;
  fx.xy_cov[0] = 0.01, fx.xy_cov[3] = 0.02;
  fx.z_cov = 0.0025;
  fx.accept_counts = upload(std::vector<uint32_t>((size_t)B * 3, 0u));

  fa.runLogFixes(log, fx, 0, E);
  fa.synchronize();
  // the same run cut at the fix epochs, the fixes as single calls
  uint8_t* acc_null = nullptr;
  int64_t first = 0;
  for (int64_t e : {19, 39, 59}) {
    fb.runLog(log, first, e + 1 - first);
    if (fix_flags[e] & UWVK_FIX_XY)
      U::check(uwvk_pose_update_xy(fb.handle(), &xy[(size_t)xy_index[e] * B * 2], nullptr, fx.xy_cov, nullptr, acc_null),
               "uwvk_pose_update_xy");
    if (fix_flags[e] & UWVK_FIX_Z)
      U::check(uwvk_pose_update_z(fb.handle(), &z[(size_t)z_index[e] * B], nullptr, &fx.z_cov, nullptr, acc_null),
               "uwvk_pose_update_z");
    first = e + 1;
  }
  std::vector<double> xa, Pa, xb, Pb;
  fa.getState(xa, &Pa);
  fb.getState(xb, &Pb);
  const bool same = xa == xb && Pa == Pb;
  std::vector<uint32_t> counts((size_t)B * 3);
  U::check(uwvk_memcpy_d2h(counts.data(), fx.accept_counts, counts.size() * 4), "uwvk_memcpy_d2h");
  bool counted = true;
  for (int64_t b = 0; b < B; b++) counted = counted && counts[b * 3] == 2 && counts[b * 3 + 1] == 2 && counts[b * 3 + 2] == 0;
  // the fixes pulled the position towards the payload: the state differs from the filter's prior
  bool moved = false;
  for (int64_t b = 0; b < B; b++) moved = moved || xa[b * fa.store()] != pos[b * 3];
  // a row out of range throws (UWVK_EINVAL) and leaves the state alone
  bool threw = false;
  try {
    std::vector<int32_t> bad = xy_index;
    bad[19] = 2;
    uwvk_pose_fixes fbad = fx;
    fbad.xy_index = bad.data();
    fa.runLogFixes(log, fbad, 0, E);
  } catch (const U::Error& e) {
    threw = e.code == UWVK_EINVAL;
  }
  std::vector<double> x2;
  fa.getState(x2);
  std::printf("fix facade: same %d, counted %d, moved %d, einval %d, untouched %d\n", (int)same, (int)counted,
              (int)moved, (int)threw, (int)(x2 == xa));
  for (const void* p : {(const void*)log.flags, (const void*)log.gyro, (const void*)log.acc,
                        (const void*)log.dvl_index, (const void*)log.dvl, (const void*)fx.xy, (const void*)fx.z,
                        (const void*)fx.accept_counts})
    uwvk_device_free(const_cast<void*>(p));
  return (same && counted && moved && threw && x2 == xa) ? 0 : 1;
}
