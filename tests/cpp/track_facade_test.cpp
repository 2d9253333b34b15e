// track_facade_test.cpp — PoseUKF::runLogTrack through the C++ facade: 60 IMU
// epochs at batch 4 with a record every 20; the last record (after epoch 59,
// the end of the run) must be bitwise the state getState reads back, and the
// variances its covariance's diagonal.  Exit 0 = equal.
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
  const int64_t B = 4, E = 60, every = 20;
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
  U::PoseUKF f(B, pos, pos_cov, rot, rot_cov, cfg, uwv);
  f.setProcessNoiseFromConfig(cfg, dt);

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

  const int64_t records = uwvk_pose_track_records(0, E, every);
  const size_t s = f.store(), n = (size_t)f.dof();
  uwvk_pose_track track{};
  track.every = every;
  track.capacity = records;
  track.mean = upload(std::vector<double>((size_t)records * B * s, -1.0));
  track.variance = upload(std::vector<double>((size_t)records * B * n, -1.0));
  f.runLogTrack(log, 0, E, track);
  f.synchronize();

  std::vector<double> mean((size_t)records * B * s), var((size_t)records * B * n), x, P;
  U::check(uwvk_memcpy_d2h(mean.data(), track.mean, mean.size() * 8), "uwvk_memcpy_d2h");
  U::check(uwvk_memcpy_d2h(var.data(), track.variance, var.size() * 8), "uwvk_memcpy_d2h");
  f.getState(x, &P);
  const double* last_mean = &mean[(size_t)(records - 1) * B * s];
  const double* last_var = &var[(size_t)(records - 1) * B * n];
  const bool mean_ok = std::memcmp(last_mean, x.data(), B * s * 8) == 0;
  bool var_ok = true, earlier_written = true;
  for (int64_t b = 0; b < B; b++)
    for (size_t d = 0; d < n; d++) var_ok = var_ok && last_var[b * n + d] == P[b * n * n + d * n + d];
  // the earlier records were written too (no -1 left) and differ from the last
  for (size_t k = 0; k < (size_t)(records - 1) * B * n; k++) earlier_written = earlier_written && var[k] > 0;
  const bool moved = std::memcmp(&mean[0], last_mean, B * s * 8) != 0;
  // an invalid track throws (UWVK_EINVAL) and leaves the state alone
  bool threw = false;
  try {
    uwvk_pose_track bad = track;
    bad.every = 0;
    f.runLogTrack(log, 0, E, bad);
  } catch (const U::Error& e) {
    threw = e.code == UWVK_EINVAL;
  }
  std::vector<double> x2;
  f.getState(x2);
  std::printf("track facade: records %lld, mean %d, variance %d, earlier %d, moved %d, einval %d, untouched %d\n",
              (long long)records, (int)mean_ok, (int)var_ok, (int)earlier_written, (int)moved, (int)threw,
              (int)(x2 == x));
  for (const void* p : {(const void*)log.flags, (const void*)log.gyro, (const void*)log.acc,
                        (const void*)log.dvl_index, (const void*)log.dvl, (const void*)track.mean,
                        (const void*)track.variance})
    uwvk_device_free(const_cast<void*>(p));
  return (records == 3 && mean_ok && var_ok && earlier_written && moved && threw && x2 == x) ? 0 : 1;
}
