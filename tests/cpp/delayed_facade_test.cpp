// delayed_facade_test.cpp — PoseUKF::runLogDelayed through the C++ facade: 60
// IMU epochs at batch 4 with an XY fix after epoch 19, a Z fix after 39 and the
// delayed XY rows (latch, arrival) = (9, 19), (19, 39), (45, 59), against a second
// filter that runs runLog cut at every latch, fix and arrival epoch with
// uwvk_pose_update_xy / _z / _delayed_xy at the cuts, delayed_xy being the
// position getState returned at the row's latch cut.  The states, the latched
// rows and the accept counts must be bitwise equal, and a latch epoch at its
// arrival must throw (UWVK_EINVAL) and leave the state alone.  Exit 0 = all of that.
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

  // XY after epoch 19 (row 0), Z after 39 (row 0)
  std::vector<uint32_t> fix_flags(E, 0u);
  std::vector<int32_t> xy_index(E, -1), z_index(E, -1);
  fix_flags[19] = UWVK_FIX_XY, fix_flags[39] = UWVK_FIX_Z;
  xy_index[19] = 0, z_index[39] = 0;
  std::vector<double> xy(B * 2), z(B);
  for (int64_t b = 0; b < B; b++) {
    xy[b * 2] = pos[b * 3] + 0.1 * n01(rng);
    xy[b * 2 + 1] = pos[b * 3 + 1] + 0.1 * n01(rng);
    z[b] = pos[b * 3 + 2] + 0.1 * n01(rng);
  }
  uwvk_pose_fixes fx{};
  fx.host_flags = fix_flags.data();
  fx.xy_index = xy_index.data();
  fx.z_index = z_index.data();
  fx.xy = upload(xy);
  fx.z = upload(z);
  fx.n_xy = fx.n_z = 1;
  fx.xy_cov[0] = 0.01, fx.xy_cov[3] = 0.02;
  fx.z_cov = 0.0025;

  // delayed rows: latched after epochs 9, 19, 45, arriving at 19 (the XY epoch), 39 (the Z epoch), 59 (the last)
  const int R = 3;
  const std::vector<int32_t> latch_epoch = {9, 19, 45};
  std::vector<int32_t> index(E, -1);
  index[19] = 0, index[39] = 1, index[59] = 2;
  std::vector<double> dxy((size_t)R * B * 2);
  for (size_t k = 0; k < dxy.size(); k++) dxy[k] = pos[((k / 2) % B) * 3 + (k % 2)] + 0.2 * n01(rng);
  uwvk_pose_delayed dl{};
  dl.index = index.data();
  dl.latch_epoch = latch_epoch.data();
  dl.xy = upload(dxy);
  dl.n = R;
  dl.xy_cov[0] = 0.0025, dl.xy_cov[3] = 0.0036;
  dl.latched = upload(std::vector<double>((size_t)R * B * 2, 0.0));
  dl.accept_counts = upload(std::vector<uint32_t>((size_t)B, 0u));

  fa.runLogDelayed(log, &fx, dl, 0, E);
  fa.synchronize();
  // the same run cut at every event epoch, the updates as single calls, the latches through getState
  uint8_t* acc_null = nullptr;
  std::vector<double> latched((size_t)R * B * 2, 0.0), xs;
  int64_t first = 0;
  for (int64_t e : {9, 19, 39, 45, 59}) {
    fb.runLog(log, first, e + 1 - first);
    if (fix_flags[e] & UWVK_FIX_XY)
      U::check(uwvk_pose_update_xy(fb.handle(), &xy[(size_t)xy_index[e] * B * 2], nullptr, fx.xy_cov, nullptr, acc_null),
               "uwvk_pose_update_xy");
    if (fix_flags[e] & UWVK_FIX_Z)
      U::check(uwvk_pose_update_z(fb.handle(), &z[(size_t)z_index[e] * B], nullptr, &fx.z_cov, nullptr, acc_null),
               "uwvk_pose_update_z");
    if (index[e] >= 0)
      U::check(uwvk_pose_update_delayed_xy(fb.handle(), &dxy[(size_t)index[e] * B * 2], nullptr, dl.xy_cov,
                                           &latched[(size_t)index[e] * B * 2], nullptr, acc_null),
               "uwvk_pose_update_delayed_xy");
    for (int r = 0; r < R; r++)
      if (latch_epoch[r] == e) {
        fb.getState(xs);
        for (int64_t b = 0; b < B; b++)
          for (int c = 0; c < 2; c++) latched[((size_t)r * B + b) * 2 + c] = xs[b * fb.store() + c];
      }
    first = e + 1;
  }
  std::vector<double> xa, Pa, xb, Pb;
  fa.getState(xa, &Pa);
  fb.getState(xb, &Pb);
  const bool same = xa == xb && Pa == Pb;
  std::vector<double> got_latched(latched.size());
  U::check(uwvk_memcpy_d2h(got_latched.data(), dl.latched, got_latched.size() * 8), "uwvk_memcpy_d2h");
  const bool same_latched = got_latched == latched;
  std::vector<uint32_t> counts((size_t)B);
  U::check(uwvk_memcpy_d2h(counts.data(), dl.accept_counts, counts.size() * 4), "uwvk_memcpy_d2h");
  bool counted = true;
  for (int64_t b = 0; b < B; b++) counted = counted && counts[b] == 3;
  // without the delayed rows the state is another one
  U::PoseUKF fc(B, pos, pos_cov, rot, rot_cov, cfg, uwv);
  fc.setProcessNoiseFromConfig(cfg, dt);
  fc.runLogFixes(log, fx, 0, E);
  fc.synchronize();
  std::vector<double> xc;
  fc.getState(xc);
  const bool moved = xc != xa;
  // a row latched at its arrival epoch throws (UWVK_EINVAL) and leaves the state alone
  bool threw = false;
  try {
    std::vector<int32_t> bad = latch_epoch;
    bad[1] = 39;
    uwvk_pose_delayed dbad = dl;
    dbad.latch_epoch = bad.data();
    fa.runLogDelayed(log, nullptr, dbad, 0, E);
  } catch (const U::Error& e) {
    threw = e.code == UWVK_EINVAL;
  }
  std::vector<double> x2;
  fa.getState(x2);
  std::printf("delayed facade: same %d, latched %d, counted %d, moved %d, einval %d, untouched %d\n", (int)same,
              (int)same_latched, (int)counted, (int)moved, (int)threw, (int)(x2 == xa));
  for (const void* p : {(const void*)log.flags, (const void*)log.gyro, (const void*)log.acc,
                        (const void*)log.dvl_index, (const void*)log.dvl, (const void*)fx.xy, (const void*)fx.z,
                        (const void*)dl.xy, (const void*)dl.latched, (const void*)dl.accept_counts})
    uwvk_device_free(const_cast<void*>(p));
  return (same && same_latched && counted && moved && threw && x2 == xa) ? 0 : 1;
}
