// vel_run_facade_test.cpp — VelocityUKF::runLog / runLogTrack through the C++
// facade: a 20-epoch log at batch 1 (DVL every third epoch, pressure every
// second) in two adjacent runLogTrack calls on the lane-per-filter layout must
// be bitwise the facade's own integrateMeasurement / predictionStep sequence on
// a second filter and runLog on a third, and the one record (after epoch 19)
// bitwise getState.  Exit 0 = equal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "uwv_kalman_filters_amd/PoseUKF.hpp"

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
  const int64_t B = 1, E = 20;
  const double dt = 0.02;
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
  const std::vector<double> x0 = {1.0, 0.2, -0.1, -10.0};
  std::vector<double> P0(16, 0.0);
  for (int k = 0; k < 4; k++) P0[k * 5] = 0.01;
  const std::array<double, 9> dcov = {1e-3, 0, 0, 0, 1e-3, 0, 0, 0, 1e-3};
  const double pcov = 1e-3;

  std::vector<uint32_t> flags(E, 0);
  std::vector<int32_t> di(E, -1), pi(E, -1);
  std::vector<double> gyro(E * B * 3), eff(E * B * 6), dvl, prs;
  for (int64_t e = 0; e < E; e++) {
    for (int k = 0; k < 3; k++) gyro[e * 3 + k] = (k == 2 ? 0.3 : 0.0) + 0.02 * n01(rng);
    for (int k = 0; k < 6; k++) eff[e * 6 + k] = 5.0 * n01(rng);
    if (e % 3 == 2) {
      flags[e] |= UWVK_EV_DVL;
      di[e] = (int32_t)(dvl.size() / 3);
      for (int k = 0; k < 3; k++) dvl.push_back(x0[k] + 0.05 * n01(rng));
    }
    if (e % 2 == 0) {
      flags[e] |= UWVK_EV_PRESSURE;
      pi[e] = (int32_t)prs.size();
      prs.push_back(x0[3] + 0.05 * n01(rng));
    }
  }
  uwvk_vel_log log{};
  log.epochs = E;
  log.dt = dt;
  log.flags = upload(flags);
  log.gyro = upload(gyro);
  log.efforts = upload(eff);
  log.dvl_index = upload(di);
  log.dvl = upload(dvl);
  std::memcpy(log.dvl_cov, dcov.data(), sizeof(log.dvl_cov));
  log.pressure_index = upload(pi);
  log.pressure = upload(prs);
  log.pressure_cov = pcov;
  uwvk_vel_log_host host{};
  host.flags = flags.data();
  host.dvl_index = di.data();
  host.n_dvl = (int64_t)(dvl.size() / 3);
  host.pressure_index = pi.data();
  host.n_pressure = (int64_t)prs.size();

  U::VelocityUKF run(B, x0, P0), plain(B, x0, P0), step(B, x0, P0);
  for (U::VelocityUKF* f : {&run, &plain, &step}) {
    f->setupMotionModel(uwv);
    f->setLaneGroups(0);  // the single calls' arithmetic
  }
  std::vector<double> rec(8, -1.0);
  double* d_rec = upload(rec);
  uwvk_vel_track track{};
  track.every = E;
  track.capacity = 1;
  track.mean = d_rec;
  track.variance = d_rec + 4;
  run.runLogTrack(log, host, 0, 8);
  run.runLogTrack(log, host, 8, E - 8, nullptr, &track);
  run.synchronize();
  plain.runLog(log, 0, E);
  plain.synchronize();
  for (int64_t e = 0; e < E; e++) {
    U::batch::GyroMeasurement g;
    g.mu.assign(gyro.begin() + e * 3, gyro.begin() + (e + 1) * 3);
    step.integrateMeasurement(g);
    U::batch::VelBodyEffortsMeasurement t;
    t.mu.assign(eff.begin() + e * 6, eff.begin() + (e + 1) * 6);
    step.integrateMeasurement(t);
    step.predictionStep(dt);
    if (flags[e] & UWVK_EV_DVL) {
      U::batch::DVLMeasurement z;
      z.mu.assign(dvl.begin() + di[e] * 3, dvl.begin() + (di[e] + 1) * 3);
      z.shared_cov = dcov;
      step.integrateMeasurement(z);
    }
    if (flags[e] & UWVK_EV_PRESSURE) {
      U::batch::PressureMeasurement z;
      z.mu.assign(1, prs[pi[e]]);
      z.shared_cov = {pcov};
      step.integrateMeasurement(z);
    }
  }
  std::vector<double> xa, Pa, xb, Pb, xc, Pc;
  run.getState(xa, &Pa);
  step.getState(xb, &Pb);
  plain.getState(xc, &Pc);
  const bool same_step = std::memcmp(xa.data(), xb.data(), 32) == 0 && std::memcmp(Pa.data(), Pb.data(), 128) == 0;
  const bool same_plain = std::memcmp(xa.data(), xc.data(), 32) == 0 && std::memcmp(Pa.data(), Pc.data(), 128) == 0;
  const bool moved = std::memcmp(xa.data(), x0.data(), 8) != 0;
  U::check(uwvk_memcpy_d2h(rec.data(), d_rec, 64), "uwvk_memcpy_d2h");
  bool record = std::memcmp(rec.data(), xa.data(), 32) == 0;
  for (int k = 0; k < 4; k++) record = record && std::memcmp(&rec[4 + k], &Pa[k * 5], 8) == 0;
  // a host index past the payload throws (UWVK_EINVAL) and leaves the state alone
  bool threw = false;
  di[2] = (int32_t)host.n_dvl;
  try {
    run.runLogTrack(log, host, 0, E);
  } catch (const U::Error& e) {
    threw = e.code == UWVK_EINVAL;
  }
  std::vector<double> x2;
  run.getState(x2);
  std::printf("vel run facade: single calls %d, runLog %d, moved %d, record %d, einval %d, untouched %d\n",
              (int)same_step, (int)same_plain, (int)moved, (int)record, (int)threw, (int)(x2 == xa));
  for (const void* p : {(const void*)log.flags, (const void*)log.gyro, (const void*)log.efforts,
                        (const void*)log.dvl_index, (const void*)log.dvl, (const void*)log.pressure_index,
                        (const void*)log.pressure, (const void*)d_rec})
    uwvk_device_free(const_cast<void*>(p));
  return (same_step && same_plain && moved && record && threw && x2 == xa) ? 0 : 1;
}
