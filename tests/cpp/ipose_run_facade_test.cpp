// ipose_run_facade_test.cpp — IndirectPoseUKF::runLog through the C++ facade: a
// 6-epoch log at batch 5 (the reference moves every epoch, a dt per epoch, 0, 1
// or 2 marker observations per epoch) in two adjacent calls must be bitwise the
// facade's own updatePoseReference / predictionStep / integrateMeasurement
// sequence on a second filter, and its last corrected-pose record must be
// getCorrectedPose to rounding.  Exit 0 = equal.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "uwv_kalman_filters_amd/IndirectPoseUKF.hpp"

namespace U = uwv_kalman_filters_amd;

static void qmul(const double a[4], const double b[4], double o[4]) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
static void qrot(const double q[4], const double v[3], double o[3], bool inv = false) {
  const double qc[4] = {q[0], inv ? -q[1] : q[1], inv ? -q[2] : q[2], inv ? -q[3] : q[3]};
  const double pv[4] = {0, v[0], v[1], v[2]}, qi[4] = {qc[0], -qc[1], -qc[2], -qc[3]};
  double t[4], r[4];
  qmul(qc, pv, t);
  qmul(t, qi, r);
  o[0] = r[1]; o[1] = r[2]; o[2] = r[3];
}
static void qexp(const double v[3], double q[4]) {
  const double th = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const double s = th > 0 ? std::sin(th / 2) / th : 0.5;
  q[0] = std::cos(th / 2); q[1] = s * v[0]; q[2] = s * v[1]; q[3] = s * v[2];
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
  const int64_t B = 5, E = 6, NF = 4;
  const int64_t offset[E + 1] = {0, 0, 1, 3, 3, 4, 4};
  const double dts[E] = {0.1, 0.05, 0.2, 0.1, 0.15, 0.1};
  const int64_t V = offset[E];
  std::mt19937_64 rng(5);
  std::normal_distribution<double> n01;
  const U::CameraConfiguration cam{600, 620, 320, 240};
  U::Pose7 cam_in;
  cam_in.t = {0.1, 0.0, 0.05};
  cam_in.q = {0.5, -0.5, 0.5, -0.5};  // z_cam = x_body, x_cam = -y_body, y_cam = -z_body
  const std::vector<std::array<double, 3>> corners = {{0.2, 0.2, 0}, {-0.2, 0.2, 0}, {-0.2, -0.2, 0}, {0.2, -0.2, 0}};
  // the scene of facade_small_test.cpp: a marker 3 m ahead of each true body pose
  std::vector<U::Pose7> ref0(B), marker0(B);
  std::vector<double> px0(B * NF * 2);
  for (int64_t b = 0; b < B; b++) {
    double rv[3] = {0.3 * n01(rng), 0.3 * n01(rng), 0.3 * n01(rng)}, ev[3] = {0.02 * n01(rng), 0.02 * n01(rng),
                                                                            0.02 * n01(rng)};
    double qe[4], pe[3] = {0.3 * n01(rng), 0.3 * n01(rng), 0.3 * n01(rng)}, bt[3], bq[4], tmp[3];
    for (int k = 0; k < 3; k++) ref0[b].t[k] = 5 * n01(rng);
    qexp(rv, ref0[b].q.data());
    qexp(ev, qe);
    qrot(ref0[b].q.data(), pe, tmp);
    for (int k = 0; k < 3; k++) bt[k] = ref0[b].t[k] + tmp[k];
    qmul(ref0[b].q.data(), qe, bq);
    const double ahead[3] = {3.0, 0.0, 0.0};
    qrot(bq, ahead, tmp);
    for (int k = 0; k < 3; k++) marker0[b].t[k] = bt[k] + tmp[k];
    for (int k = 0; k < 4; k++) marker0[b].q[k] = bq[k];
    for (int i = 0; i < NF; i++) {
      double fn[3], t[3], w[3], fc[3];
      qrot(marker0[b].q.data(), corners[i].data(), fn);
      for (int k = 0; k < 3; k++) t[k] = fn[k] + marker0[b].t[k] - bt[k];
      qrot(bq, t, w, true);
      for (int k = 0; k < 3; k++) w[k] -= cam_in.t[k];
      qrot(cam_in.q.data(), w, fc, true);
      px0[(b * NF + i) * 2] = cam.fx * fc[0] / fc[2] + cam.cx;
      px0[(b * NF + i) * 2 + 1] = cam.fy * fc[1] / fc[2] + cam.cy;
    }
  }
  // epoch e moves the references and the markers by the same offset: the pixels stay valid
  const double drift[3] = {0.3, -0.2, 0.05};
  std::vector<double> pose_ref(E * B * 7), features(V * B * NF * 2), marker(V * B * 7);
  for (int64_t e = 0; e < E; e++) {
    for (int64_t b = 0; b < B; b++) {
      double* r = &pose_ref[(e * B + b) * 7];
      for (int k = 0; k < 3; k++) r[k] = ref0[b].t[k] + drift[k] * (double)e;
      for (int k = 0; k < 4; k++) r[3 + k] = ref0[b].q[k];
    }
    for (int64_t row = offset[e]; row < offset[e + 1]; row++)
      for (int64_t b = 0; b < B; b++) {
        double* m = &marker[(row * B + b) * 7];
        for (int k = 0; k < 3; k++) m[k] = marker0[b].t[k] + drift[k] * (double)e;
        for (int k = 0; k < 4; k++) m[3 + k] = marker0[b].q[k];
        for (int64_t k = 0; k < NF * 2; k++) features[(row * B + b) * NF * 2 + k] = px0[b * NF * 2 + k] + 0.3 * n01(rng);
      }
  }
  std::array<double, 36> cm{};
  for (int k = 0; k < 6; k++) cm[k * 7] = k < 3 ? 1e-4 : 1e-5;
  const double pixel_var = 4.0;  // two observations in one epoch: see tests/ipose_run_scenes.py
  std::vector<double> fcov(NF * 4, 0.0), fpos;
  for (int i = 0; i < NF; i++) fcov[i * 4] = fcov[i * 4 + 3] = pixel_var;
  for (auto& c : corners) fpos.insert(fpos.end(), c.begin(), c.end());

  uwvk_ipose_log log{};
  log.epochs = E;
  log.dt_epoch = dts;
  log.pose_ref = upload(pose_ref);
  log.visual_offset = offset;
  log.n_visual = V;
  log.n_features = (int32_t)NF;
  log.features = upload(features);
  log.shared_feature_cov = fcov.data();
  log.feature_positions = fpos.data();
  log.marker_pose = upload(marker);
  std::memcpy(log.cov_marker_pose, cm.data(), sizeof(log.cov_marker_pose));
  const double cam4[4] = {cam.fx, cam.fy, cam.cx, cam.cy};
  std::memcpy(log.camera, cam4, sizeof(cam4));
  for (int k = 0; k < 3; k++) log.camera_in_body[k] = cam_in.t[k];
  for (int k = 0; k < 4; k++) log.camera_in_body[3 + k] = cam_in.q[k];

  const std::array<double, 3> ps = {0.1, 0.1, 0.2}, os = {0.01, 0.01, 0.02}, ips = {0.5, 0.5, 0.5};
  U::IndirectPoseUKF run(B, ps, os, 20.0, {}, ips), step(B, ps, os, 20.0, {}, ips);
  std::vector<double> x0;
  run.getState(x0);
  std::vector<double> none(B * 7, 0.0);
  uwvk_ipose_track track{};
  track.every = E;  // the only record epoch is the last one
  track.capacity = 1;
  track.corrected = upload(none);
  run.runLog(log, 0, 2);
  run.runLog(log, 2, E - 2, nullptr, &track);  // one record, after the last epoch
  run.synchronize();
  for (int64_t e = 0; e < E; e++) {
    std::vector<U::Pose7> r(B);
    for (int64_t b = 0; b < B; b++) {
      for (int k = 0; k < 3; k++) r[b].t[k] = pose_ref[(e * B + b) * 7 + k];
      for (int k = 0; k < 4; k++) r[b].q[k] = pose_ref[(e * B + b) * 7 + 3 + k];
    }
    step.updatePoseReference(r);
    step.predictionStep(dts[e]);
    for (int64_t row = offset[e]; row < offset[e + 1]; row++) {
      std::vector<U::VisualFeatureMeasurement> feats(NF);
      std::vector<U::Pose7> mk(B);
      for (int i = 0; i < NF; i++) {
        feats[i].mu.resize(B * 2);
        feats[i].shared_cov = {pixel_var, 0, 0, pixel_var};
        for (int64_t b = 0; b < B; b++) {
          feats[i].mu[b * 2] = features[((row * B + b) * NF + i) * 2];
          feats[i].mu[b * 2 + 1] = features[((row * B + b) * NF + i) * 2 + 1];
        }
      }
      for (int64_t b = 0; b < B; b++) {
        for (int k = 0; k < 3; k++) mk[b].t[k] = marker[(row * B + b) * 7 + k];
        for (int k = 0; k < 4; k++) mk[b].q[k] = marker[(row * B + b) * 7 + 3 + k];
      }
      step.integrateMeasurement(feats, corners, mk, cm, cam, cam_in);
    }
  }
  std::vector<double> xa, Pa, xb, Pb;
  run.getState(xa, &Pa);
  step.getState(xb, &Pb);
  const bool same_x = std::memcmp(xa.data(), xb.data(), xa.size() * 8) == 0;
  const bool same_P = std::memcmp(Pa.data(), Pb.data(), Pa.size() * 8) == 0;
  const bool moved = std::memcmp(xa.data(), x0.data(), xa.size() * 8) != 0;
  // the handle's reference is the last epoch's: getCorrectedPose agrees bitwise, the record to rounding
  const std::vector<U::Pose7> ca = run.getCorrectedPose(), cb = step.getCorrectedPose();
  std::vector<double> rec(B * 7);
  U::check(uwvk_memcpy_d2h(rec.data(), track.corrected, rec.size() * 8), "uwvk_memcpy_d2h");
  bool same_c = true, rec_c = true;
  const double eps = std::ldexp(1.0, -52);
  for (int64_t b = 0; b < B; b++) {
    same_c = same_c && ca[b].t == cb[b].t && ca[b].q == cb[b].q;
    double tr = 0.0, pe = 0.0;
    for (int k = 0; k < 3; k++) {
      tr = std::fmax(tr, std::fabs(pose_ref[((E - 1) * B + b) * 7 + k]));
      pe = std::fmax(pe, std::fabs(xa[b * 7 + k]));
    }
    for (int k = 0; k < 3; k++) rec_c = rec_c && std::fabs(rec[b * 7 + k] - ca[b].t[k]) <= 32 * eps * (tr + 4 * pe);
    for (int k = 0; k < 4; k++) rec_c = rec_c && std::fabs(rec[b * 7 + 3 + k] - ca[b].q[k]) <= 16 * eps;
  }
  // an invalid range throws (UWVK_EINVAL) and leaves the state alone
  bool threw = false;
  try {
    run.runLog(log, 0, E + 1);
  } catch (const U::Error& e) {
    threw = e.code == UWVK_EINVAL;
  }
  std::vector<double> x2;
  run.getState(x2);
  std::printf("ipose run facade: mean %d, covariance %d, moved %d, corrected %d, record %d, einval %d, untouched %d\n",
              (int)same_x, (int)same_P, (int)moved, (int)same_c, (int)rec_c, (int)threw, (int)(x2 == xa));
  for (const void* p : {(const void*)log.pose_ref, (const void*)log.features, (const void*)log.marker_pose,
                        (const void*)track.corrected})
    uwvk_device_free(const_cast<void*>(p));
  return (same_x && same_P && moved && same_c && rec_c && threw && x2 == xa) ? 0 : 1;
}
