// uwvk_sched.cpp — recorded-mission ingestion: the event-ordered replay that
// the reference leaves to its caller (the Rock orogen task and its stream
// aligner), turned into the epoch-indexed log the
// persistent run_log kernels consume (uwvk_pose_log / uwvk_vel_log).
//
// Host-only integer/index work, run once per recording: no device code here.
//
// Semantics:
//  * every IMU sample opens one epoch: RotationRate -> predictionStep(dt) ->
//    Acceleration (PoseUKF.cpp:446-496), dt the mean IMU interval; the IMU
//    stream must be uniform to within dt_tolerance * dt (else UWVK_EINVAL:
//    split the recording at the gap and replay the pieces with their own dt);
//  * a lower-rate sample stamped t is released at the first IMU epoch whose
//    stamp is >= t - time_epsilon (the aligner releases it once the IMU stream
//    has passed it) and integrated after that epoch's predict + acceleration
//    update, in the fixed order DVL, pressure, ADCP cells, BodyEfforts, then
//    the position fixes (uwvk_schedule_fixes) XY, Z, Geographic;
//  * two samples of one sensor landing in one epoch are queued: the later
//    one moves to the next free epoch (order is kept, nothing is merged);
//  * samples before the first IMU stamp or queued past the last epoch are
//    dropped and counted;
//  * a delayed XY sample (uwvk_schedule_delayed) has two stamps: the filter's
//    position is latched at the epoch its measurement stamp is released at, and
//    the update runs, after Geographic, at the epoch its arrival stamp is
//    released at, at least one epoch later.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/uwvk.h"

namespace {

// assign the ascending stamps t[0..n) to epochs of imu[0..E); returns dropped
int64_t place(const double* imu, int64_t E, const double* t, int64_t n, double eps, uint32_t bit,
              uint32_t* flags, int32_t* index, const uint8_t* extra, uint32_t extra_bit) {
  for (int64_t e = 0; e < E; e++) index[e] = -1;
  int64_t dropped = 0, e = 0, next_free = 0;
  int32_t row = 0;
  for (int64_t s = 0; s < n; s++) {
    const double ts = t[s];
    if (!(ts >= imu[0] - eps)) {  // before the first epoch (or NaN stamp)
      dropped++;
      continue;
    }
    while (e < E && imu[e] < ts - eps) e++;
    int64_t at = e > next_free ? e : next_free;
    if (at >= E) {
      dropped++;
      continue;
    }
    flags[at] |= bit;
    if (extra && extra[s]) flags[at] |= extra_bit;
    index[at] = row++;  // rows of the per-sensor payload are the kept samples, in order
    next_free = at + 1;
  }
  return dropped;
}

bool ascending(const double* t, int64_t n) {
  for (int64_t i = 1; i < n; i++)
    if (!(t[i] >= t[i - 1])) return false;
  return true;
}

}  // namespace

extern "C" uwvk_status uwvk_schedule_streams(const uwvk_stream_times* in, double dt_tolerance, double time_epsilon,
                                             uwvk_schedule* out) {
  if (!in || !out || !in->imu || in->n_imu < 1 || !out->flags) return UWVK_EINVAL;
  if (!(dt_tolerance >= 0.0) || !(time_epsilon >= 0.0)) return UWVK_EINVAL;
  const int64_t E = in->n_imu;
  const double* imu = in->imu;
  if (!ascending(imu, E)) return UWVK_EINVAL;
  double dt = 0.0;
  if (E > 1) {
    dt = (imu[E - 1] - imu[0]) / (double)(E - 1);
    if (!(dt > 0.0)) return UWVK_EINVAL;
    for (int64_t e = 1; e < E; e++)
      if (std::fabs((imu[e] - imu[e - 1]) - dt) > dt_tolerance * dt) return UWVK_EINVAL;
  }
  out->dt = dt;
  out->epochs = E;
  for (int64_t e = 0; e < E; e++) out->flags[e] = UWVK_EV_ACC;
  struct K {
    const double* t;
    int64_t n;
    int32_t* idx;
    uint32_t bit;
  } ks[4] = {{in->dvl, in->n_dvl, out->dvl_index, UWVK_EV_DVL},
             {in->pressure, in->n_pressure, out->pressure_index, UWVK_EV_PRESSURE},
             {in->adcp, in->n_adcp, out->adcp_index, UWVK_EV_ADCP},
             {in->efforts, in->n_efforts, out->efforts_index, UWVK_EV_EFFORTS}};
  for (int k = 0; k < 4; k++) {
    out->kept[k] = 0;
    out->dropped[k] = 0;
    if (ks[k].n < 0 || (ks[k].n > 0 && !ks[k].t)) return UWVK_EINVAL;
    if (!ks[k].idx) {
      if (ks[k].n > 0) return UWVK_EINVAL;
      continue;
    }
    if (!ascending(ks[k].t, ks[k].n)) return UWVK_EINVAL;
    const uint8_t* extra = k == 3 ? in->efforts_velocity_only : nullptr;
    out->dropped[k] = place(imu, E, ks[k].t, ks[k].n, time_epsilon, ks[k].bit, out->flags, ks[k].idx, extra,
                            UWVK_EV_EFFORTS_VELOCITY_ONLY);
    out->kept[k] = ks[k].n - out->dropped[k];
  }
  return UWVK_OK;
}

// The position fixes of a recording (uwvk_pose_fixes): XY, Z and GPS stamps
// placed on the IMU epochs by the same place() as the other sensors, into
// their own flags array (UWVK_FIX_*).
extern "C" uwvk_status uwvk_schedule_fixes(const double* imu, int64_t n_imu, const double* xy_t, int64_t n_xy,
                                           const double* z_t, int64_t n_z, const double* geo_t, int64_t n_geo,
                                           double time_epsilon, uint32_t* flags, int32_t* xy_index, int32_t* z_index,
                                           int32_t* geo_index, int64_t kept[3], int64_t dropped[3]) {
  if (!imu || n_imu < 1 || !flags || !kept || !dropped || !(time_epsilon >= 0.0)) return UWVK_EINVAL;
  if (!ascending(imu, n_imu)) return UWVK_EINVAL;
  struct K {
    const double* t;
    int64_t n;
    int32_t* idx;
    uint32_t bit;
  } ks[3] = {{xy_t, n_xy, xy_index, UWVK_FIX_XY}, {z_t, n_z, z_index, UWVK_FIX_Z}, {geo_t, n_geo, geo_index, UWVK_FIX_GEO}};
  for (int k = 0; k < 3; k++) {
    if (ks[k].n < 0 || (ks[k].n > 0 && (!ks[k].t || !ks[k].idx))) return UWVK_EINVAL;
    if (!ascending(ks[k].t, ks[k].n)) return UWVK_EINVAL;
  }
  for (int64_t e = 0; e < n_imu; e++) flags[e] = 0;
  for (int k = 0; k < 3; k++) {
    kept[k] = 0;
    dropped[k] = 0;
    if (!ks[k].idx) continue;
    dropped[k] = place(imu, n_imu, ks[k].t, ks[k].n, time_epsilon, ks[k].bit, flags, ks[k].idx, nullptr, 0);
    kept[k] = ks[k].n - dropped[k];
  }
  return UWVK_OK;
}

// Delayed XY samples (uwvk_pose_delayed): the stamp placed by the rule of
// place() gives the latch epoch, the arrival placed the same way, but not before
// L + 1 and queued behind the arrival before it, gives the arrival epoch.
extern "C" uwvk_status uwvk_schedule_delayed(const double* imu, int64_t n_imu, const double* stamp_t,
                                             const double* arrival_t, int64_t n, double time_epsilon, int32_t* index,
                                             int32_t* latch_epoch, int64_t* kept, int64_t* dropped) {
  if (!imu || n_imu < 1 || !index || !kept || !dropped || !(time_epsilon >= 0.0) || n < 0) return UWVK_EINVAL;
  if (n > 0 && (!stamp_t || !arrival_t || !latch_epoch)) return UWVK_EINVAL;
  if (!ascending(imu, n_imu) || !ascending(stamp_t, n) || !ascending(arrival_t, n)) return UWVK_EINVAL;
  for (int64_t s = 0; s < n; s++)
    if (!(arrival_t[s] >= stamp_t[s])) return UWVK_EINVAL;  // (a NaN stamp too)
  const int64_t E = n_imu;
  const double eps = time_epsilon;
  for (int64_t e = 0; e < E; e++) index[e] = -1;
  int64_t lost = 0, el = 0, ea = 0, next_free = 0;
  int32_t row = 0;
  for (int64_t s = 0; s < n; s++) {
    if (!(stamp_t[s] >= imu[0] - eps)) {  // stamped before the first epoch
      lost++;
      continue;
    }
    while (el < E && imu[el] < stamp_t[s] - eps) el++;
    while (ea < E && imu[ea] < arrival_t[s] - eps) ea++;
    int64_t at = ea > el + 1 ? ea : el + 1;
    if (next_free > at) at = next_free;
    if (at >= E) {  // (el >= E lands here too)
      lost++;
      continue;
    }
    index[at] = row;
    latch_epoch[row++] = (int32_t)el;
    next_free = at + 1;
  }
  *kept = n - lost;
  *dropped = lost;
  return UWVK_OK;
}

// ADCP cell weighting for PoseUKF::integrateMeasurement(WaterVelocityMeasurement,
// cell_weighting) (PoseUKF.cpp:133-151, 604-611): the weight of the deeper
// water layer in cell i.  Cell centres sit at r_i = first_cell_blank +
// (i + 1/2) cell_size from the transducer (PoseUKFConfig.hpp:34-38); the
// nearest cell measures the vehicle's layer (weight 0), the farthest the layer
// below (weight 1), linear in range between.  Cells whose beam correlation is
// below minimum_correlation (PoseUKFConfig.hpp:40-41) are marked invalid (the
// caller skips them).  The reference computes this in its caller; this rule
// is the engine's (unpinned).
extern "C" uwvk_status uwvk_adcp_cell_weighting(const uwvk_water_velocity* wv, int32_t cells,
                                                const double* correlation, double* weighting, uint8_t* valid) {
  if (!wv || cells < 1 || cells > 64 || !weighting) return UWVK_EINVAL;
  if (!(wv->cell_size > 0.0) || !(wv->first_cell_blank >= 0.0)) return UWVK_EINVAL;
  const double r0 = wv->first_cell_blank + 0.5 * wv->cell_size;
  const double r1 = wv->first_cell_blank + (cells - 0.5) * wv->cell_size;
  for (int32_t i = 0; i < cells; i++) {
    const double r = wv->first_cell_blank + (i + 0.5) * wv->cell_size;
    weighting[i] = cells == 1 ? 0.0 : (r - r0) / (r1 - r0);
    if (valid) valid[i] = correlation ? (uint8_t)(correlation[i] >= wv->minimum_correlation) : (uint8_t)1;
  }
  return UWVK_OK;
}
