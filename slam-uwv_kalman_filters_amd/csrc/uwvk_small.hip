// uwvk_small.hip — BottomUKF (src/BottomUKF.hpp:26-53) and IndirectPoseUKF
// (src/IndirectPoseUKF.hpp:28-86) on gfx950, batched, and their uwvk_bottom_* /
// uwvk_ipose_* C ABI.
//
// Both are small-state filters: one instance per lane group, one sigma point
// per lane (uwvk_aug_dev.hpp): BottomUKF 8 lanes (8 instances per wave),
// IndirectPoseUKF 16 lanes (4 per wave), its marker-augmented visual update
// 32 lanes (2 per wave).  Sigma lives in LDS for the duration of a call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "uwvk_aug_dev.hpp"
#include "../../include/uwvk.h"
#include "uwvk_host.hpp"
#include "uwvk_plan.hpp"
#include "uwvk_stage.hpp"
#include "uwvk_visual_rows.hpp"

using namespace uwvk;
using namespace uwvk::aug;

namespace {

using BottomM = Manifold<Seg<SEG_V, 1>, Seg<SEG_S2>>;                        // BottomUKF.hpp:18-21
// IndirectPoseUKF's orientation_error is an MTK::SO3 like PoseUKF's orientation:
// SR = 1 the body-frame [+] q exp(d) (MTK's SO3::boxplus, the default), 0 nav-frame
template <int SR>
using SO3Seg = Seg<SR ? SEG_SO3R : SEG_SO3>;
template <int SR>
using IPoseM = Manifold<Seg<SEG_V, 3>, SO3Seg<SR>>;                          // IndirectPoseUKF.hpp:19-22
template <int SR>
using IPoseMarkerM = Manifold<Seg<SEG_V, 3>, SO3Seg<SR>, Seg<SEG_V, 3>, SO3Seg<SR>>;  // IndirectPoseUKF.cpp:25-29
using BE = Engine<BottomM>;
template <int SR>
using IE = Engine<IPoseM<SR>>;
template <int SR>
using IAE = Engine<IPoseMarkerM<SR>>;

struct SmallBufs {
  int64_t batch;
  double* mu;        // [batch][store]
  double* sigma;     // [batch][n*n]
  uint32_t* status;  // [batch]
};

struct M9 { double v[9]; };
struct M36 { double v[36]; };

// load / store one instance's (mu, Sigma) between HBM and its LDS words
template <class E>
__device__ void load(E& e, const SmallBufs& b, int64_t inst) {
  if (e.live) {
    for (int i = e.g; i < E::n * E::n; i += E::G) e.sm[E::o_sig + i] = b.sigma[inst * E::n * E::n + i];
    for (int k = e.g; k < E::S; k += E::G) e.sm[E::o_mu + k] = b.mu[inst * E::S + k];
  }
  __syncthreads();
}
template <class E>
__device__ void store(E& e, const SmallBufs& b, int64_t inst, bool ok) {
  if (e.live && ok) {
    for (int i = e.g; i < E::n * E::n; i += E::G) b.sigma[inst * E::n * E::n + i] = e.sm[E::o_sig + i];
    for (int k = e.g; k < E::S; k += E::G) b.mu[inst * E::S + k] = e.sm[E::o_mu + k];
  }
  if (e.live && !ok && e.g == 0) b.status[inst] |= UWVK_ST_NOTPD;
}

template <class E>
__device__ E make_engine(double* smem, const SmallBufs& b, const uint8_t* mask, int64_t* inst) {
  const int gi = threadIdx.x / E::G;
  E e;
  e.g = threadIdx.x % E::G;
  e.sm = smem + gi * E::words;
  *inst = (int64_t)blockIdx.x * E::IPB + gi;
  e.live = *inst < b.batch && (!mask || mask[*inst]);
  return e;
}

// ---- BottomUKF -----------------------------------------------------------
// The three step bodies, on an engine whose (mu, Sigma) is in LDS.  The single
// kernels and k_bottom_run both call them, so both compile the same
// expressions: the run's bitwise contract (include/uwvk.h) rests on that.
// The inputs of an instance are read only if it is e.live; predict and range
// read them themselves, at row `at` of the caller's arrays.

// predictionStepImpl (BottomUKF.cpp:48-54) + processModel (:5-16); vel: [..][3]
UWVK_DEV bool bottom_predict_step(BE& e, const double* vel, int64_t at, const M9& Q, double dt) {
  double vz = 0.0, s = 0.0;
  if (e.live) {
    const double vx = vel[at * 3], vy = vel[at * 3 + 1];
    vz = vel[at * 3 + 2];
    const double nrm = sqrt(vx * vx + vy * vy);
    s = (nrm * nrm) * (dt * dt);  // pow(|v_xy|, 2) * pow(dt, 2)
  }
  return e.predict([&](double* x) { x[0] = x[0] + (-1.0 * vz) * dt; },
                   [&](int r, int c) { return s * Q.v[r * 3 + c]; });
}

// measurementDistance (BottomUKF.cpp:18-30)
struct RangeH {
  double dir[3], origin[3];
  UWVK_DEV void operator()(const double* x, double* z) const {
    const double bottom[3] = {0.0, 0.0, -x[0]};
    const double v = dir[0] * x[1] + dir[1] * x[2] + dir[2] * x[3];
    if (v != 0.0)
      z[0] = ((bottom[0] - origin[0]) * x[1] + (bottom[1] - origin[1]) * x[2] + (bottom[2] - origin[2]) * x[3]) / v;
    else
      z[0] = 0.0;
  }
};

// integrateMeasurement(RangeMeasurement, unit_direction, origin) (BottomUKF.cpp:56-61):
// DistanceType (mtkwrap<Scalar>) measurement -> iterative vect mean
UWVK_DEV bool bottom_range_step(BE& e, const double* z, const double* cov, double shared_cov, int64_t at, RangeH h) {
  double zz[3] = {0.0, 0.0, 0.0}, R[1] = {1.0};
  if (e.live) {
    zz[0] = z[at];
    R[0] = cov ? cov[at] : shared_cov;
  }
  return e.template update<Z_VECT, 1>(zz, R, h);
}

// measurementNormal (BottomUKF.cpp:32-37)
struct NormalH {
  UWVK_DEV void operator()(const double* x, double* z) const { z[0] = x[1]; z[1] = x[2]; z[2] = x[3]; }
};

// integrateMeasurement(NormalType, cov) (BottomUKF.cpp:63-67): S2 measurement;
// z: this instance's measured normal (normalised here), cov: its 2 x 2
UWVK_DEV bool bottom_normal_step(BE& e, const double z[3], const double cov[4]) {
  double zz[3] = {0.0, 0.0, 1.0}, R[4] = {1.0, 0.0, 0.0, 1.0};
  if (e.live) {
    s2_from(z, zz);
#pragma unroll
    for (int k = 0; k < 4; k++) R[k] = cov[k];
  }
  return e.template update<Z_S2, 2>(zz, R, NormalH{});
}

__global__ __launch_bounds__(BE::BLOCK) void k_bottom_predict(SmallBufs b, const double* vel, M9 Q, double dt) {
  __shared__ double smem[BE::IPB * BE::words];
  int64_t inst;
  BE e = make_engine<BE>(smem, b, nullptr, &inst);
  load(e, b, inst);
  const bool ok = bottom_predict_step(e, vel, inst, Q, dt);
  store(e, b, inst, ok);
}

__global__ __launch_bounds__(BE::BLOCK) void k_bottom_range(SmallBufs b, const double* z, const double* cov,
                                                            double shared_cov, RangeH h, const uint8_t* mask) {
  __shared__ double smem[BE::IPB * BE::words];
  int64_t inst;
  BE e = make_engine<BE>(smem, b, mask, &inst);
  load(e, b, inst);
  const bool ok = bottom_range_step(e, z, cov, shared_cov, inst, h);
  store(e, b, inst, ok);
}

__global__ __launch_bounds__(BE::BLOCK) void k_bottom_normal(SmallBufs b, const double* z, const double* cov,
                                                             M9 shared_cov, const uint8_t* mask) {
  __shared__ double smem[BE::IPB * BE::words];
  int64_t inst;
  BE e = make_engine<BE>(smem, b, mask, &inst);
  load(e, b, inst);
  double zi[3] = {0.0, 0.0, 1.0}, R[4] = {1.0, 0.0, 0.0, 1.0};
  if (e.live) {
#pragma unroll
    for (int k = 0; k < 3; k++) zi[k] = z[inst * 3 + k];
#pragma unroll
    for (int k = 0; k < 4; k++) R[k] = cov ? cov[inst * 4 + k] : shared_cov.v[k];
  }
  const bool ok = bottom_normal_step(e, zi, R);
  store(e, b, inst, ok);
}

// ---- BottomUKF in a run (uwvk_bottom_run_log) -------------------------------
// One launch covers up to kBottomChunk epochs: (mu, Sigma) is loaded once, stays
// in the instance's LDS words across the epochs and is stored once.  The epoch
// table is uniform over the grid, so every instance of a block takes the same
// barrier sequence; what an instance skips (a non-finite payload) is the
// engine's `live` flag of that step, as a masked-out instance of the single
// kernels, never a branch around the step.
constexpr int64_t kBottomChunk = 4096;        // epochs per launch, as uwvk_vel_run_log
constexpr uint32_t kBevRecord = 0x80000000u;  // epoch table only: a track record follows this epoch
struct BottomEpoch {                          // one row of the device epoch table
  uint32_t flags;                             // UWVK_BEV_* | kBevRecord
  int32_t range_row, normal_row, record;      // rows of the payloads, record of this call
};
struct BottomRunArgs {
  const BottomEpoch* ev;   // DEVICE [count], this launch's epochs
  int32_t count, beams;
  const double* velocity;  // this launch's first epoch: [count][batch][3]
  const double* range;     // [n_range][beams][batch]
  const double* range_var; // nullable
  const double* normal;    // [n_normal][batch][3]
  double* vel_io;          // the handle's velocity [batch][3]: read at entry, written at exit
  uint32_t* applied;       // [batch][2], nullable
  double* tr_mean;         // [records][batch][4], nullable
  double* tr_var;          // [records][batch][3], nullable
  double dt, range_cov;
  double normal_cov[4];
  RangeH beam[UWVK_BOTTOM_MAX_BEAMS];
  M9 Q;
};


__global__ __launch_bounds__(BE::BLOCK) void k_bottom_run(SmallBufs b, BottomRunArgs a) {
  __shared__ double smem[BE::IPB * BE::words];
  int64_t inst;
  BE e = make_engine<BE>(smem, b, nullptr, &inst);
  const bool in = e.live;  // instance < batch
  if (!in) {  // the tail of the last block: a valid state, so its (unused) steps converge at once
    for (int i = e.g; i < BE::n * BE::n; i += BE::G) e.sm[BE::o_sig + i] = i % (BE::n + 1) == 0 ? 1.0 : 0.0;
    for (int k = e.g; k < BE::S; k += BE::G) e.sm[BE::o_mu + k] = k == 0 || k == BE::S - 1 ? 1.0 : 0.0;
  }
  load(e, b, inst);
  double v[3] = {0.0, 0.0, 0.0};
  if (in) {
#pragma unroll
    for (int k = 0; k < 3; k++) v[k] = a.vel_io[inst * 3 + k];
  }
  uint32_t st = 0, n_range = 0, n_normal = 0;
  for (int32_t t = 0; t < a.count; t++) {
    const BottomEpoch ev = a.ev[t];
    // setVelocity + predictionStep
    bool live = in;
    if (in) {
      const double* ve = a.velocity + ((int64_t)t * b.batch + inst) * 3;
      const double nv[3] = {ve[0], ve[1], ve[2]};
      if (finite_dev(nv[0]) && finite_dev(nv[1]) && finite_dev(nv[2])) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = nv[k];
      } else {
        live = false;
        st |= UWVK_ST_NAN;
      }
    }
    e.live = live;
    if (!bottom_predict_step(e, v, 0, a.Q, a.dt) && live) st |= UWVK_ST_NOTPD;
    // the updates: Engine::update has already reduced Sigma in LDS when the
    // Cholesky of apply_delta fails (mu is written last), so Sigma is kept in
    // registers over each update (9 words over the group's 8 lanes) and put back
    const int64_t rrow = (int64_t)ev.range_row * a.beams;
    for (int32_t bm = 0; bm < a.beams; bm++) {
      if (!(ev.flags & UWVK_BEV_BEAM(bm))) continue;  // uniform
      live = in;
      const int64_t at = (rrow + bm) * b.batch + inst;
      if (in) {
        const double z = a.range[at], var = a.range_var ? a.range_var[at] : a.range_cov;
        if (!(finite_dev(z) && finite_dev(var))) {
          live = false;
          st |= UWVK_ST_NAN;
        }
      }
      const double keep0 = e.sm[BE::o_sig + e.g], keep8 = e.sm[BE::o_sig + 8];
      e.live = live;
      const bool ok = bottom_range_step(e, a.range, a.range_var, a.range_cov, at, a.beam[bm]);
      if (live && ok) n_range++;
      if (live && !ok) {
        st |= UWVK_ST_NOTPD;
        e.sm[BE::o_sig + e.g] = keep0;
        if (e.g == 0) e.sm[BE::o_sig + 8] = keep8;
      }
      __syncthreads();
    }
    if (ev.flags & UWVK_BEV_NORMAL) {  // uniform
      live = in;
      double zn[3] = {0.0, 0.0, 1.0};
      if (in) {
        const double* ne = a.normal + ((int64_t)ev.normal_row * b.batch + inst) * 3;
        const double nv[3] = {ne[0], ne[1], ne[2]};
        if (finite_dev(nv[0]) && finite_dev(nv[1]) && finite_dev(nv[2]) &&
            nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2] > 0.0) {
#pragma unroll
          for (int k = 0; k < 3; k++) zn[k] = nv[k];
        } else {
          live = false;
          st |= UWVK_ST_NAN;
        }
      }
      const double keep0 = e.sm[BE::o_sig + e.g], keep8 = e.sm[BE::o_sig + 8];
      e.live = live;
      const bool ok = bottom_normal_step(e, zn, a.normal_cov);
      if (live && ok) n_normal++;
      if (live && !ok) {
        st |= UWVK_ST_NOTPD;
        e.sm[BE::o_sig + e.g] = keep0;
        if (e.g == 0) e.sm[BE::o_sig + 8] = keep8;
      }
      __syncthreads();
    }
    // track record, straight from LDS (every step above ends in a barrier)
    if ((ev.flags & kBevRecord) && in) {
      const int64_t at = (int64_t)ev.record * b.batch + inst;
      if (a.tr_mean && e.g < BE::S) a.tr_mean[at * BE::S + e.g] = e.sm[BE::o_mu + e.g];
      if (a.tr_var && e.g < BE::n) a.tr_var[at * BE::n + e.g] = e.sm[BE::o_sig + e.g * BE::n + e.g];
    }
  }
  e.live = in;
  store(e, b, inst, true);
  if (in) {
    if (e.g < 3) a.vel_io[inst * 3 + e.g] = v[e.g];
    if (e.g == 0) {
      if (st) b.status[inst] |= st;
      if (a.applied) {
        a.applied[inst * 2] += n_range;
        a.applied[inst * 2 + 1] += n_normal;
      }
    }
  }
}

// ---- IndirectPoseUKF -------------------------------------------------------
// The step bodies, on an engine whose (mu, Sigma) is in LDS.  The single kernels
// and k_ipose_run both call them, so both compile the same expressions: the
// run's bitwise contract (include/uwvk.h) rests on that, as for BottomUKF.

// predictionStepImpl (IndirectPoseUKF.cpp:80-92) + processModel (:7-20); E is
// the 6-DOF engine at either lane count
template <int SR, class E>
UWVK_DEV bool ipose_predict_step(E& e, const M36& Q, double tau, double dt) {
  // Q' = dt^2 (Q with the orientation block R (2/(tau dt) Q_o) R^T), R = mu's rotation
  double Rm[9];
  {
    const double q[4] = {e.sm[E::o_mu + 3], e.sm[E::o_mu + 4], e.sm[E::o_mu + 5], e.sm[E::o_mu + 6]};
    qmatrix(q, Rm);
  }
  const double s = 2.0 / (tau * dt), dt2 = dt * dt;
  auto qf = [&](int r, int c) {
    if (r < 3 || c < 3) return dt2 * Q.v[r * 6 + c];
    const int i = r - 3, j = c - 3;
    double A[3];
#pragma unroll
    for (int l = 0; l < 3; l++) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) t += Rm[i * 3 + k] * (s * Q.v[(k + 3) * 6 + l + 3]);
      A[l] = t;
    }
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < 3; k++) t += A[k] * Rm[j * 3 + k];
    return dt2 * t;
  };
  const double ntau = -1.0 / tau;
  return e.predict(
      [&](double* x) {
        double l[3], d[3], ex[4], r[4];
        so3_log(x + 3, l);
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = ntau * l[k] * dt;
        so3_exp(d, ex);
        // orientation_error.boxplus(d, dt) (:17); d is a multiple of log(q), so
        // exp(d) commutes with q and both sides give the same product
        if constexpr (SR) qmul(x + 3, ex, r);
        else qmul(ex, x + 3, r);
#pragma unroll
        for (int k = 0; k < 4; k++) x[3 + k] = r[k];
      },
      qf);
}

// integrateMeasurement(marker features, ...) (IndirectPoseUKF.cpp:94-135):
// augment with the marker pose, one S2 update per feature (visual_loop), keep
// the filter block.  This instance's 36 / 7 / 7 words start at sigma[at * 36],
// mu[at * 7] and marker[mat], in HBM (the single kernel) or LDS (the run); they
// are read or written only if `take`.
template <class E>
UWVK_DEV void ipose_augment(E& e, bool take, const double* sigma, const double* mu, int64_t at,
                            const double* cov_marker, const double* marker, int64_t mat) {
  if (take) {
    for (int i = e.g; i < 144; i += E::G) {
      const int r = i / 12, c = i % 12;
      double v = 0.0;
      if (r < 6 && c < 6) v = sigma[at * 36 + r * 6 + c];
      else if (r >= 6 && c >= 6) v = cov_marker[(r - 6) * 6 + (c - 6)];
      e.sm[E::o_sig + i] = v;
    }
    for (int k = e.g; k < 14; k += E::G) e.sm[E::o_mu + k] = k < 7 ? mu[at * 7 + k] : marker[mat + (k - 7)];
  }
  __syncthreads();
}
template <class E>
UWVK_DEV void ipose_extract(E& e, bool take, double* sigma, double* mu, int64_t at) {
  if (take) {
    for (int i = e.g; i < 36; i += E::G) sigma[at * 36 + i] = e.sm[E::o_sig + (i / 6) * 12 + (i % 6)];
    for (int k = e.g; k < 7; k += E::G) mu[at * 7 + k] = e.sm[E::o_mu + k];
  }
}

template <int SR>
__global__ __launch_bounds__(IE<SR>::BLOCK) void k_ipose_predict(SmallBufs b, M36 Q, double tau, double dt) {
  using E = IE<SR>;
  __shared__ double smem[E::IPB * E::words];
  int64_t inst;
  E e = make_engine<E>(smem, b, nullptr, &inst);
  load(e, b, inst);
  const bool ok = ipose_predict_step<SR>(e, Q, tau, dt);
  store(e, b, inst, ok);
}

template <int SR>
__global__ __launch_bounds__(IAE<SR>::BLOCK) void k_ipose_visual(SmallBufs b, VisArgs va) {
  using E = IAE<SR>;
  __shared__ double smem[E::IPB * E::words];
  int64_t inst;
  E e = make_engine<E>(smem, b, va.mask, &inst);
  ipose_augment(e, e.live, b.sigma, b.mu, inst, va.cov_marker, va.marker, inst * va.marker_stride);
  const bool ok = visual_loop<E, 7, true>(e, va, inst);
  ipose_extract(e, e.live && ok, b.sigma, b.mu, inst);
  if (e.live && !ok && e.g == 0) b.status[inst] |= UWVK_ST_NOTPD;
}

// getCorrectedPose (IndirectPoseUKF.cpp:137-142): o = r * e, pose_ref * pose_error,
// each t(3) q(4): t = t_ref + R_ref p_err (Eigen _transformVector), q = q_ref * q_err
__host__ __device__ inline void ipose_corrected(const double* r, const double* e, double* o) {
  const double* q = r + 3;
  double uv[3] = {2 * (q[2] * e[2] - q[3] * e[1]), 2 * (q[3] * e[0] - q[1] * e[2]), 2 * (q[1] * e[1] - q[2] * e[0])};
  double t2[3] = {q[2] * uv[2] - q[3] * uv[1], q[3] * uv[0] - q[1] * uv[2], q[1] * uv[1] - q[2] * uv[0]};
  for (int k = 0; k < 3; k++) o[k] = r[k] + (e[k] + q[0] * uv[k] + t2[k]);
  const double* b = e + 3;
  o[3] = q[0] * b[0] - q[1] * b[1] - q[2] * b[2] - q[3] * b[3];
  o[4] = q[0] * b[1] + q[1] * b[0] + q[2] * b[3] - q[3] * b[2];
  o[5] = q[0] * b[2] + q[2] * b[0] + q[3] * b[1] - q[1] * b[3];
  o[6] = q[0] * b[3] + q[3] * b[0] + q[1] * b[2] - q[2] * b[1];
}

// ---- IndirectPoseUKF in a run (uwvk_ipose_run_log) ---------------------------
// One launch covers up to kIPoseChunk epochs.  A 64-lane block holds two
// instances of 32 lanes, the visual engine's shape; the predict runs on the
// 6-DOF engine widened to the same 32 lanes (its lanes >= 13 idle).  The home of
// (mu, Sigma 6x6) is the 6-DOF engine's LDS words: loaded once, stored once.  A
// visual row copies it into the augmented engine's own words and copies the
// filter block back only if every feature's update succeeded, so a failed row
// leaves the home untouched.  The pose reference is not copied: each instance
// keeps a pointer to its last finite one (a row of the log, or the handle's),
// which visual_loop reads as the single kernel does, and stores it at exit.
// Barriers are uniform as in k_bottom_run: the epoch table is uniform over the
// grid and a skip is the engine's `live` flag of that step.
constexpr int64_t kIPoseChunk = kBottomChunk;
template <int SR>
using IE32 = Engine<IPoseM<SR>, IAE<SR>::G>;
struct IPoseEpoch {  // one row of the device epoch table
  double dt;
  int64_t row;       // first visual row of this epoch
  int32_t rows;      // visual rows of this epoch
  int32_t record;    // track record of this call after this epoch, -1: none
};
struct IPoseRunArgs {
  const IPoseEpoch* ev;     // DEVICE [count], this launch's epochs
  int32_t count;
  const double* pose_ref;   // this launch's first epoch: [count][batch][7], nullable
  double* ref_io;           // the handle's pose_ref [batch][7]: read at entry, written at exit
  const double* marker_rows;// DEVICE shared marker poses [rows of this call][7], or NULL (per instance)
  int64_t row_base;         // the visual row that marker_rows starts at
  uint32_t* applied;        // [batch], nullable
  double* tr_mean;          // [records][batch][7], nullable
  double* tr_var;           // [records][batch][6], nullable
  double* tr_corr;          // [records][batch][7], nullable
  double tau;
  M36 Q;
  VisArgs va;               // features, fcov, marker: row 0 of the log's arrays; ref, mask unused
};

// true in every lane of a 32-lane group if `bad` is in any of them
UWVK_DEV bool group32_any(bool bad) { return (uint32_t)(__ballot(bad) >> (threadIdx.x & 32)) != 0u; }

template <int SR>
__global__ __launch_bounds__(IAE<SR>::BLOCK) void k_ipose_run(SmallBufs b, IPoseRunArgs a) {
  using EP = IE32<SR>;
  using EV = IAE<SR>;
  static_assert(EP::G == EV::G && EP::IPB == EV::IPB && EP::BLOCK == EV::BLOCK, "one lane group for both engines");
  constexpr int kWords = EP::words + EV::words;
  __shared__ double smem[EV::IPB * kWords];
  const int gi = threadIdx.x / EV::G, g = threadIdx.x % EV::G;
  const int64_t inst = (int64_t)blockIdx.x * EV::IPB + gi;
  const bool in = inst < b.batch;
  EP ep;
  EV ev;
  ep.g = ev.g = g;
  ep.sm = smem + gi * kWords;
  ev.sm = ep.sm + EP::words;
  double* const sig = ep.sm + EP::o_sig;  // the home of (mu, Sigma)
  double* const mu = ep.sm + EP::o_mu;
  if (!in) {  // the empty slot of the last block: valid states, so its (unused) steps converge at once
    for (int i = g; i < 36; i += EP::G) sig[i] = i % 7 == 0 ? 1.0 : 0.0;
    for (int k = g; k < 7; k += EP::G) mu[k] = k == 3 ? 1.0 : 0.0;
    for (int i = g; i < 144; i += EV::G) ev.sm[EV::o_sig + i] = i % 13 == 0 ? 1.0 : 0.0;
    for (int k = g; k < 14; k += EV::G) ev.sm[EV::o_mu + k] = k == 3 || k == 10 ? 1.0 : 0.0;
  }
  ep.live = in;
  load(ep, b, inst);
  const double* ref = a.ref_io + inst * 7;  // dereferenced only if `in`
  const double* const ref_in = ref;
  uint32_t st = 0, n_applied = 0;
  for (int32_t t = 0; t < a.count; t++) {
    const IPoseEpoch epoch = a.ev[t];
    // updatePoseReference: a non-finite one leaves the instance on its last finite reference
    if (a.pose_ref) {  // uniform
      const double* cand = a.pose_ref + ((int64_t)t * b.batch + inst) * 7;
      const bool bad = group32_any(in && g < 7 && !finite_dev(cand[g]));
      if (in && !bad) ref = cand;
      if (bad) st |= UWVK_ST_NAN;
    }
    // predictionStep; it does not read the reference
    ep.live = in;
    if (!ipose_predict_step<SR>(ep, a.Q, a.tau, epoch.dt) && in) st |= UWVK_ST_NOTPD;
    // the marker observations of this epoch, in row order
    for (int32_t r = 0; r < epoch.rows; r++) {  // uniform
      const int64_t row = epoch.row + r;
      VisArgs vr = a.va;
      vr.features = a.va.features + row * b.batch * vr.nf * 2;
      if (vr.fcov_stride) vr.fcov = a.va.fcov + row * b.batch * vr.fcov_stride;
      vr.marker = vr.marker_stride ? a.va.marker + row * b.batch * 7 : a.marker_rows + (row - a.row_base) * 7;
      vr.ref = ref - inst * 7;  // visual_loop reads ref[inst * 7 + k]
      bool bad = false;
      if (in) {  // what the single call refuses on the host (stage_visual), per instance
        const double* f = vr.features + inst * vr.nf * 2;
        for (int i = g; i < vr.nf * 2; i += EV::G) bad |= !finite_dev(f[i]);
        if (vr.fcov_stride) {
          const double* c = vr.fcov + inst * vr.fcov_stride;
          for (int i = g; i < vr.nf * 4; i += EV::G) bad |= !finite_dev(c[i]);
        }
        if (vr.marker_stride && g < 7) bad |= !finite_dev(vr.marker[inst * 7 + g]);
      }
      bad = group32_any(bad);
      if (bad) st |= UWVK_ST_NAN;
      ev.live = in && !bad;
      ipose_augment(ev, in, sig, mu, 0, a.va.cov_marker, vr.marker, inst * vr.marker_stride);
      const bool ok = visual_loop<EV, 7, true>(ev, vr, inst);
      ipose_extract(ev, ev.live && ok, sig, mu, 0);
      if (ev.live && ok) n_applied++;
      if (ev.live && !ok) st |= UWVK_ST_NOTPD;
      __syncthreads();
    }
    // track record, straight from LDS (every step above ends in a barrier)
    if (epoch.record >= 0 && in) {
      const int64_t at = (int64_t)epoch.record * b.batch + inst;
      if (a.tr_mean && g < 7) a.tr_mean[at * 7 + g] = mu[g];
      if (a.tr_var && g < 6) a.tr_var[at * 6 + g] = sig[g * 6 + g];
      if (a.tr_corr && g == 7) {
        double rr[7], ee[7], oo[7];
#pragma unroll
        for (int k = 0; k < 7; k++) {
          rr[k] = ref[k];
          ee[k] = mu[k];
        }
        ipose_corrected(rr, ee, oo);
#pragma unroll
        for (int k = 0; k < 7; k++) a.tr_corr[at * 7 + k] = oo[k];
      }
    }
  }
  ep.live = in;
  store(ep, b, inst, true);
  if (in) {
    if (ref != ref_in && g < 7) a.ref_io[inst * 7 + g] = ref[g];
    if (g == 0) {
      if (st) b.status[inst] |= st;
      if (a.applied) a.applied[inst] += n_applied;
    }
  }
}

int64_t grid_of(int64_t batch, int ipb) { return (batch + ipb - 1) / ipb; }

}  // namespace

// ===========================================================================
// host handles
// ===========================================================================
struct SmallHandle {
  int64_t batch = 0;
  int device = 0, n = 0, store = 0;
  hipStream_t stream = nullptr;
  double *d_mu = nullptr, *d_sigma = nullptr, *d_aux = nullptr, *d_meas = nullptr;
  uint32_t* d_status = nullptr;
  uint8_t* d_mask = nullptr;
  size_t meas_words = 0;
  VisStage vis;  // visual-update staging (IndirectPoseUKF)
  bool has_state = false;
  SmallBufs bufs() const { return SmallBufs{batch, d_mu, d_sigma, d_status}; }
};

// StageSlot, stage_acquire, StageDone, stage_release: the host arrays of one run call
// (uwvk_stage.hpp); VisualRows: the checks and the staging of the visual rows
// (uwvk_visual_rows.hpp)

struct uwvk_bottom : SmallHandle {
  M9 Q{};
  std::vector<StageSlot> stages;
};

struct uwvk_ipose : SmallHandle {
  M36 Q{};
  double tau = 1.0;
  int so3_right = 1;  // UWVK_OPT_SO3_RIGHT (uwvk_ipose_set_option), default body frame
  std::vector<StageSlot> stages;
};

static void small_destroy(SmallHandle* h) {
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->d_mu, (void*)h->d_sigma, (void*)h->d_aux, (void*)h->d_meas, (void*)h->d_status,
                  (void*)h->d_mask})
    if (p) (void)hipFree(p);
  h->vis.release();
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

// aux: BottomUKF velocity [batch][3]; IndirectPoseUKF pose_ref [batch][7]
static uwvk_status small_create(SmallHandle* h, int64_t batch, int device, int n, int store, int aux_w,
                                size_t meas_words) {
  h->batch = batch;
  h->device = device;
  h->n = n;
  h->store = store;
  h->meas_words = meas_words;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess)
    return UWVK_EDEVICE;
  const size_t B = (size_t)batch;
  const bool ok = hipMalloc(&h->d_mu, B * store * 8) == hipSuccess &&
                  hipMalloc(&h->d_sigma, B * n * n * 8) == hipSuccess &&
                  hipMalloc(&h->d_aux, B * aux_w * 8) == hipSuccess &&
                  hipMalloc(&h->d_meas, meas_words * 8) == hipSuccess && hipMalloc(&h->d_mask, B) == hipSuccess &&
                  hipMalloc(&h->d_status, B * 4) == hipSuccess;
  if (!ok) return UWVK_ENOMEM;
  (void)hipMemsetAsync(h->d_aux, 0, B * aux_w * 8, h->stream);
  (void)hipMemsetAsync(h->d_status, 0, B * 4, h->stream);
  return hipStreamSynchronize(h->stream) == hipSuccess ? UWVK_OK : UWVK_EDEVICE;
}

static uwvk_status small_get_state(SmallHandle* h, double* x, double* P) {
  if (!h || !x) return UWVK_EINVAL;
  HIPCHK(hipMemcpyAsync(x, h->d_mu, (size_t)h->batch * h->store * 8, hipMemcpyDeviceToHost, h->stream));
  if (P) HIPCHK(hipMemcpyAsync(P, h->d_sigma, (size_t)h->batch * h->n * h->n * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

static uwvk_status small_get_status(SmallHandle* h, uint32_t* st, int clear) {
  if (!h || !st) return UWVK_EINVAL;
  HIPCHK(hipMemcpyAsync(st, h->d_status, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
  if (clear) HIPCHK(hipMemsetAsync(h->d_status, 0, (size_t)h->batch * 4, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

static uwvk_status upload_mask(SmallHandle* h, const uint8_t* mask, const uint8_t** dmask) {
  *dmask = nullptr;
  if (mask) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)h->batch, hipMemcpyHostToDevice, h->stream));
    *dmask = h->d_mask;
  }
  return UWVK_OK;
}

extern "C" {

// ---- BottomUKF -----------------------------------------------------------
uwvk_status uwvk_bottom_create(int64_t batch, int device, uwvk_bottom** out) {
  ::uwvk::DeviceGuard uwvk_device_guard_(device);
  if (!out || batch <= 0) return UWVK_EINVAL;
  *out = nullptr;
  if (!uwvk_device_available(device)) return UWVK_EDEVICE;
  uwvk_bottom* h = new uwvk_bottom();
  const uwvk_status st = small_create(h, batch, device, 3, 4, 3, (size_t)batch * 8 + 16);
  if (st != UWVK_OK) {
    small_destroy(h);
    delete h;
    return st;
  }
  for (int k = 0; k < 3; k++) h->Q.v[k * 3 + k] = 1.0;  // Covariance::Identity() (BottomUKF.cpp:45)
  *out = h;
  return UWVK_OK;
}

void uwvk_bottom_destroy(uwvk_bottom* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return;
  small_destroy(h);  // waits for the stream first
  stage_release(h->stages);
  delete h;
}

void* uwvk_bottom_stream(const uwvk_bottom* h) { return h ? (void*)h->stream : nullptr; }

uwvk_status uwvk_bottom_init(uwvk_bottom* h, const double* x, const double* P) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !x || !P) return UWVK_EINVAL;
  const int64_t B = h->batch;
  if (!finite_all(x, (size_t)B * 4) || !finite_all(P, (size_t)B * 9)) return UWVK_ENAN;
  std::vector<double> xs((size_t)B * 4);
  for (int64_t i = 0; i < B; i++) {  // MTK::S2 constructor normalises the normal
    const double* v = x + i * 4;
    const double nn = std::sqrt(v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
    if (!(nn > 0.0)) return UWVK_EINVAL;
    xs[i * 4] = v[0];
    for (int k = 1; k < 4; k++) xs[i * 4 + k] = v[k] / nn;
  }
  HIPCHK(hipMemcpyAsync(h->d_mu, xs.data(), xs.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_sigma, P, (size_t)B * 9 * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->has_state = true;
  return UWVK_OK;
}

uwvk_status uwvk_bottom_set_process_noise(uwvk_bottom* h, const double Q[9]) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !Q) return UWVK_EINVAL;
  if (!finite_all(Q, 9)) return UWVK_ENAN;
  std::memcpy(h->Q.v, Q, sizeof(h->Q.v));
  return UWVK_OK;
}

uwvk_status uwvk_bottom_set_velocity(uwvk_bottom* h, const double* v) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !v) return UWVK_EINVAL;
  if (!finite_all(v, (size_t)h->batch * 3)) return UWVK_ENAN;
  HIPCHK(hipMemcpyAsync(h->d_aux, v, (size_t)h->batch * 3 * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_bottom_predict(uwvk_bottom* h, double dt) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  hipLaunchKernelGGL(k_bottom_predict, dim3(grid_of(h->batch, BE::IPB)), dim3(BE::BLOCK), 0, h->stream, h->bufs(),
                     h->d_aux, h->Q, dt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_bottom_update_range(uwvk_bottom* h, const double* mu, const double* cov, double shared_cov,
                                     const double unit_direction[3], const double origin[3], const uint8_t* mask) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !mu || !unit_direction || !origin) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  const int64_t B = h->batch;
  for (int64_t i = 0; i < B; i++) {  // checkMeasurment (BottomUKF.cpp:58)
    if (mask && !mask[i]) continue;
    if (!std::isfinite(mu[i]) || (cov && !std::isfinite(cov[i]))) return UWVK_ENAN;
  }
  if (!cov && !std::isfinite(shared_cov)) return UWVK_ENAN;
  double* dz = h->d_meas;
  double* dc = h->d_meas + B;
  HIPCHK(hipMemcpyAsync(dz, mu, (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
  if (cov) HIPCHK(hipMemcpyAsync(dc, cov, (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
  const uint8_t* dm;
  if (upload_mask(h, mask, &dm) != UWVK_OK) return UWVK_EDEVICE;
  RangeH rh;
  for (int k = 0; k < 3; k++) {
    rh.dir[k] = unit_direction[k];
    rh.origin[k] = origin[k];
  }
  hipLaunchKernelGGL(k_bottom_range, dim3(grid_of(B, BE::IPB)), dim3(BE::BLOCK), 0, h->stream, h->bufs(), dz,
                     cov ? dc : nullptr, shared_cov, rh, dm);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_bottom_update_normal(uwvk_bottom* h, const double* mu, const double* cov, const double* shared_cov,
                                      const uint8_t* mask) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !mu || (!cov && !shared_cov)) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  const int64_t B = h->batch;
  // the reference does not check this measurement (BottomUKF.cpp:63-67); here a
  // non-finite mean or covariance of a masked-in instance is UWVK_ENAN like every
  // other measurement, and a zero normal cannot be normalised into S2
  for (int64_t i = 0; i < B; i++) {
    if (mask && !mask[i]) continue;
    const double* v = mu + i * 3;
    if (!finite_all(v, 3) || (cov && !finite_all(cov + i * 4, 4))) return UWVK_ENAN;
    if (!(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] > 0.0)) return UWVK_EINVAL;
  }
  if (!cov && !finite_all(shared_cov, 4)) return UWVK_ENAN;
  double* dz = h->d_meas;
  double* dc = h->d_meas + B * 3;
  HIPCHK(hipMemcpyAsync(dz, mu, (size_t)B * 3 * 8, hipMemcpyHostToDevice, h->stream));
  if (cov) HIPCHK(hipMemcpyAsync(dc, cov, (size_t)B * 4 * 8, hipMemcpyHostToDevice, h->stream));
  M9 sc{};
  if (!cov) std::memcpy(sc.v, shared_cov, 4 * 8);
  const uint8_t* dm;
  if (upload_mask(h, mask, &dm) != UWVK_OK) return UWVK_EDEVICE;
  hipLaunchKernelGGL(k_bottom_normal, dim3(grid_of(B, BE::IPB)), dim3(BE::BLOCK), 0, h->stream, h->bufs(), dz,
                     cov ? dc : nullptr, sc, dm);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

// host only (no HIP call): what uwvk_bottom_run_log checks before it queues anything
uwvk_status uwvk_bottom_log_check(const uwvk_bottom_log* log, int64_t first, int64_t count) {
  if (!log || first < 0 || count < 0 || first > log->epochs || count > log->epochs - first) return UWVK_EINVAL;
  if (!(log->dt > 0.0)) return UWVK_EINVAL;
  if (log->beams < 0 || log->beams > UWVK_BOTTOM_MAX_BEAMS) return UWVK_EINVAL;
  if (count > 0 && (!log->flags || !log->velocity)) return UWVK_EINVAL;
  const uint32_t beam_bits = (1u << log->beams) - 1u;
  uint32_t used = 0;
  for (int64_t e = first; e < first + count; e++) {
    const uint32_t f = log->flags[e];
    if (f & ~(beam_bits | UWVK_BEV_NORMAL)) return UWVK_EINVAL;
    if (f & beam_bits) {
      if (!log->range_index || !log->range) return UWVK_EINVAL;
      if (log->range_index[e] < 0 || log->range_index[e] >= log->n_range) return UWVK_EINVAL;
    }
    if (f & UWVK_BEV_NORMAL) {
      if (!log->normal_index || !log->normal) return UWVK_EINVAL;
      if (log->normal_index[e] < 0 || log->normal_index[e] >= log->n_normal) return UWVK_EINVAL;
    }
    used |= f;
  }
  // the shared host values the flagged epochs use (checkMeasurment of the single calls)
  if ((used & beam_bits) && !log->range_var && !std::isfinite(log->range_cov)) return UWVK_ENAN;
  for (int b = 0; b < log->beams; b++)
    if ((used & UWVK_BEV_BEAM(b)) && (!finite_all(log->beam_direction[b], 3) || !finite_all(log->beam_origin[b], 3)))
      return UWVK_ENAN;
  if ((used & UWVK_BEV_NORMAL) && !finite_all(log->normal_cov, 4)) return UWVK_ENAN;
  return UWVK_OK;
}

uwvk_status uwvk_bottom_run_log(uwvk_bottom* h, const uwvk_bottom_log* log, int64_t first, int64_t count,
                                uint32_t* applied, const uwvk_bottom_track* track) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  const uwvk_status chk = uwvk_bottom_log_check(log, first, count);
  if (chk != UWVK_OK) return chk;
  if (track && !track_args_valid(track->every, track->capacity, track->mean || track->variance, first, count))
    return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  if (count == 0) return UWVK_OK;
  StageSlot* sg = stage_acquire(h->stages, (size_t)count * sizeof(BottomEpoch));
  if (!sg) return UWVK_ENOMEM;
  const StageDone stage_done{sg, h->stream};
  BottomEpoch* const table = (BottomEpoch*)sg->host;
  const uint32_t beam_bits = (1u << log->beams) - 1u;
  int32_t record = 0;
  for (int64_t k = 0; k < count; k++) {
    const int64_t e = first + k;
    BottomEpoch& ev = table[k];
    ev.flags = log->flags[e];
    ev.range_row = (ev.flags & beam_bits) ? log->range_index[e] : 0;
    ev.normal_row = (ev.flags & UWVK_BEV_NORMAL) ? log->normal_index[e] : 0;
    ev.record = 0;
    if (track && (e + 1) % track->every == 0) {
      ev.flags |= kBevRecord;
      ev.record = record++;
    }
  }
  HIPCHK(hipMemcpyAsync(sg->dev, sg->host, (size_t)count * sizeof(BottomEpoch), hipMemcpyHostToDevice, h->stream));
  sg->used = true;
  BottomRunArgs a{};
  a.beams = log->beams;
  a.range = log->range;
  a.range_var = log->range_var;
  a.normal = log->normal;
  a.vel_io = h->d_aux;
  a.applied = applied;
  a.tr_mean = track ? track->mean : nullptr;
  a.tr_var = track ? track->variance : nullptr;
  a.dt = log->dt;
  a.range_cov = log->range_cov;
  std::memcpy(a.normal_cov, log->normal_cov, sizeof(a.normal_cov));
  for (int b = 0; b < log->beams; b++)
    for (int k = 0; k < 3; k++) {
      a.beam[b].dir[k] = log->beam_direction[b][k];
      a.beam[b].origin[k] = log->beam_origin[b][k];
    }
  a.Q = h->Q;
  // one launch per chunk of epochs; the state's round trip through HBM is exact
  uwvk_status st = UWVK_OK;
  for (int64_t k = 0; k < count && st == UWVK_OK; k += kBottomChunk) {
    a.ev = (const BottomEpoch*)sg->dev + k;
    a.count = (int32_t)std::min<int64_t>(kBottomChunk, count - k);
    a.velocity = log->velocity + (first + k) * h->batch * 3;
    hipLaunchKernelGGL(k_bottom_run, dim3(grid_of(h->batch, BE::IPB)), dim3(BE::BLOCK), 0, h->stream, h->bufs(), a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) st = (uwvk_status)::uwvk::edevice_status(le, "k_bottom_run");
  }
  return st;
}

uwvk_status uwvk_bottom_synchronize(uwvk_bottom* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_bottom_get_state(uwvk_bottom* h, double* x, double* P) { UWVK_DEVICE_GUARD(h); return small_get_state(h, x, P); }
uwvk_status uwvk_bottom_get_status(uwvk_bottom* h, uint32_t* status, int clear) {
  UWVK_DEVICE_GUARD(h);
  return small_get_status(h, status, clear);
}

// ---- IndirectPoseUKF -------------------------------------------------------
uwvk_status uwvk_ipose_create(int64_t batch, int device, uwvk_ipose** out) {
  ::uwvk::DeviceGuard uwvk_device_guard_(device);
  if (!out || batch <= 0) return UWVK_EINVAL;
  *out = nullptr;
  if (!uwvk_device_available(device)) return UWVK_EDEVICE;
  uwvk_ipose* h = new uwvk_ipose();
  const uwvk_status st = small_create(h, batch, device, 6, 7, 7, 0);
  if (st != UWVK_OK) {
    small_destroy(h);
    delete h;
    return st;
  }
  std::vector<double> ref((size_t)batch * 7, 0.0);  // Affine3d::Identity() (IndirectPoseUKF.cpp:58)
  for (int64_t i = 0; i < batch; i++) ref[i * 7 + 3] = 1.0;
  if (hipMemcpy(h->d_aux, ref.data(), ref.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
    small_destroy(h);
    delete h;
    return UWVK_EDEVICE;
  }
  *out = h;
  return UWVK_OK;
}

void uwvk_ipose_destroy(uwvk_ipose* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return;
  small_destroy(h);  // waits for the stream first
  stage_release(h->stages);
  delete h;
}

void* uwvk_ipose_stream(const uwvk_ipose* h) { return h ? (void*)h->stream : nullptr; }

uwvk_status uwvk_ipose_set_option(uwvk_ipose* h, int option, int value) {
  if (!h) return UWVK_EINVAL;
  if (option == UWVK_OPT_SO3_RIGHT) {
    h->so3_right = value ? 1 : 0;
    return UWVK_OK;
  }
  return UWVK_EINVAL;
}

uwvk_status uwvk_ipose_init(uwvk_ipose* h, const double position_error_std[3], const double orientation_error_std[3],
                            double orientation_error_tau, const double* initial_position_error,
                            const double initial_position_error_std[3]) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !position_error_std || !orientation_error_std) return UWVK_EINVAL;
  if (!(orientation_error_tau > 0.0)) return UWVK_EINVAL;
  const int64_t B = h->batch;
  std::vector<double> x((size_t)B * 7, 0.0), P((size_t)B * 36, 0.0);
  double Q[36] = {0};
  for (int k = 0; k < 3; k++) {
    const double s0 = initial_position_error_std ? initial_position_error_std[k] : 1.0;
    for (int64_t i = 0; i < B; i++) {
      P[i * 36 + k * 6 + k] = std::fabs(s0) * std::fabs(s0);
      P[i * 36 + (k + 3) * 6 + k + 3] = std::fabs(orientation_error_std[k]) * std::fabs(orientation_error_std[k]);
    }
    Q[k * 6 + k] = std::fabs(position_error_std[k]) * std::fabs(position_error_std[k]);
    Q[(k + 3) * 6 + k + 3] = std::fabs(orientation_error_std[k]) * std::fabs(orientation_error_std[k]);
  }
  for (int64_t i = 0; i < B; i++) {
    for (int k = 0; k < 3; k++) x[i * 7 + k] = initial_position_error ? initial_position_error[i * 3 + k] : 0.0;
    x[i * 7 + 3] = 1.0;
  }
  if (!finite_all(x.data(), x.size()) || !finite_all(P.data(), P.size()) || !finite_all(Q, 36)) return UWVK_ENAN;
  std::memcpy(h->Q.v, Q, sizeof(Q));
  h->tau = orientation_error_tau;
  HIPCHK(hipMemcpyAsync(h->d_mu, x.data(), x.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_sigma, P.data(), P.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->has_state = true;
  return UWVK_OK;
}

uwvk_status uwvk_ipose_set_process_noise(uwvk_ipose* h, const double Q[36]) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !Q) return UWVK_EINVAL;
  if (!finite_all(Q, 36)) return UWVK_ENAN;
  std::memcpy(h->Q.v, Q, sizeof(h->Q.v));
  return UWVK_OK;
}

uwvk_status uwvk_ipose_set_pose_reference(uwvk_ipose* h, const double* pose) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !pose) return UWVK_EINVAL;
  if (!finite_all(pose, (size_t)h->batch * 7)) return UWVK_ENAN;
  HIPCHK(hipMemcpyAsync(h->d_aux, pose, (size_t)h->batch * 7 * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_ipose_predict(uwvk_ipose* h, double dt) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !(dt > 0.0)) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  if (h->so3_right)
    hipLaunchKernelGGL(k_ipose_predict<1>, dim3(grid_of(h->batch, IE<1>::IPB)), dim3(IE<1>::BLOCK), 0, h->stream,
                       h->bufs(), h->Q, h->tau, dt);
  else
    hipLaunchKernelGGL(k_ipose_predict<0>, dim3(grid_of(h->batch, IE<0>::IPB)), dim3(IE<0>::BLOCK), 0, h->stream,
                       h->bufs(), h->Q, h->tau, dt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_ipose_update_visual(uwvk_ipose* h, int32_t n_features, const double* features,
                                     const double* feature_cov, int feature_cov_per_instance,
                                     const double* feature_positions, const double* marker_pose,
                                     int marker_pose_per_instance, const double cov_marker_pose[36],
                                     const double camera[4], const double camera_in_body[7], const uint8_t* mask) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  VisArgs va{};
  const int st = stage_visual(h->stream, h->batch, n_features, features, feature_cov, feature_cov_per_instance,
                              feature_positions, marker_pose, marker_pose_per_instance, cov_marker_pose, camera,
                              camera_in_body, mask, &va, &h->vis);
  if (st != 0 || va.nf == 0) {
    (void)hipStreamSynchronize(h->stream);
    return (uwvk_status)st;
  }
  va.ref = h->d_aux;
  if (h->so3_right)
    hipLaunchKernelGGL(k_ipose_visual<1>, dim3(grid_of(h->batch, IAE<1>::IPB)), dim3(IAE<1>::BLOCK), 0, h->stream,
                       h->bufs(), va);
  else
    hipLaunchKernelGGL(k_ipose_visual<0>, dim3(grid_of(h->batch, IAE<0>::IPB)), dim3(IAE<0>::BLOCK), 0, h->stream,
                       h->bufs(), va);
  const hipError_t e = hipGetLastError();
  return (uwvk_status)::uwvk::launch_sync_status(e, h->stream, "k_ipose_visual");
}

// getCorrectedPose (IndirectPoseUKF.cpp:137-142): pose_ref * pose_error, t(3) q(4)
uwvk_status uwvk_ipose_get_corrected_pose(uwvk_ipose* h, double* out) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !out) return UWVK_EINVAL;
  const int64_t B = h->batch;
  std::vector<double> x((size_t)B * 7), ref((size_t)B * 7);
  HIPCHK(hipMemcpyAsync(x.data(), h->d_mu, x.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(ref.data(), h->d_aux, ref.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < B; i++) ipose_corrected(&ref[i * 7], &x[i * 7], out + i * 7);
  return UWVK_OK;
}

// host only (no HIP call): what uwvk_ipose_run_log checks before it queues anything
uwvk_status uwvk_ipose_log_check(const uwvk_ipose_log* log, int64_t first, int64_t count) {
  if (!log || first < 0 || count < 0 || first > log->epochs || count > log->epochs - first) return UWVK_EINVAL;
  if (log->n_visual < 0 || (!log->visual_offset && log->n_visual != 0)) return UWVK_EINVAL;
  if (log->dt_epoch) {
    for (int64_t e = first; e < first + count; e++)
      if (!(log->dt_epoch[e] > 0.0)) return UWVK_EINVAL;
  } else if (!(log->dt > 0.0)) {
    return UWVK_EINVAL;
  }
  const VisualRows vr(*log);
  int64_t row0, row1;
  if (!visual_rows_valid(vr, first, count, &row0, &row1)) return UWVK_EINVAL;
  // the shared host values the range uses (checkMeasurment of the single calls)
  if (log->dt_epoch) {
    if (!finite_all(log->dt_epoch + first, (size_t)count)) return UWVK_ENAN;
  } else if (!std::isfinite(log->dt)) {
    return UWVK_ENAN;
  }
  if (row1 > row0 && !visual_rows_finite(vr, row0, row1)) return UWVK_ENAN;
  return UWVK_OK;
}

uwvk_status uwvk_ipose_run_log(uwvk_ipose* h, const uwvk_ipose_log* log, int64_t first, int64_t count,
                               uint32_t* applied, const uwvk_ipose_track* track) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  const uwvk_status chk = uwvk_ipose_log_check(log, first, count);
  if (chk != UWVK_OK) return chk;
  if (track && !track_args_valid(track->every, track->capacity, track->mean || track->variance || track->corrected,
                                 first, count))
    return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  if (count == 0) return UWVK_OK;
  const VisualRows vr(*log);
  const int64_t row0 = log->visual_offset ? log->visual_offset[first] : 0;
  const int64_t rows = log->visual_offset ? log->visual_offset[first + count] - row0 : 0;
  // the staged words: the rows' shared visual inputs (visual_rows_stage), then the epoch table
  StageSlot* sg = stage_acquire(h->stages, visual_rows_words(vr, rows) * 8 + (size_t)count * sizeof(IPoseEpoch));
  if (!sg) return UWVK_ENOMEM;
  const StageDone stage_done{sg, h->stream};
  double* hw = (double*)sg->host;
  const double* dw = (const double*)sg->dev;
  IPoseRunArgs a{};
  const size_t w_all = visual_rows_stage(vr, row0, rows, hw, dw, &a.va, &a.marker_rows);
  IPoseEpoch* het = (IPoseEpoch*)(hw + w_all);
  int32_t record = 0;
  for (int64_t k = 0; k < count; k++) {
    const int64_t e = first + k;
    IPoseEpoch& ev = het[k];
    ev.dt = log->dt_epoch ? log->dt_epoch[e] : log->dt;
    ev.row = log->visual_offset ? log->visual_offset[e] : 0;
    ev.rows = log->visual_offset ? (int32_t)(log->visual_offset[e + 1] - log->visual_offset[e]) : 0;
    ev.record = (track && (e + 1) % track->every == 0) ? record++ : -1;
  }
  HIPCHK(hipMemcpyAsync(sg->dev, sg->host, w_all * 8 + (size_t)count * sizeof(IPoseEpoch), hipMemcpyHostToDevice,
                        h->stream));
  sg->used = true;
  a.ref_io = h->d_aux;
  a.row_base = row0;
  a.applied = applied;
  a.tr_mean = track ? track->mean : nullptr;
  a.tr_var = track ? track->variance : nullptr;
  a.tr_corr = track ? track->corrected : nullptr;
  a.tau = h->tau;
  a.Q = h->Q;
  // one launch per chunk of epochs; the state's round trip through HBM is exact
  uwvk_status st = UWVK_OK;
  const dim3 grid(grid_of(h->batch, IAE<1>::IPB)), block(IAE<1>::BLOCK);
  for (int64_t k = 0; k < count && st == UWVK_OK; k += kIPoseChunk) {
    a.ev = (const IPoseEpoch*)(dw + w_all) + k;
    a.count = (int32_t)std::min<int64_t>(kIPoseChunk, count - k);
    a.pose_ref = log->pose_ref ? log->pose_ref + (first + k) * h->batch * 7 : nullptr;
    if (h->so3_right) hipLaunchKernelGGL(k_ipose_run<1>, grid, block, 0, h->stream, h->bufs(), a);
    else hipLaunchKernelGGL(k_ipose_run<0>, grid, block, 0, h->stream, h->bufs(), a);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) st = (uwvk_status)::uwvk::edevice_status(le, "k_ipose_run");
  }
  return st;
}

uwvk_status uwvk_ipose_synchronize(uwvk_ipose* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_ipose_get_state(uwvk_ipose* h, double* x, double* P) { UWVK_DEVICE_GUARD(h); return small_get_state(h, x, P); }
uwvk_status uwvk_ipose_get_status(uwvk_ipose* h, uint32_t* status, int clear) {
  UWVK_DEVICE_GUARD(h);
  return small_get_status(h, status, clear);
}

}  // extern "C"
