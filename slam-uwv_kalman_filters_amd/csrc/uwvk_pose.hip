// uwvk_pose.hip — the uwvk_pose_* C ABI: the handle, its buffers, the copies
// and the launches.  No kernels here: they are instantiated in the
// uwvk_pose_k_*.hip and uwvk_psp_*.hip translation units (launchers in
// uwvk_pose_kernels.hpp / uwvk_psp.hpp).  What a uwvk_pose_run_log* call
// launches, and in which order, is one list made by the pure host planner
// (plan_run, uwvk_plan.hpp); run_log checks the arguments, walks that list and
// has one case per launch kind.
#include "uwvk_pose_kernels.hpp"
#include "uwvk_psp.hpp"
#include "uwvk_plan.hpp"
#include "uwvk_track.hpp"
#include "uwvk_host.hpp"
#include "uwvk_aug_dev.hpp"
#include "uwvk_stage.hpp"
#include "uwvk_visual_rows.hpp"

namespace uwvk {
hipError_t launch_pose_visual(int dof, int right, hipStream_t st, const PoseBufs& b, const aug::VisArgs& va);
hipError_t launch_pose_visual_run(int dof, int right, hipStream_t st, const PoseBufs& b, const aug::VisRunArgs& a);
}

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

using namespace uwvk;


// ===========================================================================
// host side
// ===========================================================================
// ensemble statistics per instance group: 3 store + 1 doubles (store <= 54)
constexpr int64_t kStatsMaxOut = 3 * 54 + 2;

struct uwvk_pose {
  int64_t batch = 0;
  int dof = 53, store = 54, device = 0;
  hipStream_t stream = nullptr;
  double *d_mu = nullptr, *d_sigma = nullptr, *d_Q = nullptr, *d_rot = nullptr, *d_off = nullptr,
         *d_model = nullptr, *d_uwv = nullptr;
  uint32_t* d_status = nullptr;
  double* d_meas = nullptr;  // staging: batch*36 (mu) + batch*36 (cov) + batch*2 (extra)
  uint8_t* d_mask = nullptr;
  uint8_t* d_accepted = nullptr;
  double* d_scratch = nullptr;  // [0, 256): stats out + truth; [0, 3 batch): rotation rate; then stats partials
  PoseShared* d_shared = nullptr;  // device copy of sh for the PSP kernels
  PoseShared sh_dev{};             // what d_shared holds (valid when sh_dev_ok)
  bool sh_dev_ok = false;
  double* d_Qp = nullptr;          // {A_ii A_jj, dt^2 Q_ij} per packed entry (PSP)
  double* d_qband = nullptr;       // [128] dt^2 Q band of rows >= 9 (PSP)
  double qp_dt = -1.0;             // dt d_Qp was made for (-1: stale)
  std::vector<double> Qh;          // host copy of Q
  PoseShared sh{};
  uwvk_location loc{};
  uwvk_uwv_params uwv{};
  bool has_state = false, has_Q = false;
  int dense = 0;  // UWVK_OPT_DENSE_SIGMA
  // last-generation spreading of the PSP epoch launch (UWVK_OPT_TAIL_SLOTS)
  int64_t tail_slots = 0;  // resident blocks per XCD to plan for: 0 auto, < 0 off
  int tail_force = 0;      // UWVK_OPT_TAIL_CHUNKS: >= 2 forces that many chunks (tests)
  uint32_t* d_tail_flag = nullptr;  // per tail instance (batch / 8 - 1 per XCD at most)
  double* d_tail_carry = nullptr;   // per tail instance: 64 x (ds, ids)
  int64_t tail_inst_cap = 0;
  uint32_t tail_tag = 0;
  // persistent epoch kernel (UWVK_OPT_PERSIST): ticket counter and the value
  // it holds when the next launch starts (every launch takes units + grid)
  int persist = 1;  // UWVK_OPT_PERSIST (default since r06)
  uint32_t lds_pad = 0;  // UWVK_OPT_LDS_PAD (diagnostic occupancy sweep)
  // the parameter-decoupled epoch kernel (psp::PspSmemPD):
  // pdec = the 27 model-parameter DOFs' rows of Sigma are zero off the diagonal
  // (checked on the host at init; cleared by the full BodyEfforts update and by
  // any literal-kernel step, which do not keep those zeros exact)
  int pd_opt = 1;  // UWVK_OPT_PARAM_BLOCK
  int pair_opt = 1;  // UWVK_OPT_PAIR (default on): the PD kernel with two instances per wave (uwvk_psp_pair.hip)
  bool pdec = false;
  double* d_Qp_pd = nullptr;  // the PD table: the 26-DOF subset's {A A, dt^2 Q}, then the parameters' diagonal
  int wait_bound = -1;   // UWVK_OPT_WAIT_BOUND: < 0 the planner's bound, else that many sleeps (tests)
  uint32_t* d_ticket = nullptr;
  // hand-off fault word: pinned, coherent host memory the epoch kernel writes
  // directly (no copy on the stream); read after the stream has drained
  uint32_t* h_fault = nullptr;
  uint32_t* d_fault = nullptr;  // its device address
  uint32_t ticket_next = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  aug::VisStage vis;  // visual-landmark update staging
  std::vector<StageSlot> stages;  // uwvk_pose_run_log_visual: the shared visual inputs of a call
};

// literal (all 2n+1 sigma points) kernels requested?
// (and the body-frame SO3 side, which only the literal kernels implement)
// the literal kernels: on request, or for ukfom's literal apply_delta re-spread
// (the PSP kernels run both SO3 sides, sh.so3_right, since r04)
static bool use_dense(const uwvk_pose* h) { return h->dense || h->sh.literal_apply_delta; }

static PoseBufs bufs(const uwvk_pose* h) {
  PoseBufs b;
  b.batch = h->batch; b.mu = h->d_mu; b.sigma = h->d_sigma; b.Q = h->d_Q; b.rot = h->d_rot; b.off = h->d_off;
  b.model = h->d_model; b.uwv = h->d_uwv; b.status = h->d_status;
  b.shared = h->d_shared;
  b.Qp = h->d_Qp;
  b.qband = h->d_qband;
  return b;
}

static void set_shared(uwvk_pose* h, const uwvk_pose_parameter& p, const uwvk_location& loc,
                       const uwvk_uwv_params& uwv) {
  h->loc = loc;
  h->uwv = uwv;
  h->sh.p = p;
  double rm, rn;
  host::wgs84_radii(loc.latitude, &rm, &rn);
  h->sh.lat0 = loc.latitude;
  h->sh.lon0 = loc.longitude;
  h->sh.rm = rm;
  h->sh.inv_rm = 1.0 / rm;
  h->sh.slat0 = std::sin(loc.latitude);
  h->sh.clat0 = std::cos(loc.latitude);
  h->sh.rn_cos = rn * std::cos(loc.latitude);
  const double taus[8] = {p.gyro_bias_tau, p.acc_bias_tau, p.inertia_tau, p.lin_damping_tau, p.quad_damping_tau,
                          p.water_velocity_tau, p.adcp_bias_tau, p.water_density_tau};
  for (int k = 0; k < 8; k++) h->sh.ntau[k] = -1.0 / taus[k];
  h->qp_dt = -1.0;  // the packed {A_ii A_jj, dt^2 Q} table depends on the taus
  h->sh.uwv_weight = uwv.weight;
  h->sh.uwv_buoyancy = uwv.buoyancy;
  for (int k = 0; k < 3; k++) {
    h->sh.cog[k] = uwv.distance_body2centerofgravity[k];
    h->sh.cob[k] = uwv.distance_body2centerofbuoyancy[k];
  }
}

// what run_log's kernel choice depends on (uwvk_plan.hpp: runs_pd, runs_pair),
// with the Q shape of the current host Q
static EpochFacts facts(const uwvk_pose* h) {
  return {h->dof, h->batch, h->pd_opt, h->pair_opt, h->persist, h->lds_pad, use_dense(h), h->pdec,
          q_is_simple(h->dof, h->Qh), q_params_diag(h->dof, h->Qh)};
}

// PSP kernels read the batch-shared parameters and dt^2 Q (packed) from device
// memory: the tables of build_q_tables, uploaded once per dt
static hipError_t upload_shared(uwvk_pose* h, double dt) {
  hipError_t e = hipSuccess;
  if (dt != h->qp_dt) {
    const QTables t = build_q_tables(h->dof, h->Qh, h->sh.ntau, dt);
    static_assert(sizeof(t.qlo) == sizeof(h->sh.qlo) && sizeof(t.qoff) == sizeof(h->sh.qoff), "PoseShared's band");
    static_assert(Lay<53>::d_bg == 12 && Lay<53>::d_ba == 15 && Lay<53>::d_inertia == 19 && Lay<53>::d_wv == 46 &&
                      Lay<53>::d_rho == 52 && Lay<26>::d_wv == 19 && Lay<26>::d_rho == 25,
                  "the Markov blocks of build_q_tables");
    std::memcpy(h->sh.qlo, t.qlo, sizeof(t.qlo));
    std::memcpy(h->sh.qoff, t.qoff, sizeof(t.qoff));
    h->sh.q_band = t.q_band;
    h->sh.q_bw = t.q_bw;
    h->sh.q_simple = t.q_simple;
    auto upload = [&](double* d, const std::vector<double>& v) {
      return hipMemcpyAsync(d, v.data(), v.size() * 8, hipMemcpyHostToDevice, h->stream);
    };
    e = upload(h->d_Qp, t.qp);
    if (e == hipSuccess) e = upload(h->d_qband, t.band);
    if (e == hipSuccess) e = upload(h->d_Qp_pd, t.qpd);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // the tables are locals
    if (e != hipSuccess) return e;
    h->qp_dt = dt;
  }
  // unchanged since the last upload (a run_log after another): no copy in
  // front of the launch (a pageable 2-KB copy cost ~10 us of the timed window)
  if (h->sh_dev_ok && std::memcmp(&h->sh_dev, &h->sh, sizeof(PoseShared)) == 0) return hipSuccess;
  e = hipMemcpyAsync(h->d_shared, &h->sh, sizeof(PoseShared), hipMemcpyHostToDevice, h->stream);
  h->sh_dev_ok = e == hipSuccess;
  if (h->sh_dev_ok) h->sh_dev = h->sh;
  return e;
}

extern "C" {

uwvk_status uwvk_pose_create(int64_t batch, int dof, int device, uwvk_pose** out) {
  ::uwvk::DeviceGuard uwvk_device_guard_(device);
  if (!out || batch <= 0 || (dof != 53 && dof != 26)) return UWVK_EINVAL;
  *out = nullptr;
  if (!uwvk_device_available(device)) return UWVK_EDEVICE;
  uwvk_pose* h = new uwvk_pose();
  h->batch = batch;
  h->dof = dof;
  h->store = dof == 53 ? 54 : 27;
  h->device = device;
  h->sh.so3_right = 1;  // MTK's SO3::boxplus, q exp(d): the default side since r05 (UWVK_OPT_SO3_RIGHT)
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
    delete h;
    return UWVK_EDEVICE;
  }
  const size_t B = (size_t)batch, n = (size_t)dof;
  // Sigma: packed lower triangle per instance (B n (n + 1) / 2 doubles)
  bool ok = hipMalloc(&h->d_mu, B * h->store * 8) == hipSuccess &&
            hipMalloc(&h->d_sigma, B * (n * (n + 1) / 2) * 8) == hipSuccess &&
            hipMalloc(&h->d_Q, n * n * 8) == hipSuccess && hipMalloc(&h->d_rot, B * 3 * 8) == hipSuccess &&
            hipMalloc(&h->d_off, B * 28 * 8) == hipSuccess && hipMalloc(&h->d_model, B * 27 * 8) == hipSuccess &&
            hipMalloc(&h->d_uwv, 108 * 8) == hipSuccess && hipMalloc(&h->d_status, B * 4) == hipSuccess &&
            hipMalloc(&h->d_meas, B * 74 * 8) == hipSuccess && hipMalloc(&h->d_mask, B) == hipSuccess &&
            hipMalloc(&h->d_accepted, B) == hipSuccess && hipMalloc(&h->d_scratch, (B * 3 + 256 + ((B + 63) / 64) * kStatsMaxOut) * 8) == hipSuccess &&
            hipMalloc(&h->d_shared, sizeof(PoseShared)) == hipSuccess &&
            hipMalloc(&h->d_Qp, n * (n + 1) * 8) == hipSuccess && hipMalloc(&h->d_qband, kQBand * 8) == hipSuccess &&
            hipMalloc(&h->d_Qp_pd, kQpdEntries * 2 * 8) == hipSuccess &&
            hipMalloc(&h->d_ticket, 4) == hipSuccess &&
            hipHostMalloc((void**)&h->h_fault, 4, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
            hipHostGetDevicePointer((void**)&h->d_fault, h->h_fault, 0) == hipSuccess &&
            hipEventCreate(&h->ev0) == hipSuccess && hipEventCreate(&h->ev1) == hipSuccess;
  if (!ok) {
    uwvk_pose_destroy(h);
    return UWVK_ENOMEM;
  }
  (void)hipMemsetAsync(h->d_status, 0, B * 4, h->stream);
  (void)hipMemsetAsync(h->d_rot, 0, B * 3 * 8, h->stream);
  (void)hipMemsetAsync(h->d_Q, 0, n * n * 8, h->stream);
  (void)hipMemsetAsync(h->d_ticket, 0, 4, h->stream);
  *h->h_fault = 0;
  if (hipStreamSynchronize(h->stream) != hipSuccess) {
    uwvk_pose_destroy(h);
    return UWVK_EDEVICE;
  }
  *out = h;
  return UWVK_OK;
}

void uwvk_pose_destroy(uwvk_pose* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return;
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  for (void* p : {(void*)h->d_mu, (void*)h->d_sigma, (void*)h->d_Q, (void*)h->d_rot, (void*)h->d_off,
                  (void*)h->d_model, (void*)h->d_uwv, (void*)h->d_status, (void*)h->d_meas, (void*)h->d_mask,
                  (void*)h->d_accepted, (void*)h->d_scratch, (void*)h->d_shared, (void*)h->d_Qp, (void*)h->d_qband,
                  (void*)h->d_Qp_pd,
                  (void*)h->d_tail_flag, (void*)h->d_tail_carry, (void*)h->d_ticket})
    if (p) (void)hipFree(p);
  if (h->h_fault) (void)hipHostFree(h->h_fault);
  h->vis.release();
  stage_release(h->stages);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

int64_t uwvk_pose_batch(const uwvk_pose* h) { return h ? h->batch : 0; }
int uwvk_pose_dof(const uwvk_pose* h) { return h ? h->dof : 0; }
void* uwvk_pose_stream(const uwvk_pose* h) { return h ? (void*)h->stream : nullptr; }
// a tail-chunk hand-off that timed out in a launch that has completed (the
// kernel wrote the handle's host-mapped fault word); reported once
static bool take_fault(uwvk_pose* h) { return __atomic_exchange_n(h->h_fault, 0u, __ATOMIC_ACQ_REL) != 0; }

uwvk_status uwvk_pose_synchronize(uwvk_pose* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  const hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return (uwvk_status)::uwvk::edevice_status(e, "uwvk_pose_synchronize");
  return take_fault(h) ? UWVK_ESCHEDULE : UWVK_OK;
}

// Both init calls replace the reference's constructors (PoseUKF.cpp:288-391):
// the filter object is new, so the process noise is zero until it is set again
// and the stored rotation rate is zero (:380); the handle keeps its stream,
// buffers and options.
static uwvk_status upload_state(uwvk_pose* h, const std::vector<double>& x, const std::vector<double>& P,
                                const std::vector<double>& off, const std::vector<double>& model) {
  const size_t n = (size_t)h->dof;
  h->Qh.assign(n * n, 0.0);
  h->qp_dt = -1.0;
  for (double& v : h->sh.q_ori) v = 0.0;
  for (double& v : h->sh.q_wv) v = 0.0;
  HIPCHK(hipMemsetAsync(h->d_Q, 0, n * n * 8, h->stream));
  HIPCHK(hipMemsetAsync(h->d_rot, 0, (size_t)h->batch * 3 * 8, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_mu, x.data(), x.size() * 8, hipMemcpyHostToDevice, h->stream));
  // HBM keeps the packed lower triangle (the caller's P is the full matrix;
  // its lower triangle is taken, like the Cholesky-based ukfom reads it)
  const int tn = h->dof * (h->dof + 1) / 2;
  std::vector<double> Pp((size_t)h->batch * tn);
  for (int64_t b = 0; b < h->batch; b++)
    for (int i = 0, k = 0; i < h->dof; i++)
      for (int j = 0; j <= i; j++, k++) Pp[b * tn + k] = P[(b * h->dof + i) * h->dof + j];
  HIPCHK(hipMemcpyAsync(h->d_sigma, Pp.data(), Pp.size() * 8, hipMemcpyHostToDevice, h->stream));
  h->pdec = param_block_decoupled(h->dof, h->batch, Pp.data());
  HIPCHK(hipMemcpyAsync(h->d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_model, model.data(), model.size() * 8, hipMemcpyHostToDevice, h->stream));
  double uw[108];
  std::memcpy(uw, h->uwv.inertia_matrix, 36 * 8);
  std::memcpy(uw + 36, h->uwv.damping_matrices[0], 36 * 8);
  std::memcpy(uw + 72, h->uwv.damping_matrices[1], 36 * 8);
  HIPCHK(hipMemcpyAsync(h->d_uwv, uw, sizeof(uw), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->d_status, 0, (size_t)h->batch * 4, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->has_state = true;
  return UWVK_OK;
}

uwvk_status uwvk_pose_init_from_config(uwvk_pose* h, const double* pos, const double* pos_cov, const double* rot,
                                       const double* rot_cov, const uwvk_pose_config* cfg, const uwvk_uwv_params* uwv,
                                       const double imu_in_body[7]) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !pos || !pos_cov || !rot || !rot_cov || !cfg || !uwv) return UWVK_EINVAL;
  const int64_t B = h->batch;
  const int n = h->dof, s = h->store;
  std::vector<double> x(B * s), P(B * n * n), off(B * 28), model(B * 27);
  uwvk_pose_parameter par{};
  for (int64_t i = 0; i < B; i++) {
    host::pose_initial_state(n, pos + 3 * i, pos_cov + 9 * i, rot + 4 * i, rot_cov + 9 * i, *cfg, *uwv, imu_in_body,
                             &x[i * s], &P[i * n * n], &par);
    host::pose_offsets(n, &x[i * s], &off[i * 28]);
    host::model_blocks(*uwv, &model[i * 27]);
  }
  set_shared(h, par, cfg->location, *uwv);
  return upload_state(h, x, P, off, model);
}

uwvk_status uwvk_pose_init_from_state(uwvk_pose* h, const double* x, const double* P, const uwvk_location* loc,
                                      const uwvk_uwv_params* uwv, const uwvk_pose_parameter* param) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !x || !P || !loc || !uwv || !param) return UWVK_EINVAL;
  const int64_t B = h->batch;
  const int n = h->dof, s = h->store;
  std::vector<double> xs(x, x + B * s), Ps(P, P + B * n * n), off(B * 28), model(B * 27);
  for (int64_t i = 0; i < B; i++) {
    host::pose_offsets(n, &xs[i * s], &off[i * 28]);
    host::model_blocks(*uwv, &model[i * 27]);
  }
  set_shared(h, *param, *loc, *uwv);
  return upload_state(h, xs, Ps, off, model);
}

uwvk_status uwvk_pose_set_process_noise_from_config(uwvk_pose* h, const uwvk_pose_config* cfg, double imu_delta_t,
                                                    const double q_imu_in_body[4]) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !cfg || !(imu_delta_t > 0)) return UWVK_EINVAL;
  std::vector<double> Q(h->dof * h->dof);
  host::pose_process_noise(h->dof, *cfg, imu_delta_t, q_imu_in_body, Q.data());
  return uwvk_pose_set_process_noise(h, Q.data());
}

uwvk_status uwvk_pose_set_process_noise(uwvk_pose* h, const double* Q) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !Q) return UWVK_EINVAL;
  HIPCHK(hipMemcpyAsync(h->d_Q, Q, (size_t)h->dof * h->dof * 8, hipMemcpyHostToDevice, h->stream));
  h->Qh.assign(Q, Q + (size_t)h->dof * h->dof);
  h->qp_dt = -1.0;
  {
    const int n = h->dof, o = 3, wv = n == 53 ? 46 : 19;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) h->sh.q_ori[r * 3 + c] = Q[(o + r) * n + o + c];
    for (int k = 0; k < 4; k++) h->sh.q_wv[k] = Q[(wv + k) * n + wv + k];
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->has_Q = true;
  return UWVK_OK;
}

uwvk_status uwvk_pose_set_rotation_rate(uwvk_pose* h, const double* w, const double* cov) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !w) return UWVK_EINVAL;
  if (!finite_all(w, (size_t)h->batch * 3) || (cov && !finite_all(cov, (size_t)h->batch * 9))) return UWVK_ENAN;
  HIPCHK(hipMemcpyAsync(h->d_rot, w, (size_t)h->batch * 3 * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_pose_predict(uwvk_pose* h, double dt) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  PoseBufs b = bufs(h);
  if (use_dense(h)) {
    h->pdec = false;  // the literal covariance GEMM does not keep the parameter block's zeros exact
    HIPCHK(launch_pose_predict(h->dof, h->stream, b, h->sh, dt));
  }
  else {
    // upload_shared recomputes the Q shape (q_bw, q_simple, qlo, qoff) for this dt:
    // the by-value PoseShared handed to the kernel must be taken after it
    HIPCHK(upload_shared(h, dt));
    const PoseShared sh = h->sh;
    HIPCHK(launch_psp_predict(h->dof, h->stream, b, sh, dt));
  }
  return UWVK_OK;
}

}  // extern "C"

template <int K>
static uwvk_status launch_update(uwvk_pose* h, int m, const double* mu, const double* cov, const double* shared_cov,
                                 const uint8_t* mask, uint8_t* accepted, const double* extra, int extra_w,
                                 const double* v3, int only_vel) {
  if (!h || !mu || (!cov && !shared_cov)) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  const int64_t B = h->batch;
  // checkMeasurment [EXT] (PoseUKF.cpp:478): NaN -> error, nothing applied
  for (int64_t i = 0; i < B; i++) {
    if (mask && !mask[i]) continue;
    if (!finite_all(mu + i * m, m) || (cov && !finite_all(cov + i * m * m, (size_t)m * m))) return UWVK_ENAN;
  }
  if (!cov && !finite_all(shared_cov, (size_t)m * m)) return UWVK_ENAN;
  MeasArgs ma{};
  double* dmu = h->d_meas;
  double* dcov = h->d_meas + B * 36;
  double* dext = h->d_meas + B * 72;
  HIPCHK(hipMemcpyAsync(dmu, mu, (size_t)B * m * 8, hipMemcpyHostToDevice, h->stream));
  ma.mu = dmu;
  if (cov) {
    HIPCHK(hipMemcpyAsync(dcov, cov, (size_t)B * m * m * 8, hipMemcpyHostToDevice, h->stream));
    ma.cov = dcov;
  } else {
    std::memcpy(ma.shared_cov, shared_cov, (size_t)m * m * 8);
  }
  if (mask) {
    HIPCHK(hipMemcpyAsync(h->d_mask, mask, (size_t)B, hipMemcpyHostToDevice, h->stream));
    ma.mask = h->d_mask;
  }
  if (extra) {
    HIPCHK(hipMemcpyAsync(dext, extra, (size_t)B * extra_w * 8, hipMemcpyHostToDevice, h->stream));
    ma.extra = dext;
  }
  if (v3)
    for (int k = 0; k < 3; k++) ma.v3[k] = v3[k];
  ma.only_vel = only_vel;
  ma.accepted = h->d_accepted;
  PoseBufs b = bufs(h);
  // BodyEfforts on PSP too (r05): the full model with k = 48 (psp_update_eff),
  // its velocity-only form (constrainVelocity) with k = 9
  // the literal kernels, and the full BodyEfforts model (non-affine in the
  // parameters), couple the parameter block: no PD kernel afterwards
  if (use_dense(h) || (K == MK_EFFORTS && !only_vel)) h->pdec = false;
  if (use_dense(h))
    HIPCHK(launch_pose_update(h->dof, K, h->stream, b, h->sh, ma, m));
  else {
    HIPCHK(upload_shared(h, h->qp_dt));
    const PoseShared sh = h->sh;  // after upload_shared (it refreshes the Q shape)
    HIPCHK(launch_psp_update(h->dof, K, h->stream, b, sh, ma, m));
  }
  if (accepted) HIPCHK(hipMemcpyAsync(accepted, h->d_accepted, (size_t)B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

extern "C" {

uwvk_status uwvk_pose_update_acceleration(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                          const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  return launch_update<MK_ACC>(h, 3, mu, cov, sc, mask, acc, nullptr, 0, nullptr, 0);
}
uwvk_status uwvk_pose_update_velocity(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                      const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  return launch_update<MK_VEL>(h, 3, mu, cov, sc, mask, acc, nullptr, 0, nullptr, 0);
}
uwvk_status uwvk_pose_update_pressure(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                      const double sensor_in_imu[3], const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  const double zero[3] = {0, 0, 0};
  return launch_update<MK_PRESSURE>(h, 1, mu, cov, sc, mask, acc, nullptr, 0, sensor_in_imu ? sensor_in_imu : zero, 0);
}
uwvk_status uwvk_pose_update_water_velocity(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                            const double* cw, const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  if (!cw) return UWVK_EINVAL;
  return launch_update<MK_WATER>(h, 2, mu, cov, sc, mask, acc, cw, 1, nullptr, 0);
}
uwvk_status uwvk_pose_update_efforts(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                     int only_affect_velocity, const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  return launch_update<MK_EFFORTS>(h, 6, mu, cov, sc, mask, acc, nullptr, 0, nullptr, only_affect_velocity ? 1 : 0);
}
uwvk_status uwvk_pose_update_xy(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  return launch_update<MK_XY>(h, 2, mu, cov, sc, mask, acc, nullptr, 0, nullptr, 0);
}
uwvk_status uwvk_pose_update_z(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                               const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  return launch_update<MK_Z>(h, 1, mu, cov, sc, mask, acc, nullptr, 0, nullptr, 0);
}
uwvk_status uwvk_pose_update_geographic(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                        const double gps_in_body[3], const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  const double zero[3] = {0, 0, 0};
  return launch_update<MK_GEO>(h, 2, mu, cov, sc, mask, acc, nullptr, 0, gps_in_body ? gps_in_body : zero, 0);
}
// integrateMeasurement(vector<VisualFeatureMeasurement>, feature_positions, marker_pose,
// cov_marker_pose, camera_config, camera_in_IMU) (PoseUKF.cpp:613-654)
uwvk_status uwvk_pose_update_visual_landmark(uwvk_pose* h, int32_t n_features, const double* features,
                                             const double* feature_cov, int feature_cov_per_instance,
                                             const double* feature_positions, const double* marker_pose,
                                             int marker_pose_per_instance, const double cov_marker_pose[36],
                                             const double camera[4], const double camera_in_imu[7],
                                             const uint8_t* mask) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  aug::VisArgs va{};
  const int st = aug::stage_visual(h->stream, h->batch, n_features, features, feature_cov, feature_cov_per_instance,
                                   feature_positions, marker_pose, marker_pose_per_instance, cov_marker_pose, camera,
                                   camera_in_imu, mask, &va, &h->vis);
  if (st != 0 || va.nf == 0) {
    (void)hipStreamSynchronize(h->stream);
    return (uwvk_status)st;
  }
  h->pdec = false;  // the literal augmented update (all sigma points)
  const hipError_t e = launch_pose_visual(h->dof, h->sh.so3_right, h->stream, bufs(h), va);
  return (uwvk_status)::uwvk::launch_sync_status(e, h->stream, "launch_pose_visual");
}

uwvk_status uwvk_pose_update_delayed_xy(uwvk_pose* h, const double* mu, const double* cov, const double* sc,
                                        const double* delayed_xy, const uint8_t* mask, uint8_t* acc) {
  UWVK_DEVICE_GUARD(h);
  if (!delayed_xy) return UWVK_EINVAL;
  return launch_update<MK_DELAYED>(h, 2, mu, cov, sc, mask, acc, delayed_xy, 2, nullptr, 0);
}

uwvk_status uwvk_pose_reset_with_external_pose(uwvk_pose* h, const double* pose) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !pose) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  const int64_t B = h->batch;
  std::vector<double> x(B * h->store);
  HIPCHK(hipMemcpyAsync(x.data(), h->d_mu, x.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int64_t i = 0; i < B; i++) std::memcpy(&x[i * h->store], pose + 7 * i, 7 * 8);  // PoseUKF.cpp:687-690
  HIPCHK(hipMemcpyAsync(h->d_mu, x.data(), x.size() * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_pose_get_state(uwvk_pose* h, double* x, double* P) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !x) return UWVK_EINVAL;
  HIPCHK(hipMemcpyAsync(x, h->d_mu, (size_t)h->batch * h->store * 8, hipMemcpyDeviceToHost, h->stream));
  if (!P) {
    HIPCHK(hipStreamSynchronize(h->stream));
    return UWVK_OK;
  }
  // packed lower triangle -> the full symmetric matrix
  const int n = h->dof, tn = n * (n + 1) / 2;
  std::vector<double> Pp((size_t)h->batch * tn);
  HIPCHK(hipMemcpyAsync(Pp.data(), h->d_sigma, Pp.size() * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int64_t b = 0; b < h->batch; b++) {
    const double* s = &Pp[b * tn];
    double* d = P + (size_t)b * n * n;
    for (int i = 0, k = 0; i < n; i++)
      for (int j = 0; j <= i; j++, k++) d[i * n + j] = d[j * n + i] = s[k];
  }
  return UWVK_OK;
}

uwvk_status uwvk_pose_get_rotation_rate(uwvk_pose* h, double* out) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !out) return UWVK_EINVAL;
  PoseBufs b = bufs(h);
  PoseShared sh = h->sh;
  double* d = h->d_scratch;
  HIPCHK(launch_pose_rotation_rate(h->dof, h->stream, b, sh, d));
  HIPCHK(hipMemcpyAsync(out, d, (size_t)h->batch * 3 * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_pose_get_status(uwvk_pose* h, uint32_t* status, int clear) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !status) return UWVK_EINVAL;
  HIPCHK(hipMemcpyAsync(status, h->d_status, (size_t)h->batch * 4, hipMemcpyDeviceToHost, h->stream));
  if (clear) HIPCHK(hipMemsetAsync(h->d_status, 0, (size_t)h->batch * 4, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

// flags and carries for `need` tail instances (sized once for the largest
// plan: 8 chunks of these slots), and this launch's flag tag
static hipError_t tail_buffers(uwvk_pose* h, int64_t need, int64_t cap) {
  if (need > h->tail_inst_cap) {
    // the previous buffers may still be read by a queued launch
    hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return e;
    if (h->d_tail_flag) (void)hipFree(h->d_tail_flag);
    if (h->d_tail_carry) (void)hipFree(h->d_tail_carry);
    h->d_tail_flag = nullptr;
    h->d_tail_carry = nullptr;
    h->tail_inst_cap = 0;
    cap = std::max(cap, need);
    e = hipMalloc(&h->d_tail_flag, (size_t)cap * 4);
    if (e == hipSuccess) e = hipMalloc(&h->d_tail_carry, (size_t)cap * 128 * 8);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_tail_flag, 0, (size_t)cap * 4, h->stream);
    if (e != hipSuccess) return e;
    h->tail_inst_cap = cap;
    h->tail_tag = 0;
  }
  if (++h->tail_tag >= (1u << 27)) {  // flags hold tag * 16 + chunks done: restart on zeroed flags
    hipError_t e = hipMemsetAsync(h->d_tail_flag, 0, (size_t)h->tail_inst_cap * 4, h->stream);
    if (e != hipSuccess) return e;
    h->tail_tag = 1;
  }
  return hipSuccess;
}

// the ensemble statistics' truth, by value in the kernel arguments: no upload
// in front of the kernel.  truth: host store-vector, or null (zeros, identity)
static StatTruth stat_truth(const uwvk_pose* h, const double* truth) {
  StatTruth t{};
  if (truth) std::memcpy(t.v, truth, h->store * 8);
  else t.v[3] = 1.0;
  t.right = h->sh.so3_right;
  return t;
}
// the ensemble partials' area, after the rotation-rate area: d_scratch + 256 + 3 batch
static double* stats_partials(const uwvk_pose* h) { return h->d_scratch + 256 + 3 * h->batch; }

static_assert(kFixDelayed == kDelayedArrive, "FixArgs::kinds holds the planner's arrival bit");

// LATCH: the state's XY position into every row r of `latched` with latch_epoch[r] = e
static hipError_t latch_epoch_rows(uwvk_pose* h, const DelayedEvents& ev, double* latched, int64_t e) {
  auto it = std::lower_bound(ev.latches.begin(), ev.latches.end(), std::make_pair(e, (int32_t)-1));
  LatchRows rows{};
  hipError_t le = hipSuccess;
  for (; le == hipSuccess && it != ev.latches.end() && it->first == e; ++it) {
    rows.row[rows.n++] = it->second;
    if (rows.n == kLatchRows) {
      le = launch_pose_latch(h->dof, h->stream, h->d_mu, h->batch, latched, rows);
      rows.n = 0;
    }
  }
  if (le == hipSuccess && rows.n > 0) le = launch_pose_latch(h->dof, h->stream, h->d_mu, h->batch, latched, rows);
  return le;
}

// FIX on PSP: epoch e's position fixes and its arriving delayed row in one launch (kinds: Launch::ev_any)
static hipError_t fix_psp(uwvk_pose* h, const PoseBufs& b, const PoseShared& sh, const uwvk_pose_fixes* fx,
                          const uwvk_pose_delayed* d, int64_t e, uint32_t kinds) {
  const int64_t B = h->batch;
  FixArgs fa{};
  fa.kinds = kinds;
  if (kinds & kFixDelayed) {
    const int64_t off = (int64_t)d->index[e] * B * 2;
    fa.dxy = d->xy + off;
    fa.latched = d->latched + off;
    std::memcpy(fa.dxy_cov, d->xy_cov, sizeof(fa.dxy_cov));
    fa.delayed_counts = d->accept_counts;
  }
  if (kinds & (UWVK_FIX_XY | UWVK_FIX_Z | UWVK_FIX_GEO)) {  // (an arrival alone: fx may be null)
    if (kinds & UWVK_FIX_XY) fa.xy = fx->xy + (int64_t)fx->xy_index[e] * B * 2;
    if (kinds & UWVK_FIX_Z) fa.z = fx->z + (int64_t)fx->z_index[e] * B;
    if (kinds & UWVK_FIX_GEO) fa.geo = fx->geo + (int64_t)fx->geo_index[e] * B * 2;
    std::memcpy(fa.xy_cov, fx->xy_cov, sizeof(fa.xy_cov));
    fa.z_cov = fx->z_cov;
    std::memcpy(fa.geo_cov, fx->geo_cov, sizeof(fa.geo_cov));
    std::memcpy(fa.gps_in_body, fx->gps_in_body, sizeof(fa.gps_in_body));
    fa.accept_counts = fx->accept_counts;
  }
  return launch_psp_fix(h->dof, h->stream, b, sh, fa);
}

// FIX on a dense handle: the literal k_pose_update per kind on the log's device
// rows, in the order XY, Z, Geographic, delayed (delayed_xy the latched row),
// each followed by its count kernel
static hipError_t fix_dense(uwvk_pose* h, const PoseBufs& b, const PoseShared& sh, const uwvk_pose_fixes* fx,
                            const uwvk_pose_delayed* d, int64_t e, uint32_t kinds) {
  const int64_t B = h->batch;
  auto fix = [&](int kind, int slot, int m, const double* row, const double* cov, const double* v3) {
    MeasArgs ma{};
    ma.mu = row;
    std::memcpy(ma.shared_cov, cov, (size_t)m * m * 8);
    if (v3)
      for (int k = 0; k < 3; k++) ma.v3[k] = v3[k];
    ma.accepted = fx->accept_counts ? h->d_accepted : nullptr;
    hipError_t le = launch_pose_update(h->dof, kind, h->stream, b, sh, ma, m);
    if (le == hipSuccess && fx->accept_counts) le = launch_fix_count(h->stream, h->d_accepted, B, slot, fx->accept_counts);
    return le;
  };
  hipError_t le = hipSuccess;
  if (kinds & UWVK_FIX_XY) le = fix(MK_XY, 0, 2, fx->xy + (int64_t)fx->xy_index[e] * B * 2, fx->xy_cov, nullptr);
  if (le == hipSuccess && (kinds & UWVK_FIX_Z)) le = fix(MK_Z, 1, 1, fx->z + (int64_t)fx->z_index[e] * B, &fx->z_cov, nullptr);
  if (le == hipSuccess && (kinds & UWVK_FIX_GEO))
    le = fix(MK_GEO, 2, 2, fx->geo + (int64_t)fx->geo_index[e] * B * 2, fx->geo_cov, fx->gps_in_body);
  if (le == hipSuccess && (kinds & kFixDelayed)) {
    const int64_t off = (int64_t)d->index[e] * B * 2;
    MeasArgs ma{};
    ma.mu = d->xy + off;
    std::memcpy(ma.shared_cov, d->xy_cov, sizeof(d->xy_cov));
    ma.extra = d->latched + off;
    ma.check_extra = 1;
    ma.accepted = d->accept_counts ? h->d_accepted : nullptr;
    le = launch_pose_update(h->dof, MK_DELAYED, h->stream, b, sh, ma, 2);
    if (le == hipSuccess && d->accept_counts) le = launch_delayed_count(h->stream, h->d_accepted, B, d->accept_counts);
  }
  return le;
}

// EPOCH_ONE / EPOCH_PAIR: the PSP epoch kernel over l's epochs.  ea: the log's
// arguments with first and count set; the launch's geometry is filled in here
static uwvk_status launch_epochs(uwvk_pose* h, const PoseBufs& b, const PoseShared& sh, EpochArgs ea, const Launch& l) {
  const bool pair = l.kind == EPOCH_PAIR;
  // the pair kernel runs a 53-DOF state decoupled only (runs_pair implies runs_pd there)
  if (pair && h->dof == 53 && !l.pd) return UWVK_EINVAL;
  // the persistent, ticket-ordered launch: the pair kernel's only form, the
  // default, and the static launch's stand-in where block placement is not
  // the round-robin its XCD-ordered tail needs (a partitioned device, another
  // runtime): tickets spread the tail without any placement assumption
  const bool spread = static_may_spread(h->batch, h->tail_slots, h->lds_pad);
  Geometry g;
  ea.ticket = nullptr;
  if (pair || h->persist || (spread && !xcd_round_robin(h->device))) {
    const int64_t slots = pair ? psp_pair_slots(h->device) : psp_epoch_slots(h->dof, h->device, true, l.pd);
    HIPCHK(slots > 0 ? hipSuccess : hipErrorInvalidValue);
    g = persist_geometry(pair ? h->batch / 2 : h->batch, slots, h->tail_slots, h->tail_force, h->lds_pad, l.count,
                         pair, h->wait_bound);
    // ticket_next advances only once the launch is queued: a launch that
    // fails leaves the device counter where it was
    ea.ticket = h->d_ticket;
    ea.ticket_base = h->ticket_next;
  } else {
    const int64_t slots = spread && h->tail_slots <= 0 ? psp_epoch_slots_per_xcd(h->dof, h->device, l.pd) : 0;
    g = static_geometry(h->batch, slots, h->tail_slots, h->tail_force, h->lds_pad, l.count, h->wait_bound);
  }
  if (g.tail_need > 0) {
    HIPCHK(tail_buffers(h, g.tail_need, g.tail_cap));
    ea.tail_flag = h->d_tail_flag;
    ea.tail_carry = h->d_tail_carry;
    ea.tag = h->tail_tag;
  }
  ea.chunks = g.chunks; ea.n_x = g.n_x; ea.tail0 = g.tail0; ea.r_x = g.r_x;
  ea.units = g.units; ea.wait_bound = g.wait_bound;
  PoseBufs bl = b;
  if (l.pd) bl.Qp = h->d_Qp_pd;
  const hipError_t le = pair ? launch_psp_epoch_pair(h->stream, bl, sh, ea, g.grid, l.ev_any, l.pd)
                             : launch_psp_epoch(h->dof, h->stream, bl, sh, ea, g.grid, l.ev_any, h->lds_pad, l.pd);
  if (le != hipSuccess) {
    ::uwvk::note_hip_error((int)le, pair ? "launch_psp_epoch_pair" : "launch_psp_epoch");
    // a persistent launch that did not run took no tickets: restart the
    // counter from zero (stream-ordered, before any later launch)
    if (ea.ticket) {
      h->ticket_next = 0;
      (void)hipMemsetAsync(h->d_ticket, 0, 4, h->stream);
    }
    return UWVK_EDEVICE;
  }
  if (ea.ticket) h->ticket_next += ea.units;  // the tickets the launch takes
  return UWVK_OK;
}

int64_t uwvk_pose_track_records(int64_t first, int64_t count, int64_t every) {
  return first < 0 || count < 0 || every <= 0 ? 0 : track_records(first, count, every);
}

// host only (no HIP call): what uwvk_pose_run_log_visual checks of its visual
// argument before it queues anything (the rules of uwvk_ipose_log_check)
uwvk_status uwvk_pose_visual_check(const uwvk_pose_visual* v, int64_t epochs, int64_t first, int64_t count) {
  if (!v || epochs < 0 || first < 0 || count < 0 || first > epochs || count > epochs - first) return UWVK_EINVAL;
  if (v->n_visual < 0 || (!v->visual_offset && v->n_visual != 0)) return UWVK_EINVAL;
  const VisualRows vr(*v);
  int64_t row0, row1;
  if (!visual_rows_valid(vr, first, count, &row0, &row1)) return UWVK_EINVAL;
  if (row1 > row0 && !visual_rows_finite(vr, row0, row1)) return UWVK_ENAN;
  return UWVK_OK;
}

// VISUAL: the rows of epoch e in one launch (kVisRunRows at most per launch;
// the state's round trip through HBM between two launches is exact)
static hipError_t visual_epoch_rows(uwvk_pose* h, const PoseBufs& b, const uwvk_pose_visual* vis, aug::VisRunArgs a,
                                    int64_t e) {
  const int64_t r0 = vis->visual_offset[e], r1 = vis->visual_offset[e + 1];
  hipError_t le = hipSuccess;
  for (int64_t r = r0; r < r1 && le == hipSuccess; r += aug::kVisRunRows) {
    a.row = r;
    a.rows = (int32_t)std::min<int64_t>(aug::kVisRunRows, r1 - r);
    le = launch_pose_visual_run(h->dof, h->sh.so3_right, h->stream, b, a);
  }
  return le;
}

// The five uwvk_pose_run_log* entry points: track, fx, dly and vis are each
// null or that call's argument.  After the argument checks
// (uwvk_pose_visual_check; fixes_valid and delayed_events, uwvk_plan.hpp) the
// whole call is planned once by plan_run and its launches are queued on the
// handle's stream in the plan's order.
static uwvk_status run_log(uwvk_pose* h, const uwvk_pose_log* log, int64_t first, int64_t count,
                           uint32_t* accept_counts, const uwvk_pose_track* track,
                           const uwvk_pose_fixes* fx = nullptr, const uwvk_pose_delayed* dly = nullptr,
                           const uwvk_pose_visual* vis = nullptr) {
  if (!h || !log) return UWVK_EINVAL;
  if (vis) {
    const uwvk_status chk = uwvk_pose_visual_check(vis, log->epochs, first, count);
    if (chk != UWVK_OK) return chk;
  }
  if (first < 0 || count < 0 || first + count > log->epochs || log->adcp_cells > 8) return UWVK_EINVAL;
  if (track && !track_args_valid(track->every, track->capacity, track->mean || track->variance || track->stats, first,
                                 count))
    return UWVK_EINVAL;
  if (fx && !fixes_valid(fx, first, count)) return UWVK_EINVAL;
  DelayedEvents events;
  if (dly && !delayed_events(dly, log->epochs, first, count, &events)) return UWVK_EINVAL;
  if (!h->has_state) return UWVK_ENOTINIT;
  // ABI 3: a hand-off timeout of an earlier, completed launch is reported here
  // (or by uwvk_pose_synchronize), before any new work is queued
  if (take_fault(h)) return UWVK_ESCHEDULE;
  EpochArgs ea{};
  ea.flags = log->flags; ea.gyro = log->gyro; ea.acc = log->acc;
  std::memcpy(ea.acc_cov, log->acc_cov, sizeof(ea.acc_cov));
  ea.dvl_index = log->dvl_index; ea.dvl = log->dvl;
  std::memcpy(ea.dvl_cov, log->dvl_cov, sizeof(ea.dvl_cov));
  ea.p_index = log->pressure_index; ea.pressure = log->pressure; ea.p_cov = log->pressure_cov;
  std::memcpy(ea.p_sens, log->pressure_sensor_in_imu, sizeof(ea.p_sens));
  ea.a_index = log->adcp_index; ea.adcp = log->adcp; ea.cells = log->adcp_cells;
  std::memcpy(ea.cw, log->adcp_cell_weighting, sizeof(ea.cw));
  std::memcpy(ea.adcp_cov, log->adcp_cov, sizeof(ea.adcp_cov));
  ea.e_index = log->efforts_index; ea.efforts = log->efforts;
  std::memcpy(ea.e_cov, log->efforts_cov, sizeof(ea.e_cov));
  ea.dt = log->dt;
  ea.accept_counts = accept_counts;
  PoseBufs b = bufs(h);
  std::vector<uint32_t> fl;
  const uint32_t* hf = nullptr;  // the flags of epochs first .. first + count - 1 (PSP)
  if (use_dense(h)) {
    h->pdec = false;
  } else {
    hf = log->host_flags ? log->host_flags + first : nullptr;
    if (!hf && count > 0) {
      fl.resize((size_t)count);
      HIPCHK(hipMemcpyAsync(fl.data(), log->flags + first, (size_t)count * 4, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      hf = fl.data();
    }
    std::memcpy(h->sh.log_acc_cov, log->acc_cov, sizeof(h->sh.log_acc_cov));
    std::memcpy(h->sh.log_dvl_cov, log->dvl_cov, sizeof(h->sh.log_dvl_cov));
    HIPCHK(upload_shared(h, log->dt));
    ea.fault = h->d_fault;
    ea.efforts_only = 0;
  }
  const PoseShared sh = h->sh;  // after upload_shared (it refreshes the Q shape)
  // the visual rows of the range: the per-epoch flags of the plan, and the
  // shared host inputs of all of the call's rows staged once (feature
  // positions, shared feature covariance, the rows' shared marker poses)
  std::vector<uint32_t> vfl;
  aug::VisRunArgs vra{};
  StageSlot* sg = nullptr;
  const int64_t vrow0 = vis && vis->visual_offset ? vis->visual_offset[first] : 0;
  const int64_t vrows = vis && vis->visual_offset ? vis->visual_offset[first + count] - vrow0 : 0;
  if (vrows > 0) {
    vfl.resize((size_t)count);
    for (int64_t k = 0; k < count; k++)
      vfl[(size_t)k] = vis->visual_offset[first + k + 1] > vis->visual_offset[first + k] ? 1u : 0u;
    const VisualRows vr(*vis);
    sg = stage_acquire(h->stages, visual_rows_words(vr, vrows) * 8);
    if (!sg) return UWVK_ENOMEM;
    const size_t w_all = visual_rows_stage(vr, vrow0, vrows, (double*)sg->host, (const double*)sg->dev, &vra.va,
                                           &vra.marker_rows);
    HIPCHK(hipMemcpyAsync(sg->dev, sg->host, w_all * 8, hipMemcpyHostToDevice, h->stream));
    sg->used = true;
    vra.row_base = vrow0;
    vra.applied = vis->applied;
  }
  const EpochPlan plan = plan_run(hf, fx ? fx->host_flags + first : nullptr, dly ? events.flags.data() : nullptr,
                                  track ? track->every : 0, first, count, facts(h), vrows > 0 ? vfl.data() : nullptr);
  const StageDone stage_done{sg, h->stream};  // when this function returns, early returns included
  const int s = h->store, nout = 3 * s + 2;
  int64_t r = 0;  // the next record of this call
  for (const Launch& l : plan.launches) {
    ea.first = l.first;
    ea.count = l.count;
    switch (l.kind) {
      case EPOCH_ONE:
      case EPOCH_PAIR: {
        const uwvk_status st = launch_epochs(h, b, sh, ea, l);
        if (st != UWVK_OK) return st;
        break;
      }
      case EPOCH_DENSE:  // the literal kernels: the epoch's predict and log updates fused
        HIPCHK(launch_pose_epoch(h->dof, h->stream, b, sh, ea));
        break;
      case EFFORTS:
        // constrainVelocity (PEffVO) or the full measurementEfforts (psp_update_eff)
        if (!l.vo) h->pdec = false;  // the full model couples the parameters (PD off from here)
        HIPCHK(launch_psp_efforts(h->dof, l.vo, h->stream, b, sh, ea));
        break;
      case FIX:  // the position updates leave pdec as it is
        HIPCHK(use_dense(h) ? fix_dense(h, b, sh, fx, dly, l.first, l.ev_any) : fix_psp(h, b, sh, fx, dly, l.first, l.ev_any));
        break;
      case VISUAL:  // the literal augmented update (all sigma points), as the single call
        h->pdec = false;
        HIPCHK(visual_epoch_rows(h, b, vis, vra, l.first));
        break;
      case LATCH:
        HIPCHK(latch_epoch_rows(h, events, dly->latched, l.first));
        break;
      case RECORD:  // the snapshot of the state the epoch's last launch stored, and the statistics, into slot r
        if (track->mean || track->variance)
          HIPCHK(launch_pose_track(h->dof, h->stream, h->d_mu, h->d_sigma, h->batch,
                                   track->mean ? track->mean + r * h->batch * s : nullptr,
                                   track->variance ? track->variance + r * h->batch * h->dof : nullptr));
        if (track->stats)
          HIPCHK(launch_pose_stats(h->dof, h->stream, b, stat_truth(h, track->truth ? track->truth + r * s : nullptr),
                                   track->stats + r * nout, stats_partials(h)));
        r++;
        break;
    }
  }
  return UWVK_OK;
}

uwvk_status uwvk_pose_run_log(uwvk_pose* h, const uwvk_pose_log* log, int64_t first, int64_t count,
                              uint32_t* accept_counts) {
  UWVK_DEVICE_GUARD(h);
  return run_log(h, log, first, count, accept_counts, nullptr);
}

uwvk_status uwvk_pose_run_log_track(uwvk_pose* h, const uwvk_pose_log* log, int64_t first, int64_t count,
                                    uint32_t* accept_counts, const uwvk_pose_track* track) {
  UWVK_DEVICE_GUARD(h);
  return run_log(h, log, first, count, accept_counts, track);
}

uwvk_status uwvk_pose_run_log_fixes(uwvk_pose* h, const uwvk_pose_log* log, const uwvk_pose_fixes* fixes,
                                    int64_t first, int64_t count, uint32_t* accept_counts,
                                    const uwvk_pose_track* track) {
  UWVK_DEVICE_GUARD(h);
  return run_log(h, log, first, count, accept_counts, track, fixes);
}

uwvk_status uwvk_pose_run_log_delayed(uwvk_pose* h, const uwvk_pose_log* log, const uwvk_pose_fixes* fixes,
                                      const uwvk_pose_delayed* delayed, int64_t first, int64_t count,
                                      uint32_t* accept_counts, const uwvk_pose_track* track) {
  UWVK_DEVICE_GUARD(h);
  return run_log(h, log, first, count, accept_counts, track, fixes, delayed);
}

uwvk_status uwvk_pose_run_log_visual(uwvk_pose* h, const uwvk_pose_log* log, const uwvk_pose_fixes* fixes,
                                     const uwvk_pose_delayed* delayed, const uwvk_pose_visual* visual, int64_t first,
                                     int64_t count, uint32_t* accept_counts, const uwvk_pose_track* track) {
  UWVK_DEVICE_GUARD(h);
  return run_log(h, log, first, count, accept_counts, track, fixes, delayed, visual);
}

uwvk_status uwvk_pose_ensemble_stats(uwvk_pose* h, const double* truth, double* out) {
  UWVK_DEVICE_GUARD(h);
  return uwvk_pose_ensemble_allreduce(h, truth, out, nullptr);
}

uwvk_status uwvk_pose_ensemble_allreduce(uwvk_pose* h, const double* truth, double* out, void* comm) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !out) return UWVK_EINVAL;
  const int s = h->store;
  const int nout = 3 * s + 2;
  double* d_out = h->d_scratch;
  PoseBufs b = bufs(h);
  HIPCHK(launch_pose_stats(h->dof, h->stream, b, stat_truth(h, truth), d_out, stats_partials(h)));
  if (comm) {  // RCCL sum across the ranks' shards, stream-ordered after the stats kernel
    const uwvk_status st = uwvk_comm_allreduce_sum_device(comm, d_out, nout, (void*)h->stream);
    if (st != UWVK_OK) return st;
  }
  HIPCHK(hipMemcpyAsync(out, d_out, nout * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return UWVK_OK;
}

uwvk_status uwvk_pose_set_option(uwvk_pose* h, int option, int value) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  if (option == UWVK_OPT_LITERAL_APPLY_DELTA) {
    h->sh.literal_apply_delta = value ? 1 : 0;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_DENSE_SIGMA) {
    h->dense = value ? 1 : 0;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_TAIL_SLOTS) {
    h->tail_slots = value;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_SO3_RIGHT) {
    h->sh.so3_right = value ? 1 : 0;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_TAIL_CHUNKS) {
    if (value < 0 || value > 8) return UWVK_EINVAL;
    h->tail_force = value;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_PERSIST) {
    h->persist = value ? 1 : 0;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_LDS_PAD) {  // diagnostic: occupancy sweep of the epoch kernel
    // the pad plus the kernel's static PspSmem<53> must fit gfx950's 160 KiB
    if (value < 0 || value > 160 * 1024 - (int)psp_epoch_lds_bytes(53)) return UWVK_EINVAL;
    h->lds_pad = (uint32_t)value;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_WAIT_BOUND) {  // tests: force hand-off timeouts (0 = every one)
    h->wait_bound = value;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_PARAM_BLOCK) {
    h->pd_opt = value ? 1 : 0;
    return UWVK_OK;
  }
  if (option == UWVK_OPT_PAIR) {
    h->pair_opt = value ? 1 : 0;
    return UWVK_OK;
  }
  return UWVK_EINVAL;
}

int64_t uwvk_pose_resident_slots(int dof, int device) {
  if (dof != 53 && dof != 26) return 0;
  return psp_epoch_slots_per_xcd(dof, device);
}

int uwvk_pose_param_block(uwvk_pose* h) { return (h && runs_pd(facts(h))) ? 1 : 0; }

int uwvk_pose_pair_active(uwvk_pose* h) { return (h && runs_pair(facts(h))) ? 1 : 0; }

int uwvk_xcd_round_robin(int device) { return xcd_round_robin(device); }

int uwvk_pose_epoch_qshape(const uwvk_pose* h) { return h ? (q_is_simple(h->dof, h->Qh) ? 1 : 2) : 0; }

int uwvk_pose_tail_chunks(int64_t instances_per_xcd, int64_t slots_per_xcd, int64_t epochs) {
  return plan_tail(instances_per_xcd, slots_per_xcd, epochs);
}

uwvk_status uwvk_pose_timer_start(uwvk_pose* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  HIPCHK(hipEventRecord(h->ev0, h->stream));
  return UWVK_OK;
}
uwvk_status uwvk_pose_timer_stop(uwvk_pose* h, float* ms) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !ms) return UWVK_EINVAL;
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return UWVK_OK;
}
uwvk_status uwvk_pose_timer_mark(uwvk_pose* h) {
  UWVK_DEVICE_GUARD(h);
  if (!h) return UWVK_EINVAL;
  HIPCHK(hipEventRecord(h->ev1, h->stream));
  return UWVK_OK;
}
uwvk_status uwvk_pose_timer_elapsed(uwvk_pose* h, float* ms) {
  UWVK_DEVICE_GUARD(h);
  if (!h || !ms) return UWVK_EINVAL;
  HIPCHK(hipEventSynchronize(h->ev1));
  HIPCHK(hipEventElapsedTime(ms, h->ev0, h->ev1));
  return UWVK_OK;
}

}  // extern "C"
