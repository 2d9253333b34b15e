/*
 * uwvk.h — C ABI of the MI355X-native batched UKF engine (PoseUKF / VelocityUKF).
 *
 * This is the drop-in boundary for the predict / measurement-update hot path of
 * tomcreutz/slam-uwv_kalman_filters.  The reference exposes single-instance C++
 * classes (src/PoseUKF.hpp:89-255, src/VelocityUKF.hpp:231-266) that derive from
 * pose_estimation::UnscentedKalmanFilter<State> [EXT].  Each entry point below
 * names the reference member it replaces (file:line).  Every call works on a
 * BATCH of independent filter instances held in device memory by the handle;
 * batch = 1 is the reference's single-instance case.
 *
 * Conventions
 *  - Plain C types only.  Host arrays passed in are borrowed for the duration
 *    of the call (copied to the device before it returns).
 *  - Arrays are instance-major: element [i][k] of a per-instance array of width
 *    K lives at index i*K + k.  Matrices are row-major, n x n.
 *  - Quaternions are stored (w, x, y, z).
 *  - One handle owns one HIP stream and is NOT thread-safe (the reference is
 *    not re-entrant either: PoseUKF.cpp:173, VelocityUKF.cpp:18).
 *  - Errors are returned as uwvk_status codes; the C++ facade
 *    (slam-uwv_kalman_filters_amd/include/uwv_kalman_filters_amd/PoseUKF.hpp)
 *    maps them to std::runtime_error like the reference's checkMeasurment [EXT]
 *    (PoseUKF.cpp:478) and the missing-model throw (VelocityUKF.cpp:117-118).
 *  - There is NO CPU fallback: without a usable gfx950 device every create call
 *    returns UWVK_EDEVICE.
 */
#ifndef UWVK_H_
#define UWVK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  A caller checks uwvk_abi_version() == UWVK_ABI_VERSION of the
 * header it was built against (the Python binding and the C++ facade do).
 *   1  round 1.
 *   2  uwvk_pose_ensemble_stats / _allreduce write 3*store+2 doubles (was
 *      3*store+1: the count of instances left out of the NEES sum was added);
 *      uwvk_pose_init_from_state reads only the lower triangle of P;
 *      uwvk_memcpy_h2d / _d2h wait for the buffer's own device only.
 *   3  (r05/r06) the default UWVK_OPT_SO3_RIGHT of pose and ipose handles is 1
 *      (body-frame SO3 [+], MTK's SO3::boxplus; was 0, nav frame): a caller
 *      that wants the old convention sets the option to 0;
 *      new entry points uwvk_last_device_error, uwvk_synth_normal_at,
 *      uwvk_ipose_set_option, uwvk_pose_track_records, uwvk_pose_run_log_track;
 *      a tail-chunk hand-off that timed out is an error of the API, not only
 *      the instances' UWVK_ST_SCHEDULE bit: the next uwvk_pose_synchronize
 *      or uwvk_pose_run_log on the handle after the launch has completed
 *      returns UWVK_ESCHEDULE (once); new option UWVK_OPT_WAIT_BOUND;
 *      UWVK_OPT_PERSIST defaults to 1 (no dispatch-order assumption);
 *      added within 3, purely additive (no existing struct, flag or entry
 *      point changed): uwvk_pose_fixes, UWVK_FIX_*, uwvk_pose_run_log_fixes,
 *      uwvk_schedule_fixes; uwvk_pose_delayed, uwvk_pose_run_log_delayed,
 *      uwvk_schedule_delayed; uwvk_bottom_log, uwvk_bottom_track, UWVK_BEV_*,
 *      uwvk_bottom_log_check, uwvk_bottom_run_log, uwvk_bottom_synchronize;
 *      uwvk_vel_get_status; uwvk_ipose_log, uwvk_ipose_track,
 *      uwvk_ipose_log_check, uwvk_ipose_run_log, uwvk_ipose_synchronize;
 *      uwvk_vel_log_host, uwvk_vel_track, uwvk_vel_log_check,
 *      uwvk_vel_run_log_track; uwvk_pose_visual, uwvk_pose_visual_check,
 *      uwvk_pose_run_log_visual. */
#define UWVK_ABI_VERSION 3

/* ---- status codes ------------------------------------------------------ */
typedef enum uwvk_status {
  UWVK_OK = 0,
  UWVK_EINVAL = 1,   /* bad argument (null handle, wrong size, unsupported layout) */
  UWVK_ENAN = 2,     /* NaN/Inf in a measurement mean or covariance (checkMeasurment [EXT]) */
  UWVK_ENOTPD = 3,   /* covariance not positive definite in at least one instance */
  UWVK_ENOMODEL = 4, /* VelocityUKF predict without setupMotionModel (VelocityUKF.cpp:117-118) */
  UWVK_EDEVICE = 5,  /* no gfx950 device / HIP runtime error */
  UWVK_ENOMEM = 6,
  UWVK_ENOTINIT = 7, /* state or process noise not initialised */
  UWVK_ESCHEDULE = 8 /* a run_log tail-chunk hand-off timed out (instances flagged UWVK_ST_SCHEDULE);
                        returned by the next uwvk_pose_synchronize / uwvk_pose_run_log */
} uwvk_status;

/* per-instance status bits (the *_get_status getters of every filter family) */
#define UWVK_ST_NOTPD 0x1u    /* Cholesky of Sigma failed (non-positive pivot) */
#define UWVK_ST_NAN 0x2u      /* non-finite measurement skipped for this instance */
#define UWVK_ST_NONFINITE 0x4u/* non-finite state after a step: RESERVED, no kernel raises it today (part of ABI 3) */
/* UWVK_ST_SCHEDULE: engine fault, a tail-chunk hand-off timed out (see
 * UWVK_OPT_TAIL_SLOTS; never observed outside forced tests).  The instance's
 * state is then INVALID, not merely late: the chunks after the lost hand-off
 * did not run, and the late predecessor may have left Sigma in the kernel's
 * time-scaled (unfolded) form.  Re-initialise a flagged instance
 * (uwvk_pose_init_from_state with a state of the caller's choosing) before
 * using it again. */
#define UWVK_ST_SCHEDULE 0x8u

/* ---- PoseState layout (src/PoseState.hpp:29-45) ------------------------ */
/* Full layout: 53 DOF, 54 stored scalars (SO3 as a quaternion).           */
/* Kinematic layout: the same without inertia / lin_damping / quad_damping */
/* (26 DOF, 27 stored scalars) — the "~30-dim" config of BASELINE.json.     */
#define UWVK_POSE_DOF_FULL 53
#define UWVK_POSE_STORE_FULL 54
#define UWVK_POSE_DOF_KIN 26
#define UWVK_POSE_STORE_KIN 27
/* storage offsets, full layout */
#define UWVK_S_POS 0
#define UWVK_S_QUAT 3
#define UWVK_S_VEL 7
#define UWVK_S_ACC 10
#define UWVK_S_BIAS_GYRO 13
#define UWVK_S_BIAS_ACC 16
#define UWVK_S_GRAVITY 19
#define UWVK_S_INERTIA 20      /* 3x3 column-major (PoseState.hpp:37) */
#define UWVK_S_LIN_DAMPING 29  /* 3x3 column-major */
#define UWVK_S_QUAD_DAMPING 38 /* 3x3 column-major */
#define UWVK_S_WATER_VEL 47
#define UWVK_S_WATER_VEL_BELOW 49
#define UWVK_S_BIAS_ADCP 51
#define UWVK_S_WATER_DENSITY 53

/* ---- configuration PODs (Eigen-free mirrors of PoseUKFConfig.hpp) ------ */
typedef struct uwvk_inertial_noise { /* InertialNoiseParameters, PoseUKFConfig.hpp:50-63 */
  double randomwalk[3];
  double bias_offset[3];
  double bias_instability[3];
  double bias_tau;
} uwvk_inertial_noise;

typedef struct uwvk_model_noise { /* DynamicModelNoiseParameters, PoseUKFConfig.hpp:65-97 */
  double body_efforts_std[6];
  double inertia_instability[9];
  double lin_damping_instability[9];
  double quad_damping_instability[9];
  double inertia_tau;
  double lin_damping_tau;
  double quad_damping_tau;
} uwvk_model_noise;

typedef struct uwvk_water_velocity { /* WaterVelocityParameters, PoseUKFConfig.hpp:20-48 */
  double tau;
  double limits;
  double measurement_std[3];
  double scale;
  double cell_size;
  double first_cell_blank;
  double minimum_correlation;
  double adcp_bias_tau;
  double adcp_bias_limits;
} uwvk_water_velocity;

typedef struct uwvk_location { /* LocationConfiguration, PoseUKFConfig.hpp:99-109 */
  double latitude;  /* rad */
  double longitude; /* rad */
  double altitude;  /* m */
} uwvk_location;

typedef struct uwvk_hydrostatics { /* HydrostaticConfiguration, PoseUKFConfig.hpp:145-157 */
  double water_density;
  double water_density_limits;
  double water_density_tau;
  double atmospheric_pressure;
  double pressure_std;
} uwvk_hydrostatics;

typedef struct uwvk_pose_config { /* PoseUKFConfig, PoseUKFConfig.hpp:159-194 (visual-landmark config: passed per call) */
  uwvk_inertial_noise acceleration;
  uwvk_inertial_noise rotation_rate;
  uwvk_model_noise model_noise_parameters;
  uwvk_water_velocity water_velocity;
  uwvk_location location;
  uwvk_hydrostatics hydrostatics;
  double max_jerk[3];
  double max_effort[6];
  double dynamic_model_min_depth;
} uwvk_pose_config;

/* [EXT] uwv_dynamic_model::UWVParameters, the subset the hot path reads
 * (PoseUKF.cpp:159-171, VelocityUKF.cpp:60-74).  6x6 matrices row-major.
 * Forces/torques follow M*nu_dot + C(nu)*nu + D_l*nu + D_q*|nu|*nu + g(q) = tau. */
typedef struct uwvk_uwv_params {
  double inertia_matrix[36];
  double damping_matrices[2][36]; /* [0] linear, [1] quadratic */
  double weight;
  double buoyancy;
  double distance_body2centerofgravity[3];
  double distance_body2centerofbuoyancy[3];
} uwvk_uwv_params;

/* PoseUKF::PoseUKFParameter, PoseUKF.hpp:46-76 */
typedef struct uwvk_pose_parameter {
  double imu_in_body[3];
  double gyro_bias_offset[3];
  double gyro_bias_tau;
  double acc_bias_offset[3];
  double acc_bias_tau;
  double inertia_tau;
  double lin_damping_tau;
  double quad_damping_tau;
  double water_velocity_tau;
  double water_velocity_limits;
  double water_velocity_scale;
  double adcp_bias_tau;
  double atmospheric_pressure;
  double water_density_tau;
} uwvk_pose_parameter;

/* ---- library ------------------------------------------------------------ */
int uwvk_abi_version(void);
/* 1 when a gfx950 device is visible and the kernels' code object loads. */
int uwvk_device_available(int device);
const char* uwvk_status_string(uwvk_status s);
/* The HIP error (name, message, failing entry point) behind the calling host
 * thread's most recent UWVK_EDEVICE, "" if none (diagnostics). */
const char* uwvk_last_device_error(void);

/* device memory helpers for device-resident logs (bench / run_log).
 * uwvk_memcpy_h2d / _d2h are synchronous with all work on the device that owns
 * the device-side buffer (they make that device current, wait for every
 * stream on it, the handles' non-blocking ones included, then copy); work
 * queued on OTHER devices is not waited for.
 * uwvk_memcpy_*_on are ordered on one stream (a handle's uwvk_*_stream) and
 * return once the copy has completed. */
uwvk_status uwvk_device_malloc(int device, size_t bytes, void** out);
uwvk_status uwvk_device_free(void* p);
uwvk_status uwvk_memcpy_h2d(void* dst, const void* src, size_t bytes);
uwvk_status uwvk_memcpy_d2h(void* dst, const void* src, size_t bytes);
uwvk_status uwvk_memcpy_h2d_on(void* dst, const void* src, size_t bytes, void* stream);
uwvk_status uwvk_memcpy_d2h_on(void* dst, const void* src, size_t bytes, void* stream);

/* Synthetic-log noise (host only, no device work): out[j * count + k] is the
 * k-th standard normal variate of stream `stream` (< 256) of global instance
 * first_instance + j, a pure function of (seed, instance, stream, k):
 * Philox4x32-10 blocks, Box-Muller (csrc/uwvk_synth.cpp).  Instance-sharded
 * runs therefore draw bitwise the rows of the full batch. */
uwvk_status uwvk_synth_normal(uint64_t seed, int64_t first_instance, int64_t batch, uint32_t stream, int64_t count,
                              double* out);
/* The variates [offset, offset + count) of the same per-(instance, stream)
 * sequences (uwvk_synth_normal is offset 0, group 0).  group 0: out[batch][count];
 * group g > 0 (count a multiple of g): record-major out[count / g][batch][g],
 * the logs' [epoch][instance][component] layout. */
uwvk_status uwvk_synth_normal_at(uint64_t seed, int64_t first_instance, int64_t batch, uint32_t stream,
                                 int64_t offset, int64_t count, int32_t group, double* out);

/* ======================================================================== */
/* PoseUKF                                                                   */
/* ======================================================================== */
typedef struct uwvk_pose uwvk_pose;

/* dof = 53 (PoseState) or 26 (kinematic subset).  Allocates device state. */
uwvk_status uwvk_pose_create(int64_t batch, int dof, int device, uwvk_pose** out);
void uwvk_pose_destroy(uwvk_pose* h);
int64_t uwvk_pose_batch(const uwvk_pose* h);
int uwvk_pose_dof(const uwvk_pose* h);
/* hipStream_t of the handle (as void*), for event timing by the caller. */
void* uwvk_pose_stream(const uwvk_pose* h);
uwvk_status uwvk_pose_synchronize(uwvk_pose* h);

/* Both init calls are the reference's constructors: every instance becomes a
 * NEW filter, so the process noise is zero until set again and the stored
 * rotation rate is zero (PoseUKF.cpp:380).
 *
 * PoseUKF::PoseUKF(pos, pos_cov, rot, rot_cov, cfg, uwv, imu_in_body)
 * (PoseUKF.hpp:100-103, PoseUKF.cpp:288-372).  Per instance: pos[3],
 * pos_cov[9], rot[4] (w,x,y,z), rot_cov[9].  imu_in_body = {tx,ty,tz,qw,qx,qy,qz}
 * (NULL = identity), shared by the batch. */
uwvk_status uwvk_pose_init_from_config(uwvk_pose* h, const double* pos, const double* pos_cov,
                                       const double* rot, const double* rot_cov,
                                       const uwvk_pose_config* cfg, const uwvk_uwv_params* uwv,
                                       const double imu_in_body[7]);
/* PoseUKF::PoseUKF(state, cov, location, uwv, param) (PoseUKF.hpp:113-115,
 * PoseUKF.cpp:374-391).  x: batch*store, P: batch*dof*dof. */
uwvk_status uwvk_pose_init_from_state(uwvk_pose* h, const double* x, const double* P,
                                      const uwvk_location* location, const uwvk_uwv_params* uwv,
                                      const uwvk_pose_parameter* param);
/* setProcessNoiseFromConfig (PoseUKF.hpp:126-127, PoseUKF.cpp:393-439);
 * q_imu_in_body (w,x,y,z) may be NULL (identity). */
uwvk_status uwvk_pose_set_process_noise_from_config(uwvk_pose* h, const uwvk_pose_config* cfg,
                                                    double imu_delta_t, const double q_imu_in_body[4]);
/* setProcessNoiseCovariance [EXT base]: dof*dof, shared by the batch. */
uwvk_status uwvk_pose_set_process_noise(uwvk_pose* h, const double* Q);

/* integrateMeasurement(RotationRate) (PoseUKF.cpp:492-496): stores omega.
 * w: batch*3, cov: batch*9 (checked for NaN only, may be NULL). */
uwvk_status uwvk_pose_set_rotation_rate(uwvk_pose* h, const double* w, const double* cov);
/* predictionStep(dt) -> predictionStepImpl (PoseUKF.cpp:446-474). */
uwvk_status uwvk_pose_predict(uwvk_pose* h, double dt);

/* Measurement updates.  mu: batch*m, cov: batch*m*m (NULL = shared_cov),
 * shared_cov: m*m used when cov == NULL.  mask: batch bytes, 0 = skip this
 * instance (NULL = all).  accepted (out, nullable): batch bytes, 1 when the
 * innovation gate passed and the state was updated. */
/* integrateMeasurement(Acceleration) (PoseUKF.cpp:484-490), m = 3 */
uwvk_status uwvk_pose_update_acceleration(uwvk_pose* h, const double* mu, const double* cov,
                                          const double* shared_cov, const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(Velocity) (PoseUKF.cpp:476-482), m = 3, DVL in IMU frame */
uwvk_status uwvk_pose_update_velocity(uwvk_pose* h, const double* mu, const double* cov,
                                      const double* shared_cov, const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(Pressure, sensor_in_imu) (PoseUKF.cpp:559-565), m = 1 */
uwvk_status uwvk_pose_update_pressure(uwvk_pose* h, const double* mu, const double* cov,
                                      const double* shared_cov, const double sensor_in_imu[3],
                                      const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(WaterVelocityMeasurement, cell_weighting)
 * (PoseUKF.cpp:604-611), m = 2, d2p95 gate.  cell_weighting: batch doubles. */
uwvk_status uwvk_pose_update_water_velocity(uwvk_pose* h, const double* mu, const double* cov,
                                            const double* shared_cov, const double* cell_weighting,
                                            const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(BodyEffortsMeasurement, only_affect_velocity)
 * (PoseUKF.cpp:581-602), m = 6. */
uwvk_status uwvk_pose_update_efforts(uwvk_pose* h, const double* mu, const double* cov,
                                     const double* shared_cov, int only_affect_velocity,
                                     const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(XY_Position) (PoseUKF.cpp:506-512), m = 2 */
uwvk_status uwvk_pose_update_xy(uwvk_pose* h, const double* mu, const double* cov,
                                const double* shared_cov, const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(Z_Position) (PoseUKF.cpp:498-504), m = 1 */
uwvk_status uwvk_pose_update_z(uwvk_pose* h, const double* mu, const double* cov,
                               const double* shared_cov, const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(GeographicPosition, gps_in_body) (PoseUKF.cpp:567-579),
 * m = 2 (lat, lon in rad), d2p95 gate. */
uwvk_status uwvk_pose_update_geographic(uwvk_pose* h, const double* mu, const double* cov,
                                        const double* shared_cov, const double gps_in_body[3],
                                        const uint8_t* mask, uint8_t* accepted);
/* integrateDelayedPositionMeasurement (PoseUKF.cpp:514-527): delayed_xy batch*2 */
uwvk_status uwvk_pose_update_delayed_xy(uwvk_pose* h, const double* mu, const double* cov,
                                        const double* shared_cov, const double* delayed_xy,
                                        const uint8_t* mask, uint8_t* accepted);
/* integrateMeasurement(vector<VisualFeatureMeasurement>, feature_positions, marker_pose,
 * cov_marker_pose, camera_config, camera_in_IMU) (PoseUKF.cpp:613-654): the state is
 * augmented with the marker pose (PoseStateWithMarker, :221-229), one S2-valued
 * update per feature (measurementVisualLandmark, :231-244; accept any Mahalanobis
 * distance), then reset to the leading block.  Per instance n_features features:
 *   features           [batch][nf][2] undistorted image coordinates (px)
 *   feature_cov        [batch][nf][4] (feature_cov_per_instance) or [nf][4], px^2
 *   feature_positions  [nf][3] in the marker frame (shared)
 *   marker_pose        [batch][7] (marker_pose_per_instance) or [7]: t(3), q(w,x,y,z)
 *   cov_marker_pose    [36] (shared), camera {fx, fy, cx, cy}, camera_in_imu t(3) q(4)
 * A NaN feature fails the whole call with UWVK_ENAN and changes nothing (the
 * reference throws before its ukf.reset). */
uwvk_status uwvk_pose_update_visual_landmark(uwvk_pose* h, int32_t n_features, const double* features,
                                             const double* feature_cov, int feature_cov_per_instance,
                                             const double* feature_positions, const double* marker_pose,
                                             int marker_pose_per_instance, const double cov_marker_pose[36],
                                             const double camera[4], const double camera_in_imu[7],
                                             const uint8_t* mask);
/* resetFilterWithExternalPose (PoseUKF.cpp:685-691): pose batch*7 {t, q(w,x,y,z)} */
uwvk_status uwvk_pose_reset_with_external_pose(uwvk_pose* h, const double* pose);

/* getCurrentState / ukf->mu(), ukf->sigma() [EXT]: x batch*store, P batch*dof*dof (nullable) */
uwvk_status uwvk_pose_get_state(uwvk_pose* h, double* x, double* P);
/* getRotationRate (PoseUKF.cpp:693-699): batch*3 */
uwvk_status uwvk_pose_get_rotation_rate(uwvk_pose* h, double* out);
/* Per-instance status words (UWVK_ST_*), batch uint32: waits for the handle's
 * stream, copies the words and, if clear, zeroes the device words.  Both init
 * calls zero them too (every instance becomes a new filter).  The bits are
 * sticky until then.  NULL handle or status: UWVK_EINVAL.
 *  - UWVK_ST_NAN: a non-finite measurement was skipped for that instance.
 *  - UWVK_ST_NOTPD: a Cholesky factorisation of that instance's Sigma met a
 *    non-positive pivot (negative, zero or NaN).  The call still returns
 *    UWVK_OK.  The step is NOT skipped: the flagged instance's state and
 *    covariance are overwritten and unspecified from then on (the full
 *    BodyEfforts kernel even factors Sigma in place; in a run the later epochs
 *    run on it as NaN); re-initialise the handle.  Every other instance,
 *    the partner in a wave of the two-instances-per-wave kernel included, is
 *    bitwise what it is beside a valid Sigma.
 *    Which pivots are seen depends on the path.  The literal kernels
 *    (UWVK_OPT_DENSE_SIGMA) and the CPU oracle factor all of Sigma at every
 *    step and see every pivot.  A PSP step factors the leading k tangent DOFs
 *    only and sees the first non-positive pivot p iff p < k:
 *    predict 15; acceleration, velocity (DVL), water velocity (ADCP) 6;
 *    pressure 19; BodyEfforts velocity-only 9; full BodyEfforts all of them;
 *    XY, Z, geographic and delayed XY 0, i.e. never.  run_log sees what its
 *    steps see, so a pivot below 15 at its first predict.  With p >= k the
 *    step's formulas stay defined and its result is finite: an indefinite
 *    Sigma whose leading 15 x 15 block is positive definite is not detected
 *    on the PSP paths until a pressure or full BodyEfforts step reaches it.
 *    A negative measurement variance is not screened (UWVK_ENAN is for
 *    non-finite values only): where it leaves Sigma - C K^T indefinite the
 *    update itself raises nothing, the next predict does (pivot < 15).
 *    tests/test_gpu_pose_edges.py pins all of this.
 *  - UWVK_ST_NONFINITE is reserved: no kernel raises it today.
 *  - UWVK_ST_SCHEDULE: see above. */
uwvk_status uwvk_pose_get_status(uwvk_pose* h, uint32_t* status, int clear);

/* ---- device-resident measurement log (persistent multi-epoch path) ----- */
/* Event flags per epoch (what the out-of-repo driver would call, §3 of SURVEY):
 * every epoch: RotationRate -> predictionStep(dt) -> Acceleration update;
 * then, when flagged: Velocity (DVL), Pressure, ADCP cells, BodyEfforts. */
#define UWVK_EV_ACC 0x1u
#define UWVK_EV_DVL 0x2u
#define UWVK_EV_PRESSURE 0x4u
#define UWVK_EV_ADCP 0x8u
#define UWVK_EV_EFFORTS 0x10u
#define UWVK_EV_EFFORTS_VELOCITY_ONLY 0x20u

typedef struct uwvk_pose_log {
  /* ALL pointers are DEVICE pointers (uwvk_device_malloc) unless noted. */
  int64_t epochs;
  double dt;                 /* predict step, seconds (host value) */
  const uint32_t* flags;     /* [epochs] UWVK_EV_* */
  const double* gyro;        /* [epochs][batch][3] */
  const double* acc;         /* [epochs][batch][3] */
  double acc_cov[9];         /* host value, shared */
  const int32_t* dvl_index;  /* [epochs] row into dvl (valid when EV_DVL) */
  const double* dvl;         /* [n_dvl][batch][3] */
  double dvl_cov[9];
  const int32_t* pressure_index;
  const double* pressure;    /* [n_pressure][batch] */
  double pressure_cov;
  double pressure_sensor_in_imu[3];
  const int32_t* adcp_index;
  const double* adcp;        /* [n_adcp][cells][batch][2] */
  int32_t adcp_cells;
  double adcp_cell_weighting[8]; /* host values, per cell */
  double adcp_cov[4];
  const int32_t* efforts_index;
  const double* efforts;     /* [n_efforts][batch][6] */
  double efforts_cov[36];
  /* HOST copy of flags (nullable): lets run_log plan its launches without a
   * device->host read of `flags`.  It must equal `flags`: run_log also picks
   * each launch's kernel from it (a launch whose host flags hold no pressure or
   * ADCP event runs a kernel without those updates). */
  const uint32_t* host_flags;
} uwvk_pose_log;

/* Runs epochs [first, first+count) of the log.  Default (PSP) path: one launch
 * per run of epochs, each instance's Sigma resident in LDS across the run;
 * BodyEfforts epochs run through the literal kernel (one launch per epoch).
 * UWVK_OPT_DENSE_SIGMA = 1: one literal fused launch per epoch.
 * accept_counts (device, nullable): [batch][4] uint32 accepted DVL/pressure/ADCP/efforts. */
uwvk_status uwvk_pose_run_log(uwvk_pose* h, const uwvk_pose_log* log, int64_t first, int64_t count,
                              uint32_t* accept_counts);

/* The filter's trajectory during a run: after every `every`-th epoch of the log
 * a record of all instances is written to the caller's DEVICE buffers, on the
 * handle's stream like the epochs themselves (no host synchronisation, no host
 * copy).  A record epoch ends a launch, as a BodyEfforts epoch does; a small
 * kernel then reads the state that launch stored. */
typedef struct uwvk_pose_track {
  int64_t every;        /* > 0.  A record is taken after each absolute epoch e of the log
                           with (e + 1) % every == 0, after all of that epoch's updates
                           (BodyEfforts included). */
  int64_t capacity;     /* records each non-NULL buffer below can hold */
  double* mean;         /* DEVICE [records][batch][store]   (nullable) */
  double* variance;     /* DEVICE [records][batch][dof]     diagonal of Sigma (nullable) */
  double* stats;        /* DEVICE [records][3*store+2]      layout of uwvk_pose_ensemble_stats (nullable) */
  const double* truth;  /* HOST   [records][store], read before the call returns; NULL = that
                           function's NULL truth.  Used only when stats != NULL. */
} uwvk_pose_track;

/* host only: the records of epochs [first, first+count),
 * floor((first+count)/every) - floor(first/every); 0 for every <= 0 or a negative range */
int64_t uwvk_pose_track_records(int64_t first, int64_t count, int64_t every);

/* uwvk_pose_run_log with a track.  Record r of the call is the r-th record epoch
 * inside [first, first+count); epochs are numbered from the log's start, so the
 * records of calls over adjacent ranges concatenate to those of one call.
 * The result is bitwise that of uwvk_pose_run_log on each segment between
 * record epochs with uwvk_pose_get_state / uwvk_pose_ensemble_stats at each cut:
 * every record, the final state, accept_counts and the kernel choice of later
 * calls.  track == NULL is uwvk_pose_run_log.
 * UWVK_EINVAL, with nothing queued and the state untouched: every <= 0; mean,
 * variance and stats all NULL; capacity < uwvk_pose_track_records(first, count,
 * every).  Otherwise the errors of uwvk_pose_run_log. */
uwvk_status uwvk_pose_run_log_track(uwvk_pose* h, const uwvk_pose_log* log, int64_t first, int64_t count,
                                    uint32_t* accept_counts, const uwvk_pose_track* track);

/* Position fixes as events of a device-resident run: XY (USBL / LBL,
 * integrateMeasurement(XY_Position), PoseUKF.cpp:506-512), Z (PoseUKF.cpp:498-504)
 * and GPS (integrateMeasurement(GeographicPosition, gps_in_body),
 * PoseUKF.cpp:567-579, d2p95 gate).  They have their own per-epoch flags (the
 * UWVK_EV_* bits and uwvk_pose_log are not extended); flags and row indices are
 * HOST arrays (a fix epoch ends a launch and the host plans it), the payloads
 * DEVICE arrays.  Order within an epoch: predict, Acceleration, DVL, pressure,
 * ADCP cells, BodyEfforts, then XY, Z, Geographic; a track record of that epoch
 * is taken after the fixes. */
#define UWVK_FIX_XY  0x1u
#define UWVK_FIX_Z   0x2u
#define UWVK_FIX_GEO 0x4u
typedef struct uwvk_pose_fixes {
  const uint32_t* host_flags;  /* HOST [log->epochs] UWVK_FIX_* per epoch, required */
  const int32_t* xy_index;     /* HOST [epochs] row into xy where UWVK_FIX_XY (NULL if never) */
  const double* xy;            /* DEVICE [n_xy][batch][2] */
  int64_t n_xy;
  double xy_cov[4];            /* host values, shared */
  const int32_t* z_index;      /* HOST [epochs] */
  const double* z;             /* DEVICE [n_z][batch] */
  int64_t n_z;
  double z_cov;
  const int32_t* geo_index;    /* HOST [epochs] */
  const double* geo;           /* DEVICE [n_geo][batch][2] lat, lon (rad) */
  int64_t n_geo;
  double geo_cov[4];
  double gps_in_body[3];
  uint32_t* accept_counts;     /* DEVICE [batch][3] XY, Z, GEO accepted (nullable) */
} uwvk_pose_fixes;

/* uwvk_pose_run_log_track with fixes.  The result is bitwise that of
 * uwvk_pose_run_log on each segment between fix epochs with uwvk_pose_update_xy,
 * _z and _geographic (in that order, on the same rows, with the shared
 * covariances and gps_in_body of `fixes`) at each cut: the final state, every
 * track record, accept_counts, the per-instance status and the kernel choice of
 * later calls (a fix does not couple the parameter block).  A non-finite fix
 * value is skipped for that instance and kind (UWVK_ST_NAN), as the log's other
 * sensors are; the call does not fail.
 * fixes == NULL is uwvk_pose_run_log_track (track == NULL too: uwvk_pose_run_log).
 * UWVK_EINVAL, with nothing queued and the state untouched, checked over
 * [first, first + count) before the first launch: host_flags NULL; a flag bit
 * outside UWVK_FIX_*; a flagged kind whose index or payload pointer is NULL; an
 * index outside [0, n_kind) at a flagged epoch.  Otherwise the errors of
 * uwvk_pose_run_log_track. */
uwvk_status uwvk_pose_run_log_fixes(uwvk_pose* h, const uwvk_pose_log* log, const uwvk_pose_fixes* fixes,
                                    int64_t first, int64_t count, uint32_t* accept_counts,
                                    const uwvk_pose_track* track /* nullable */);

/* Delayed XY fixes (USBL / LBL: a fix stamped t reaches the vehicle seconds
 * later; integrateDelayedPositionMeasurement, PoseUKF.cpp:514-527) as events of
 * a device-resident run.  A delayed sample is a payload row r with two epochs:
 *   latch epoch L[r] = latch_epoch[r]: after ALL updates of that epoch (its
 *     fixes and any delayed update of another row included), every instance's
 *     own position mu[pos.x, pos.y] is copied into latched[r];
 *   arrival epoch A[r] (index[A[r]] == r), A[r] > L[r]: the delayed update runs
 *     with delayed_xy = latched[r], z = xy[r] + (mu.xy - latched[r]).
 * Order within an epoch: predict, Acceleration, DVL, pressure, ADCP cells,
 * BodyEfforts, XY, Z, Geographic, delayed XY, the latches of that epoch, then a
 * track record.  The reference leaves the lookup of the delayed position to its
 * caller; this latch rule is the engine's own (unpinned), as the ADCP cell
 * weighting is.  latch_epoch[r] == -1: the caller filled latched[r] itself and
 * the run never writes that row (the reference's literal call form).
 * `latched` belongs to the caller and survives calls: a row latched in one call
 * may arrive in a later call over the adjacent range, and calls over adjacent
 * ranges give, bitwise, what one call over the whole range gives. */
typedef struct uwvk_pose_delayed {
  const int32_t* index;        /* HOST [log->epochs]: row arriving at epoch e, or -1 */
  const int32_t* latch_epoch;  /* HOST [n]: L[r], or -1 = caller-filled row */
  const double*  xy;           /* DEVICE [n][batch][2] the measured positions */
  int64_t n;
  double xy_cov[4];            /* host, shared */
  double* latched;             /* DEVICE [n][batch][2], written by the run at L[r], read at A[r] */
  uint32_t* accept_counts;     /* DEVICE [batch], nullable, caller zeroes */
} uwvk_pose_delayed;

/* uwvk_pose_run_log_fixes (fixes may be NULL) with delayed XY rows: over
 * [first, first + count) the call latches every row with L[r] in the range and
 * applies every row arriving in the range.  delayed == NULL is
 * uwvk_pose_run_log_fixes.  The result is bitwise that of uwvk_pose_run_log cut
 * after every latch, fix and arrival epoch, with at each cut the single calls
 * XY, Z, Geographic, then uwvk_pose_update_delayed_xy whose delayed_xy is the
 * x[:, 0:2] uwvk_pose_get_state returned at that row's latch cut, then the
 * latches: the final state, every track record, both accept-count arrays,
 * delayed->accept_counts, the per-instance status, `latched`, and the kernel
 * choice of later calls (a delayed update is linear in the position rows and
 * leaves the parameter block decoupled).  A sample whose value, shared
 * covariance or latched position is non-finite is skipped for that instance
 * only (UWVK_ST_NAN, PoseUKF.cpp:523); the call does not fail.
 * UWVK_EINVAL, with nothing queued and the state untouched, checked before the
 * first launch: index, latch_epoch, xy or latched NULL while n > 0; n < 0; an
 * index[e] outside [-1, n) at an epoch of the range; a latch_epoch[r] below -1
 * or at or beyond log->epochs; a row arriving in the range with latch_epoch[r]
 * >= its arrival epoch.  Otherwise the errors of uwvk_pose_run_log_fixes. */
uwvk_status uwvk_pose_run_log_delayed(uwvk_pose* h, const uwvk_pose_log* log,
                                      const uwvk_pose_fixes* fixes /* nullable */,
                                      const uwvk_pose_delayed* delayed /* nullable */,
                                      int64_t first, int64_t count, uint32_t* accept_counts,
                                      const uwvk_pose_track* track /* nullable */);

/* Visual-landmark observations (uwvk_pose_update_visual_landmark,
 * PoseUKF.cpp:613-654) as events of a device-resident run.  The rows are laid
 * out as the visual part of uwvk_ipose_log: epoch e integrates the rows
 * visual_offset[e] .. visual_offset[e+1]-1, in that order, after the epoch's
 * delayed XY update and before its latches. */
typedef struct uwvk_pose_visual {
  const int64_t* visual_offset;    /* HOST [log->epochs + 1], non-decreasing (CSR); NULL only if n_visual == 0 */
  int64_t n_visual;                /* visual rows */
  int32_t n_features;              /* features of every row, >= 1 if a row is used */
  const double* features;          /* DEVICE [n_visual][batch][n_features][2] */
  const double* feature_cov;       /* DEVICE [n_visual][batch][n_features][4], NULL = shared_feature_cov */
  const double* shared_feature_cov;/* HOST [n_features][4], serves every row */
  const double* feature_positions; /* HOST [n_features][3] */
  const double* marker_pose;       /* DEVICE [n_visual][batch][7], NULL = shared_marker_pose */
  const double* shared_marker_pose;/* HOST [n_visual][7], one per row */
  double cov_marker_pose[36];      /* host, shared */
  double camera[4];                /* host, shared: fx, fy, cx, cy */
  double camera_in_imu[7];         /* host, shared */
  uint32_t* applied;               /* DEVICE [batch], nullable, caller zeroes: the rows that changed the
                                      instance are added to it */
} uwvk_pose_visual;

/* host only, no device needed: the checks uwvk_pose_run_log_visual makes on its
 * visual argument before it queues anything, over epochs [first, first + count)
 * of a log of `epochs` epochs and their visual rows (the rules of
 * uwvk_ipose_log_check for the same fields).
 * UWVK_EINVAL: visual NULL; a negative range or one past `epochs`; n_visual < 0,
 * or visual_offset NULL while n_visual != 0; a visual_offset entry of the range
 * that is negative, above n_visual or below its predecessor; and, if the range
 * holds a visual row: n_features < 1; features or feature_positions NULL;
 * feature_cov and shared_feature_cov both NULL; marker_pose and
 * shared_marker_pose both NULL.
 * UWVK_ENAN: if the range holds a visual row, a non-finite value among
 * shared_feature_cov (when feature_cov is NULL), feature_positions, the range's
 * rows of shared_marker_pose (when marker_pose is NULL), cov_marker_pose,
 * camera, camera_in_imu. */
uwvk_status uwvk_pose_visual_check(const uwvk_pose_visual* visual, int64_t epochs, int64_t first, int64_t count);

/* uwvk_pose_run_log_delayed (fixes and delayed may be NULL) with visual rows.
 * visual == NULL is uwvk_pose_run_log_delayed.  Order within an epoch: predict,
 * Acceleration, DVL, pressure, ADCP cells, BodyEfforts, XY, Z, Geographic,
 * delayed XY, the epoch's visual rows in row order, the latches of that epoch,
 * then a track record.  One launch per visual epoch runs all of its rows with
 * the augmented (mu, Sigma) resident in LDS.
 *
 * The result is bitwise that of uwvk_pose_run_log_delayed cut after every epoch
 * with a visual row, with at each cut one uwvk_pose_update_visual_landmark per
 * row of that epoch, called with that row's payload, mask = the instances whose
 * payload of that row is finite, and the shared arrays passed as shared: the
 * final mu and Sigma, every track record, all accept-count arrays, `latched`,
 * the status words, and the kernel choice of later calls (a visual epoch ends
 * the parameter-decoupled kernels, as the single call does).  Calls over
 * adjacent ranges give bitwise what one call over the whole range gives.
 *
 * The payloads are in device memory, so what the single call refuses on the
 * host is handled per instance, as by uwvk_ipose_run_log:
 *  - a non-finite feature, feature covariance or per-instance marker pose of an
 *    instance at a row: that row is skipped for that instance, UWVK_ST_NAN;
 *  - a row in which any feature's update fails (at the sigma spread or in
 *    apply_delta's re-spread) is discarded for that instance as a whole:
 *    (mu, Sigma) as before the row, UWVK_ST_NOTPD, later rows and epochs run.
 *
 * Returns uwvk_pose_visual_check(visual, log->epochs, first, count) first (h or
 * log NULL: UWVK_EINVAL), then the errors of uwvk_pose_run_log_delayed, all
 * with nothing queued and the state untouched.  Asynchronous on the handle's
 * stream like the other runs: the host arrays are copied before it returns. */
uwvk_status uwvk_pose_run_log_visual(uwvk_pose* h, const uwvk_pose_log* log,
                                     const uwvk_pose_fixes* fixes /* nullable */,
                                     const uwvk_pose_delayed* delayed /* nullable */,
                                     const uwvk_pose_visual* visual /* nullable */,
                                     int64_t first, int64_t count, uint32_t* accept_counts,
                                     const uwvk_pose_track* track /* nullable */);

/* Ensemble statistics over the batch (for Monte-Carlo runs):
 * out[0..store)        = sum_i x_i (orientation quaternion summed componentwise)
 * out[store..2*store)  = sum_i x_i^2
 * out[2*store..3*store)= sum_i (x_i - truth)^2 (orientation: rotation-vector error, 3 entries used)
 * out[3*store]         = sum_i NEES_i over (position, orientation, velocity) (9 DOF),
 *                        over the instances whose 9x9 covariance block is positive definite
 * out[3*store+1]       = number of instances left out of that NEES sum (not positive definite / NaN)
 * truth: host store-vector (nullable -> zeros).  out: host doubles, 3*store+2. */
uwvk_status uwvk_pose_ensemble_stats(uwvk_pose* h, const double* truth, double* out);

/* Multi-GPU ensembles: one process (or thread) per GPU owns a
 * contiguous instance range; the only collective is this statistics sum over
 * RCCL.  `comm` is an RCCL communicator (ncclComm_t) as void*, from
 * uwvk_comm_init or the caller's own RCCL setup; NULL = this handle only (same
 * as uwvk_pose_ensemble_stats).  The sum runs on the handle's stream. */
uwvk_status uwvk_pose_ensemble_allreduce(uwvk_pose* h, const double* truth, double* out, void* comm);
/* RCCL communicator helpers (no RCCL headers needed by the caller): rank 0
 * calls uwvk_comm_unique_id and ships the uwvk_comm_unique_id_bytes() bytes to
 * the other ranks out of band; every rank then calls uwvk_comm_init. */
int uwvk_comm_unique_id_bytes(void);
uwvk_status uwvk_comm_unique_id(char* id);
uwvk_status uwvk_comm_init(int nranks, const char* id, int rank, int device, void** comm);
void uwvk_comm_destroy(void* comm);
uwvk_status uwvk_comm_allreduce_sum_device(void* comm, double* d_buf, int64_t n, void* stream);

/* Engine options (not part of the reference surface).
 * UWVK_OPT_LITERAL_APPLY_DELTA: 0 (default) applies ukfom's apply_delta through
 *   its exact nav-frame identity mu <- mu [+] d, Sigma <- T Sigma T^T
 *   (T rotates the orientation block by exp(d)); 1 runs the literal re-spread
 *   (Cholesky + sigma points + covariance GEMM).  Results agree to rounding. */
#define UWVK_OPT_LITERAL_APPLY_DELTA 1
/* UWVK_OPT_DENSE_SIGMA: 0 (default) evaluates ukfom's unscented transform in
 *   partitioned form (PSP): sigma points only along the Cholesky columns a model
 *   is non-affine in, the affine remainder in closed form (A Sigma A^T, H Sigma
 *   H^T); equal to the literal spread up to rounding.
 *   1 propagates all 2n+1 sigma points (MFMA covariance GEMM).  Setting
 *   UWVK_OPT_LITERAL_APPLY_DELTA also selects the literal kernels. */
#define UWVK_OPT_DENSE_SIGMA 2
/* UWVK_OPT_TAIL_SLOTS: last-generation spreading of the PSP run_log launch.
 *   When batch / 8 instances per XCD leave a partial last generation of the
 *   XCD's resident blocks, those tail instances run as a few epoch chunks
 *   handed from block to block (Sigma~ and its time scale unfolded, so the
 *   result is bitwise the one-block run), spread over the slots that would
 *   idle.  0 (default): plan for the occupancy the runtime reports; > 0: plan
 *   for that many resident blocks per XCD (tests); < 0: off.  Needs
 *   batch % 8 == 0. */
#define UWVK_OPT_TAIL_SLOTS 3
/* UWVK_OPT_TAIL_CHUNKS: 0 (default) the planner picks the chunk count; 2..8
 *   forces that many chunks per tail instance whenever the launch allows it
 *   (chunks x slots <= batch / 8, chunks <= epochs), for tests.  Spreading of
 *   any kind runs only where uwvk_xcd_round_robin(device) is 1. */
#define UWVK_OPT_TAIL_CHUNKS 4
/* UWVK_OPT_SO3_RIGHT: the side of the SO3 [+] / [-] [EXT MTK], SURVEY 8(c)
 *   item 5, the largest unpinned semantic.  1 (default since r05): body frame
 *   (right), q [+] d = q exp(d), MTK's published SO3::boxplus, through which the
 *   reference's orientation.boxplus runs (mtkwrap<MTK::SO3<double>>,
 *   PoseState.hpp:15; PoseUKF.cpp:32), in every orientation [+] / [-]: sigma
 *   points, processModel's orientation step, manifold mean, apply_delta, the
 *   visual update's filter and marker orientations and the ensemble
 *   statistics' orientation error (log(t^-1 q)).  0: nav frame (left),
 *   q [+] d = exp(d) q, an option (the convention SURVEY 8(c) had inferred
 *   from PoseUKF.cpp:31 / :451).  Every engine path runs either side (the PSP
 *   kernels are instantiated per side, SR); the oracle's or_set_so3_right is
 *   the same switch. */
#define UWVK_OPT_SO3_RIGHT 5
/* UWVK_OPT_PERSIST: scheduling of the PSP run_log launch.  1 (default since
 *   r06): persistent workgroups, as many as are resident, run their own unit
 *   first and then take work units (whole instances, then the epoch chunks of
 *   the last chunks x resident-slots instances) from a ticket counter: faster
 *   XCDs and CUs take more units, no workgroup dispatch between units, and a
 *   chunk's hand-off waits only on a unit a running workgroup holds (no
 *   placement or dispatch-order assumption).  0: one workgroup per instance
 *   (plus UWVK_OPT_TAIL_SLOTS spreading, which relies on the round-robin XCD
 *   placement of uwvk_xcd_round_robin and in-order dispatch; without the
 *   placement the launch falls back to the persistent form).  Results are
 *   bitwise the same.  (MI355X, C3 batch 65,536, four interleaved rounds: tie,
 *   200.6 against 200.9 M steps/s over 20 epochs, 219.2 against 219.1 M over
 *   200) */
#define UWVK_OPT_PERSIST 6
/* UWVK_OPT_LDS_PAD (diagnostic, r05): bytes of dynamic LDS requested per PSP
 *   epoch workgroup on top of its static 12.8 KB, unused by the kernel: it only
 *   lowers the resident workgroups per CU (12 -> 9 / 6 / 4 ...), to measure the
 *   epoch kernel's rate against occupancy.  0 default,
 *   at most 160 KiB minus the static 12.8 KB (else UWVK_EINVAL); a non-zero pad
 *   turns tail spreading off (the planners assume the unpadded occupancy). */
#define UWVK_OPT_LDS_PAD 7
/* UWVK_OPT_WAIT_BOUND (tests, r06): sleeps of ~1.7 us a tail chunk waits for
 *   its predecessor's hand-off before it gives up (UWVK_ST_SCHEDULE, and
 *   the next synchronize / run_log returns UWVK_ESCHEDULE).  < 0 (default): the planner's
 *   bound (~2 s plus 64-128 sleeps per epoch); 0 forces every hand-off of a
 *   spread launch to time out. */
#define UWVK_OPT_WAIT_BOUND 8
/* UWVK_OPT_PARAM_BLOCK (r06): 1 (default) runs run_log's PSP epoch launches of
 *   a 53-DOF handle on the parameter-decoupled kernel while the 27 model-
 *   parameter DOFs (inertia, linear / quadratic damping) are uncoupled: their
 *   rows of Sigma zero off the diagonal (as PoseUKF.cpp:333-335 make P0; checked
 *   on the host at init) and Q diagonal there (PoseUKF.cpp:417-422).  That
 *   kernel keeps the other 26 DOFs in the 26-DOF layout with the 53-DOF
 *   sigma-point weights and evolves each parameter alone; the results are the
 *   53-DOF kernel's.  The full BodyEfforts update (and
 *   any literal-kernel step) couples the block: the handle then runs the
 *   general kernel until it is re-initialised.  0: always the general kernel.
 *   uwvk_pose_param_block says which the next launch runs. */
#define UWVK_OPT_PARAM_BLOCK 9
/* UWVK_OPT_PAIR (r06, default 1): run_log runs two instances per wave (each on
 *   32 lanes; uwvk_psp_pair.hip) for 53-DOF handles while the parameter-
 *   decoupled kernel applies and for 26-DOF handles, on the persistent
 *   scheduler, an even batch and the lane-resident Q.  The pressure update's
 *   39 sigma points do not fit a half-wave: a launch is split around its
 *   pressure epochs (those run one instance per wave) when the runs between
 *   them are at least 48 epochs long.  The results agree with the one-instance
 *   kernel to rounding (the rank-M update sums in another order), gate
 *   decisions bitwise.  0: one instance per wave. */
#define UWVK_OPT_PAIR 10
uwvk_status uwvk_pose_set_option(uwvk_pose* h, int option, int value);
/* Host-only query (no device work): the chunks per tail instance the
 * UWVK_OPT_TAIL_SLOTS planner picks for one XCD's instances over its resident
 * blocks in an epochs-long launch; 1 = no spreading. */
int uwvk_pose_tail_chunks(int64_t instances_per_xcd, int64_t slots_per_xcd, int64_t epochs);
/* Resident PSP epoch-kernel blocks per XCD the runtime reports for this dof on
 * device (occupancy x CUs / 8; what UWVK_OPT_TAIL_SLOTS = 0 plans for), 0 if
 * unknown. */
int64_t uwvk_pose_resident_slots(int dof, int device);
/* Host-only query: the process-noise shape the PSP epoch kernel is
 * instantiated for on this handle's current Q: 1 = the lane-resident simple
 * shape (no coupling of the rewritten rows < 9, band <= 2; the default
 * configuration's), 2 = general (psp_predict QM). */
int uwvk_pose_epoch_qshape(const uwvk_pose* h);
/* Host-only query: 1 when the next run_log PSP launch runs the
 * parameter-decoupled kernel (UWVK_OPT_PARAM_BLOCK), else 0. */
int uwvk_pose_param_block(uwvk_pose* h);
/* Host-only query: 1 when run_log's launches (their epochs without a pressure
 * update) run the two-instances-per-wave form (UWVK_OPT_PAIR). */
int uwvk_pose_pair_active(uwvk_pose* h);
/* 1 when a probe grid on device showed round-robin workgroup placement over 8
 * XCCs (block b on the XCC of block b % 8, read from the hardware XCC_ID
 * register): the placement tail spreading's hand-off order relies on.  0 on a
 * partitioned device (or any other placement): spreading is then off.  The
 * probe runs once per device and process. */
int uwvk_xcd_round_robin(int device);

/* Kernel-timing helper: HIP events recorded on the handle's stream. */
uwvk_status uwvk_pose_timer_start(uwvk_pose* h);
uwvk_status uwvk_pose_timer_stop(uwvk_pose* h, float* elapsed_ms);
/* Split form of uwvk_pose_timer_stop: _mark records the stop event without
 * waiting, so work queued after it (the ensemble statistics) follows the
 * timed launches with no host round trip; _elapsed waits for that event and
 * returns the time since uwvk_pose_timer_start. */
uwvk_status uwvk_pose_timer_mark(uwvk_pose* h);
uwvk_status uwvk_pose_timer_elapsed(uwvk_pose* h, float* elapsed_ms);

/* ---- recorded-mission ingestion (host only, no device needed) ---------- */
/* The reference is driven by its caller's stream aligner (Rock orogen task,
 * outside the repository): RotationRate + predictionStep +
 * Acceleration per IMU sample (PoseUKF.cpp:446-496), the lower-rate sensors
 * integrated as their samples arrive (PoseUKF.cpp:476-611).  This turns the
 * per-sensor sample stamps of a recording into the epoch-indexed flags and
 * row indices of uwvk_pose_log (the payload arrays keep sample order).
 * Semantics: DESIGN.md §11 (fixed-step replay, lag < dt, per-sensor queue). */
typedef struct uwvk_stream_times { /* seconds, ascending per sensor; NULL when n = 0 */
  const double* imu;      int64_t n_imu;  /* one epoch per IMU sample */
  const double* dvl;      int64_t n_dvl;
  const double* pressure; int64_t n_pressure;
  const double* adcp;     int64_t n_adcp;  /* one sample = all cells of one ADCP ping */
  const double* efforts;  int64_t n_efforts;
  const uint8_t* efforts_velocity_only;    /* [n_efforts], nullable: only_affect_velocity */
} uwvk_stream_times;

typedef struct uwvk_schedule {
  /* caller-allocated HOST arrays of n_imu entries (index arrays may be NULL
   * when that sensor has no samples) */
  uint32_t* flags;         /* UWVK_EV_* per epoch */
  int32_t* dvl_index;      /* row of the sample integrated at that epoch, -1 = none */
  int32_t* pressure_index;
  int32_t* adcp_index;
  int32_t* efforts_index;
  /* outputs */
  double dt;               /* mean IMU interval (0 for a single sample) */
  int64_t epochs;
  int64_t kept[4];         /* DVL, pressure, ADCP, efforts samples placed */
  int64_t dropped[4];      /* before the first IMU stamp / queued past the last epoch */
} uwvk_schedule;

/* dt_tolerance: allowed |interval - dt| / dt of the IMU stream (non-uniform ->
 * UWVK_EINVAL); time_epsilon: stamp slack in seconds. */
uwvk_status uwvk_schedule_streams(const uwvk_stream_times* in, double dt_tolerance, double time_epsilon,
                                  uwvk_schedule* out);

/* The position-fix stamps of a recording placed on the epochs of its IMU
 * stream (imu[n_imu], ascending), for uwvk_pose_fixes: the release rule, the
 * per-sensor queue and the drop counting of uwvk_schedule_streams.  flags
 * [n_imu] receives UWVK_FIX_* (overwritten); each index array [n_imu] the row
 * of the sample integrated at that epoch, -1 = none (NULL allowed when that
 * sensor has no samples); rows are the kept samples in order.  kept / dropped:
 * XY, Z, GEO.  Stamps ascending per sensor, else UWVK_EINVAL. */
uwvk_status uwvk_schedule_fixes(const double* imu, int64_t n_imu,
                                const double* xy_t, int64_t n_xy, const double* z_t, int64_t n_z,
                                const double* geo_t, int64_t n_geo, double time_epsilon,
                                uint32_t* flags, int32_t* xy_index, int32_t* z_index, int32_t* geo_index,
                                int64_t kept[3], int64_t dropped[3]);

/* The delayed XY samples of a recording placed on its IMU epochs, for
 * uwvk_pose_delayed: sample s is stamped stamp_t[s] and reaches the vehicle at
 * arrival_t[s] >= stamp_t[s] (both arrays ascending, else UWVK_EINVAL).  By the
 * rule of uwvk_schedule_streams the latch epoch L is the first epoch whose IMU
 * stamp is >= stamp - time_epsilon, and the arrival epoch A is the largest of
 * the first epoch with stamp >= arrival - time_epsilon, L + 1 (the update needs
 * a latched position of an earlier epoch) and the next free arrival epoch (two
 * arrivals in one epoch are queued).  A sample stamped before the first IMU
 * stamp, or whose A falls past the last epoch, is dropped and counted; the kept
 * samples are the payload rows, in order.  index [n_imu] receives the row
 * arriving at each epoch (-1 = none), latch_epoch the L of the kept rows
 * (capacity n). */
uwvk_status uwvk_schedule_delayed(const double* imu, int64_t n_imu, const double* stamp_t,
                                  const double* arrival_t, int64_t n, double time_epsilon,
                                  int32_t* index, int32_t* latch_epoch, int64_t* kept, int64_t* dropped);

/* ADCP cell weighting for integrateMeasurement(WaterVelocityMeasurement,
 * cell_weighting) (PoseUKF.cpp:133-151,604-611) from cell_size and
 * first_cell_blank (PoseUKFConfig.hpp:34-38): 0 at the nearest cell centre,
 * 1 at the farthest, linear in range.  valid[i] (nullable) = correlation[i] >=
 * minimum_correlation (PoseUKFConfig.hpp:40-41), all 1 when correlation is NULL. */
uwvk_status uwvk_adcp_cell_weighting(const uwvk_water_velocity* wv, int32_t cells, const double* correlation,
                                     double* weighting, uint8_t* valid);

/* ======================================================================== */
/* VelocityUKF (src/VelocityUKF.hpp:231-266)                                 */
/* ======================================================================== */
#define UWVK_VEL_DOF 4
typedef struct uwvk_vel uwvk_vel;

uwvk_status uwvk_vel_create(int64_t batch, int device, uwvk_vel** out);
void uwvk_vel_destroy(uwvk_vel* h);
void* uwvk_vel_stream(const uwvk_vel* h);
/* VelocityUKF(state, cov) (VelocityUKF.cpp:49-56): x batch*4 {v, z}, P batch*16 */
uwvk_status uwvk_vel_init(uwvk_vel* h, const double* x, const double* P);
/* setupMotionModel (VelocityUKF.cpp:58-77) */
uwvk_status uwvk_vel_setup_motion_model(uwvk_vel* h, const uwvk_uwv_params* uwv);
/* GyroMeasurement (VelocityUKF.cpp:87-98): batch*3 */
uwvk_status uwvk_vel_set_gyro(uwvk_vel* h, const double* w, const double* cov);
/* BodyEffortsMeasurement (VelocityUKF.cpp:100-104): batch*6 */
uwvk_status uwvk_vel_set_efforts(uwvk_vel* h, const double* tau, const double* cov);
/* predictionStep -> predictionStepImpl (VelocityUKF.cpp:114-130) */
uwvk_status uwvk_vel_predict(uwvk_vel* h, double dt);
/* DVLMeasurement (VelocityUKF.cpp:79-85), m = 3 */
uwvk_status uwvk_vel_update_dvl(uwvk_vel* h, const double* mu, const double* cov, const double* shared_cov,
                                const uint8_t* mask);
/* PressureMeasurement (z) (VelocityUKF.cpp:106-112), m = 1 */
uwvk_status uwvk_vel_update_pressure(uwvk_vel* h, const double* mu, const double* cov, const double* shared_cov,
                                     const uint8_t* mask);
uwvk_status uwvk_vel_get_state(uwvk_vel* h, double* x, double* P);
/* motion-model side state: batch*13 {p(3), q(4: w,x,y,z), v(3), w(3)} */
uwvk_status uwvk_vel_get_model_state(uwvk_vel* h, double* out);
/* Per-instance status words: waits for the handle's stream, copies batch words
 * and, if clear, zeroes the device words (as the pose and bottom getters do).
 * NULL handle or status: UWVK_EINVAL.  The bits VelocityUKF raises:
 *  - UWVK_ST_NAN, sticky until cleared, by uwvk_vel_run_log_track alone: a
 *    non-finite sample or input of that instance was skipped.
 *  - UWVK_ST_NOTPD, sticky until cleared: the Cholesky factorisation at the
 *    start of a predict or an update (single calls and every run_log epoch
 *    alike) met a non-positive pivot.  The step is NOT skipped: the flagged
 *    instance's state and covariance are overwritten and unspecified from then
 *    on (unlike BottomUKF, which keeps the state it had); re-initialise it.
 *    The other instances are unaffected.
 *  - uwvk_vel_run_log does not screen the samples of its device-resident log
 *    (the single calls reject a non-finite one with UWVK_ENAN): a bad sample
 *    enters that instance's state and surfaces as UWVK_ST_NOTPD at the next
 *    step's factorisation, so one in a run's LAST step leaves no bit.  Use
 *    uwvk_vel_run_log_track (below) for logs that may hold drop-outs: it skips
 *    the bad sample for that instance and raises UWVK_ST_NAN. */
uwvk_status uwvk_vel_get_status(uwvk_vel* h, uint32_t* status, int clear);

typedef struct uwvk_vel_log {
  int64_t epochs;
  double dt;
  const uint32_t* flags;    /* UWVK_EV_DVL / UWVK_EV_PRESSURE */
  const double* gyro;       /* [epochs][batch][3] */
  const double* efforts;    /* [epochs][batch][6] */
  const int32_t* dvl_index;
  const double* dvl;        /* [n_dvl][batch][3] */
  double dvl_cov[9];
  const int32_t* pressure_index;
  const double* pressure;   /* [n_pressure][batch] (z position) */
  double pressure_cov;
} uwvk_vel_log;
/* Runs epochs [first, first + count): one launch per 4096 epochs, state in
 * registers across the launch.  Asynchronous on the handle's stream (the
 * getters and uwvk_vel_synchronize wait). */
uwvk_status uwvk_vel_run_log(uwvk_vel* h, const uwvk_vel_log* log, int64_t first, int64_t count);

/* ---- VelocityUKF in a run, screened and with records --------------------- */
/* HOST mirror of the log's device index arrays (required): what lets the call
 * check flags and row indices before it queues anything.  It must equal the
 * device arrays; the kernels read the device ones. */
typedef struct uwvk_vel_log_host {
  const uint32_t* flags;                /* HOST [log->epochs], must equal log->flags */
  const int32_t*  dvl_index;            /* HOST [epochs] (NULL if UWVK_EV_DVL never set) */
  int64_t         n_dvl;                /* rows of log->dvl */
  const int32_t*  pressure_index;       /* HOST [epochs] (NULL if UWVK_EV_PRESSURE never set) */
  int64_t         n_pressure;           /* rows of log->pressure */
} uwvk_vel_log_host;

typedef struct uwvk_vel_track {
  int64_t every, capacity;              /* as uwvk_pose_track / uwvk_bottom_track: a record after each absolute
                                           epoch e with (e + 1) % every == 0; capacity in records */
  double* mean;                         /* DEVICE [records][batch][4]   nullable */
  double* variance;                     /* DEVICE [records][batch][4]   diag(Sigma), nullable */
  double* model;                        /* DEVICE [records][batch][13]  layout of uwvk_vel_get_model_state, nullable */
} uwvk_vel_track;

/* host only, no device needed: the checks uwvk_vel_run_log_track makes before
 * it queues anything, over epochs [first, first + count).
 * UWVK_EINVAL: log or host NULL; a negative range or one past log->epochs; dt
 * not finite or not > 0; host->flags, log->flags, gyro or efforts NULL while
 * count > 0; a host flag bit other than UWVK_EV_DVL | UWVK_EV_PRESSURE; a
 * flagged kind whose host index, device index or payload pointer is NULL; a
 * host index outside [0, n_kind) at a flagged epoch of the range.
 * UWVK_ENAN: a non-finite dvl_cov or pressure_cov that a flagged epoch of the
 * range uses. */
uwvk_status uwvk_vel_log_check(const uwvk_vel_log* log, const uwvk_vel_log_host* host,
                               int64_t first, int64_t count);

/* Epochs [first, first + count) of the log, each as uwvk_vel_run_log runs it
 * (gyro, efforts, predict, DVL, pressure), on the layout UWVK_VEL_OPT_LANE_GROUPS
 * selects for that call, one launch per 4096 epochs, asynchronous on the
 * handle's stream.  A record of every instance (any of mean, diag(Sigma), the
 * motion-model state) is written after all updates of each record epoch, by the
 * epoch kernel from the state it holds: a record does not end a launch.  Record
 * r of the call is the r-th record epoch inside the range, so the records of
 * calls over adjacent ranges concatenate to those of one call.
 *
 * For an instance whose samples are all finite, (x, P), the motion-model state,
 * the status word and the handle's stored gyro / efforts are bitwise those of
 * uwvk_vel_run_log on the same layout over the same range, and every record is
 * bitwise uwvk_vel_get_state / uwvk_vel_get_model_state with that run cut
 * after the record's epoch.  count == 0 changes nothing.
 *
 * Screening, per instance (the others stay bitwise as beside a clean log):
 *  - a non-finite DVL or pressure sample: that update is skipped for that
 *    instance (the single call with the instance masked out), UWVK_ST_NAN;
 *  - a non-finite gyro or efforts component at an epoch: the instance skips
 *    that epoch's predict (filter, side motion model and its rate keep what
 *    they had), UWVK_ST_NAN; the epoch's updates still run.  The gyro / efforts
 *    the call leaves in the handle are those of the instance's last epoch with
 *    finite inputs (none: unchanged);
 *  - UWVK_ST_NOTPD as in uwvk_vel_run_log: the step is not skipped.
 * applied (DEVICE [batch][2], nullable, zeroed by the caller): the DVL and
 * pressure updates not skipped for the instance are added to it.
 *
 * Returns uwvk_vel_log_check's result first, then UWVK_EINVAL for a track with
 * every <= 0, all three buffers NULL or capacity < uwvk_pose_track_records(
 * first, count, every), then UWVK_ENOMODEL before uwvk_vel_setup_motion_model,
 * all with nothing queued and the state untouched. */
uwvk_status uwvk_vel_run_log_track(uwvk_vel* h, const uwvk_vel_log* log, const uwvk_vel_log_host* host,
                                   int64_t first, int64_t count,
                                   uint32_t* applied /* DEVICE [batch][2] DVL, pressure; nullable, caller zeroes */,
                                   const uwvk_vel_track* track /* nullable */);
/* UWVK_VEL_OPT_LANE_GROUPS: -1 (default) auto by batch size, 0 one filter per
 * lane (9 sigma points in one lane's registers), 1 one filter per 16-lane DPP
 * row (one sigma point per lane; fills the chip at small batches, e.g. C2's 4096);
 * 2 (diagnostic, r05) the 16-lane kernel with each filter duplicated in a second
 * row that stores nothing: twice the waves, the same per-wave work. */
#define UWVK_VEL_OPT_LANE_GROUPS 1
uwvk_status uwvk_vel_set_option(uwvk_vel* h, int option, int value);
/* setProcessNoiseCovariance [EXT pose_estimation base]: 4x4, shared by the
 * batch (default: VelocityUKF.cpp:54-55, velocity diag 1e-4); predict adds dt * Q. */
uwvk_status uwvk_vel_set_process_noise(uwvk_vel* h, const double Q[16]);
uwvk_status uwvk_vel_synchronize(uwvk_vel* h);
/* HIP events on the handle's stream around queued work (bench timing) */
uwvk_status uwvk_vel_timer_start(uwvk_vel* h);
uwvk_status uwvk_vel_timer_stop(uwvk_vel* h, float* elapsed_ms);

/* ======================================================================== */
/* BottomUKF (src/BottomUKF.hpp:26-53, BottomUKF.cpp:1-71)                  */
/* State {distance, normal}: 3 DOF, stored as 4 scalars {d, nx, ny, nz}      */
/* (the normal is an MTK::S2 unit vector).             */
/* ======================================================================== */
#define UWVK_BOTTOM_DOF 3
typedef struct uwvk_bottom uwvk_bottom;
uwvk_status uwvk_bottom_create(int64_t batch, int device, uwvk_bottom** out);
void uwvk_bottom_destroy(uwvk_bottom* h);
void* uwvk_bottom_stream(const uwvk_bottom* h);
/* BottomUKF(initial_state, state_cov) (BottomUKF.cpp:40-46): x batch*4 (normal
 * normalised here, as MTK::S2 does), P batch*9; process noise = identity. */
uwvk_status uwvk_bottom_init(uwvk_bottom* h, const double* x, const double* P);
/* setProcessNoiseCovariance [EXT base]: 3x3, shared by the batch */
uwvk_status uwvk_bottom_set_process_noise(uwvk_bottom* h, const double Q[9]);
/* setVelocity (BottomUKF.cpp:69-72): batch*3 */
uwvk_status uwvk_bottom_set_velocity(uwvk_bottom* h, const double* velocity);
/* predictionStep -> predictionStepImpl (BottomUKF.cpp:48-54) */
uwvk_status uwvk_bottom_predict(uwvk_bottom* h, double dt);
/* integrateMeasurement(RangeMeasurement, unit_direction, origin) (BottomUKF.cpp:56-61):
 * mu batch, cov batch (NULL = shared_cov); beam direction / origin shared. */
uwvk_status uwvk_bottom_update_range(uwvk_bottom* h, const double* mu, const double* cov, double shared_cov,
                                     const double unit_direction[3], const double origin[3], const uint8_t* mask);
/* integrateMeasurement(NormalType, cov) (BottomUKF.cpp:63-67): mu batch*3 (normalised),
 * cov batch*4 (NULL = shared_cov[4]).  A non-finite mean or covariance of a
 * masked-in instance fails the call with UWVK_ENAN, a zero-length mean with
 * UWVK_EINVAL; both change nothing. */
uwvk_status uwvk_bottom_update_normal(uwvk_bottom* h, const double* mu, const double* cov, const double* shared_cov,
                                      const uint8_t* mask);
uwvk_status uwvk_bottom_get_state(uwvk_bottom* h, double* x, double* P);
uwvk_status uwvk_bottom_get_status(uwvk_bottom* h, uint32_t* status, int clear);

/* ---- BottomUKF in a run: a device-resident multi-epoch log --------------- */
/* One epoch is one DVL ping: setVelocity, predictionStep(dt), the range
 * updates of the beams that have a range, then the normal update if there is
 * one.  One launch covers up to 4096 epochs with (mu, Sigma) resident in LDS. */
#define UWVK_BOTTOM_MAX_BEAMS 8
#define UWVK_BEV_BEAM(b)  (1u << (b))   /* b < beams: beam b has a range this epoch */
#define UWVK_BEV_NORMAL   0x100u        /* a normal measurement this epoch */

typedef struct uwvk_bottom_log {
  int64_t epochs;
  double dt;                       /* predict step (host value), > 0 */
  const uint32_t* flags;           /* HOST [epochs] UWVK_BEV_* */
  const double* velocity;          /* DEVICE [epochs][batch][3] (setVelocity of that epoch) */
  int32_t beams;                   /* 0..UWVK_BOTTOM_MAX_BEAMS */
  double beam_direction[UWVK_BOTTOM_MAX_BEAMS][3];  /* host, shared; unit_direction of beam b */
  double beam_origin[UWVK_BOTTOM_MAX_BEAMS][3];     /* host, shared */
  const int32_t* range_index;      /* HOST [epochs]: row into range where any beam bit is set */
  const double* range;             /* DEVICE [n_range][beams][batch] */
  const double* range_var;         /* DEVICE [n_range][beams][batch], NULL = range_cov for all */
  int64_t n_range;
  double range_cov;                /* host, shared */
  const int32_t* normal_index;     /* HOST [epochs] */
  const double* normal;            /* DEVICE [n_normal][batch][3], normalised by the filter */
  int64_t n_normal;
  double normal_cov[4];            /* host, shared */
} uwvk_bottom_log;

typedef struct uwvk_bottom_track {
  int64_t every, capacity;         /* as uwvk_pose_track: a record after each absolute epoch e
                                      with (e + 1) % every == 0; capacity in records */
  double* mean;                    /* DEVICE [records][batch][4], nullable */
  double* variance;                /* DEVICE [records][batch][3] diagonal of Sigma, nullable */
} uwvk_bottom_track;

/* host only, no device needed: the checks uwvk_bottom_run_log makes before it
 * queues anything, over epochs [first, first + count).
 * UWVK_EINVAL: log NULL; a negative range or one past log->epochs; dt not > 0;
 * beams outside 0..UWVK_BOTTOM_MAX_BEAMS; a flag bit that is neither a beam
 * below `beams` nor UWVK_BEV_NORMAL; flags or velocity NULL while count > 0; a
 * flagged kind whose index or payload pointer is NULL; an index outside
 * [0, n_kind) at a flagged epoch.
 * UWVK_ENAN: a non-finite range_cov (when range_var is NULL), normal_cov, beam
 * direction or beam origin that a flagged epoch of the range uses. */
uwvk_status uwvk_bottom_log_check(const uwvk_bottom_log* log, int64_t first, int64_t count);

/* Epochs [first, first + count) of the log.  Epoch e: velocity[e] becomes the
 * handle's velocity; predict with dt; the range updates of the flagged beams in
 * beam order 0..beams-1 (beam b's direction and origin, range_var if given,
 * else range_cov); the normal update if flagged; a track record if e is a
 * record epoch (numbered as uwvk_pose_track_records numbers them; a record does
 * not end a launch).  Afterwards the handle's velocity is that of the last
 * epoch, as after the single calls; the process noise is the handle's.
 *
 * The result is bitwise that of the single calls on the same handle state in
 * this order: mu, Sigma, the status words, and every record against
 * uwvk_bottom_get_state at that epoch.  Calls over adjacent ranges give bitwise
 * what one call over the whole range gives.
 *
 * The payloads are in device memory, so what the single calls refuse on the
 * host is handled per instance here:
 *  - a non-finite range or variance: that update is skipped for that instance
 *    and beam (the single call with the instance masked out), UWVK_ST_NAN;
 *  - a non-finite or zero-length normal: skipped for that instance, UWVK_ST_NAN;
 *  - a non-finite velocity: that instance skips the epoch's predict,
 *    UWVK_ST_NAN, and its stored velocity keeps its last finite value;
 *  - a step whose Cholesky meets a non-positive pivot (at the sigma spread or
 *    in apply_delta's re-spread): (mu, Sigma) stays exactly as before that
 *    step, UWVK_ST_NOTPD, and the later steps of the run still run on it.
 * applied (DEVICE [batch][2], nullable, zeroed by the caller): the range and
 * normal updates that changed the instance are added to it.
 *
 * Returns uwvk_bottom_log_check's result first, then UWVK_EINVAL for a track
 * with every <= 0, both buffers NULL or capacity < uwvk_pose_track_records(
 * first, count, every), all with nothing queued and the state untouched;
 * UWVK_ENOTINIT before uwvk_bottom_init.
 * Asynchronous on the handle's stream like uwvk_vel_run_log: the host arrays
 * are copied before it returns; the getters and uwvk_bottom_synchronize wait. */
uwvk_status uwvk_bottom_run_log(uwvk_bottom* h, const uwvk_bottom_log* log, int64_t first, int64_t count,
                                uint32_t* applied /* DEVICE [batch][2] ranges, normals applied; nullable, caller zeroes */,
                                const uwvk_bottom_track* track /* nullable */);
uwvk_status uwvk_bottom_synchronize(uwvk_bottom* h);

/* ======================================================================== */
/* IndirectPoseUKF (src/IndirectPoseUKF.hpp:28-86, IndirectPoseUKF.cpp:1-147) */
/* State {position_error, orientation_error}: 6 DOF, stored t(3) q(w,x,y,z).  */
/* ======================================================================== */
#define UWVK_IPOSE_DOF 6
typedef struct uwvk_ipose uwvk_ipose;
uwvk_status uwvk_ipose_create(int64_t batch, int device, uwvk_ipose** out);
void uwvk_ipose_destroy(uwvk_ipose* h);
void* uwvk_ipose_stream(const uwvk_ipose* h);
/* UWVK_OPT_SO3_RIGHT only: the side of the orientation_error [+] / [-] (an
 * MTK::SO3, IndirectPoseUKF.hpp:21), 1 (default) body frame q exp(d), 0 nav
 * frame exp(d) q, as uwvk_pose_set_option; the oracle's or_set_so3_right. */
uwvk_status uwvk_ipose_set_option(uwvk_ipose* h, int option, int value);
/* IndirectPoseUKF(position_error_std, orientation_error_std, orientation_error_tau,
 * initial_position_error, initial_position_error_std) (IndirectPoseUKF.cpp:53-78):
 * stds shared; initial_position_error batch*3 (NULL = zero); initial std NULL = ones. */
uwvk_status uwvk_ipose_init(uwvk_ipose* h, const double position_error_std[3], const double orientation_error_std[3],
                            double orientation_error_tau, const double* initial_position_error,
                            const double initial_position_error_std[3]);
/* setProcessNoiseCovariance [EXT pose_estimation base]: 6x6, shared by the
 * batch (uwvk_ipose_init sets diag(position_error_std^2, orientation_error_std^2),
 * IndirectPoseUKF.cpp:72-77); predict shapes it as predictionStepImpl (:80-92). */
uwvk_status uwvk_ipose_set_process_noise(uwvk_ipose* h, const double Q[36]);
/* updatePoseReference (IndirectPoseUKF.cpp:144-147): batch*7 body in world, t(3) q(4) */
uwvk_status uwvk_ipose_set_pose_reference(uwvk_ipose* h, const double* pose);
/* predictionStep -> predictionStepImpl (IndirectPoseUKF.cpp:80-92) */
uwvk_status uwvk_ipose_predict(uwvk_ipose* h, double dt);
/* integrateMeasurement(marker_features, feature_positions, marker_pose, cov_marker_pose,
 * camera_config, camera_in_body) (IndirectPoseUKF.cpp:94-135); arrays as for
 * uwvk_pose_update_visual_landmark. */
uwvk_status uwvk_ipose_update_visual(uwvk_ipose* h, int32_t n_features, const double* features,
                                     const double* feature_cov, int feature_cov_per_instance,
                                     const double* feature_positions, const double* marker_pose,
                                     int marker_pose_per_instance, const double cov_marker_pose[36],
                                     const double camera[4], const double camera_in_body[7], const uint8_t* mask);
/* getCorrectedPose (IndirectPoseUKF.cpp:137-142): pose_ref * pose_error, batch*7 */
uwvk_status uwvk_ipose_get_corrected_pose(uwvk_ipose* h, double* out);
uwvk_status uwvk_ipose_get_state(uwvk_ipose* h, double* x, double* P);
uwvk_status uwvk_ipose_get_status(uwvk_ipose* h, uint32_t* status, int clear);

/* ---- IndirectPoseUKF in a run: a device-resident multi-epoch log --------- */
/* One epoch is updatePoseReference, predictionStep(dt), then zero or more
 * marker observations (integrateMeasurement), in this order.  One launch covers
 * up to 4096 epochs with (mu, Sigma) resident in LDS. */
typedef struct uwvk_ipose_log {
  int64_t epochs;
  double dt;                       /* predict step (host value), > 0; unused if dt_epoch is given */
  const double* dt_epoch;          /* HOST [epochs] predict step of each epoch, each > 0; NULL = dt for all */
  const double* pose_ref;          /* DEVICE [epochs][batch][7] (updatePoseReference of that epoch);
                                      NULL = the handle's reference stays what it is */
  const int64_t* visual_offset;    /* HOST [epochs + 1], non-decreasing (CSR): epoch e integrates the visual
                                      rows visual_offset[e] .. visual_offset[e+1]-1 in that order;
                                      NULL only if n_visual == 0 */
  int64_t n_visual;                /* visual rows */
  int32_t n_features;              /* features of every row, >= 1 if a row is used */
  const double* features;          /* DEVICE [n_visual][batch][n_features][2] */
  const double* feature_cov;       /* DEVICE [n_visual][batch][n_features][4], NULL = shared_feature_cov */
  const double* shared_feature_cov;/* HOST [n_features][4], serves every row */
  const double* feature_positions; /* HOST [n_features][3] */
  const double* marker_pose;       /* DEVICE [n_visual][batch][7], NULL = shared_marker_pose */
  const double* shared_marker_pose;/* HOST [n_visual][7], one per row */
  double cov_marker_pose[36];      /* host, shared */
  double camera[4];                /* host, shared: fx, fy, cx, cy */
  double camera_in_body[7];        /* host, shared */
} uwvk_ipose_log;

typedef struct uwvk_ipose_track {
  int64_t every, capacity;         /* as uwvk_bottom_track */
  double* mean;                    /* DEVICE [records][batch][7], nullable */
  double* variance;                /* DEVICE [records][batch][6] diagonal of Sigma, nullable */
  double* corrected;               /* DEVICE [records][batch][7] pose_ref * pose_error at that epoch, in
                                      uwvk_ipose_get_corrected_pose's layout, nullable */
} uwvk_ipose_track;

/* host only, no device needed: the checks uwvk_ipose_run_log makes before it
 * queues anything, over epochs [first, first + count) and their visual rows.
 * UWVK_EINVAL: log NULL; a negative range or one past log->epochs; n_visual < 0,
 * or visual_offset NULL while n_visual != 0; the predict step of an epoch of
 * the range (dt_epoch's entry, or dt if dt_epoch is NULL) not > 0, a NaN
 * included; a visual_offset entry of the range that is negative, above n_visual
 * or below its predecessor; and, if the range holds a visual row: n_features
 * < 1; features or feature_positions NULL; feature_cov and shared_feature_cov
 * both NULL; marker_pose and shared_marker_pose both NULL.
 * UWVK_ENAN: a non-finite value among the host inputs the range uses: the
 * predict steps and, if it holds a visual row, shared_feature_cov (when
 * feature_cov is NULL), feature_positions, the range's rows of
 * shared_marker_pose (when marker_pose is NULL), cov_marker_pose, camera,
 * camera_in_body. */
uwvk_status uwvk_ipose_log_check(const uwvk_ipose_log* log, int64_t first, int64_t count);

/* Epochs [first, first + count) of the log.  Epoch e: pose_ref[e] becomes the
 * handle's reference; predict with that epoch's step; one visual update per row
 * of the epoch, in row order; a track record if e is a record epoch (numbered
 * as uwvk_pose_track_records numbers them; a record does not end a launch).
 * The handle's UWVK_OPT_SO3_RIGHT, process noise and tau apply.  Afterwards the
 * handle's pose reference is that of the last epoch (per instance: its last
 * finite one), as after the single calls.
 *
 * The result is bitwise that of the single calls on the same handle state in
 * this order (uwvk_ipose_set_pose_reference, uwvk_ipose_predict, one
 * uwvk_ipose_update_visual per row): mu, Sigma, the status words, and every
 * mean / variance record against uwvk_ipose_get_state at that epoch.  Calls
 * over adjacent ranges give bitwise what one call over the whole range gives.
 * The corrected records are computed on the device and agree with
 * uwvk_ipose_get_corrected_pose (host arithmetic) to rounding, not bitwise.
 *
 * The payloads are in device memory, so what the single calls refuse on the
 * host is handled per instance here:
 *  - a non-finite feature, feature covariance or per-instance marker pose of an
 *    instance at a row: that row is skipped for that instance (the single call
 *    with the instance masked out), UWVK_ST_NAN;
 *  - a non-finite pose_ref of an instance at an epoch: the instance keeps its
 *    last finite reference (so does the handle's stored one), UWVK_ST_NAN; its
 *    predict still runs, which does not read the reference;
 *  - a predict whose Cholesky meets a non-positive pivot: (mu, Sigma) stays as
 *    before it, UWVK_ST_NOTPD, and the run carries on;
 *  - a visual row in which any feature's update fails (at the sigma spread or
 *    in apply_delta's re-spread) is discarded for that instance as a whole, as
 *    by uwvk_ipose_update_visual: (mu, Sigma) as before the row,
 *    UWVK_ST_NOTPD, later rows and epochs still run.
 * applied (DEVICE [batch], nullable, zeroed by the caller): the visual rows
 * that changed the instance are added to it.
 *
 * Returns uwvk_ipose_log_check's result first, then UWVK_EINVAL for a track
 * with every <= 0, all three buffers NULL or capacity <
 * uwvk_pose_track_records(first, count, every), then UWVK_ENOTINIT before
 * uwvk_ipose_init, all with nothing queued and the state untouched.
 * Asynchronous on the handle's stream like uwvk_bottom_run_log: the host arrays
 * are copied before it returns; the getters and uwvk_ipose_synchronize wait. */
uwvk_status uwvk_ipose_run_log(uwvk_ipose* h, const uwvk_ipose_log* log, int64_t first, int64_t count,
                               uint32_t* applied /* DEVICE [batch] visual rows applied; nullable, caller zeroes */,
                               const uwvk_ipose_track* track /* nullable */);
uwvk_status uwvk_ipose_synchronize(uwvk_ipose* h);

#ifdef __cplusplus
}
#endif
#endif /* UWVK_H_ */
