// uwvk_pose_visual.hip — PoseUKF::integrateMeasurement(vector<VisualFeatureMeasurement>,
// feature_positions, marker_pose, cov_marker_pose, camera_config, camera_in_IMU)
// (PoseUKF.cpp:613-654) on gfx950.
//
// The reference augments the filter with the marker pose (PoseStateWithMarker,
// PoseUKF.cpp:221-229: n = 53 + 6 = 59 DOF, 119 sigma points), runs one
// S2-valued ukf::update per feature and keeps the leading n x n block.  Here:
// one 128-lane workgroup per instance, one sigma point per lane, the 59 x 59
// augmented Sigma and the deviation matrix in LDS (uwvk_aug_dev.hpp).  This is
// a camera-rate event, not the per-IMU-epoch hot path.
#include "uwvk_aug_dev.hpp"
#include "uwvk_pose_dev.hpp"

namespace uwvk {

namespace {

// SR: the handle's SO3 side (UWVK_OPT_SO3_RIGHT); both SO3 segments follow it
// (MTK has one SO3::boxplus, so the marker orientation takes the filter's side)
template <int DOF, int SR>
using PoseMarkerM = aug::Manifold<aug::Seg<aug::SEG_V, 3>, aug::Seg<SR ? aug::SEG_SO3R : aug::SEG_SO3>,
                                  aug::Seg<aug::SEG_V, DOF - 6>, aug::Seg<aug::SEG_V, 3>,
                                  aug::Seg<SR ? aug::SEG_SO3R : aug::SEG_SO3>>;

template <int DOF, int SR>
__global__ __launch_bounds__((aug::Engine<PoseMarkerM<DOF, SR>>::BLOCK)) void k_pose_visual(PoseBufs b, aug::VisArgs va) {
  using E = aug::Engine<PoseMarkerM<DOF, SR>>;
  static_assert(E::IPB == 1, "one instance per workgroup");
  constexpr int n = DOF, na = E::n, S = Lay<DOF>::store;
  __shared__ double smem[E::words];
  const int64_t inst = blockIdx.x;
  E e;
  e.g = threadIdx.x;
  e.sm = smem;
  e.live = inst < b.batch && (!va.mask || va.mask[inst]);
  if (e.live) {
    // augmented_state_cov: blockdiag(Sigma, cov_marker_pose) (PoseUKF.cpp:624-627)
    for (int i = e.g; i < na * na; i += E::G) {
      const int r = i / na, c = i % na;
      double v = 0.0;
      if (r < n && c < n) v = b.sigma[inst * tri_n<n>() + pidx(r, c)];
      else if (r >= n && c >= n) v = va.cov_marker[(r - n) * 6 + (c - n)];
      e.sm[E::o_sig + i] = v;
    }
    for (int k = e.g; k < E::S; k += E::G)
      e.sm[E::o_mu + k] = k < S ? b.mu[inst * S + k] : va.marker[inst * va.marker_stride + (k - S)];
  }
  __syncthreads();
  const bool ok = aug::visual_loop<E, S, false>(e, va, inst);
  // ukf.reset(new MTK_UKF(mu.filter_state, sigma.block(0, 0, n, n))) (PoseUKF.cpp:652)
  if (e.live && ok) {
    for (int i = e.g; i < tri_n<n>(); i += E::G) {
      int r, c;
      unpack(i, r, c);
      b.sigma[inst * tri_n<n>() + i] = e.sm[E::o_sig + r * na + c];
    }
    for (int k = e.g; k < S; k += E::G) b.mu[inst * S + k] = e.sm[E::o_mu + k];
  }
  if (e.live && !ok && e.g == 0) b.status[inst] |= UWVK_ST_NOTPD;
}

// All visual rows of one epoch (uwvk_pose_run_log_visual, a VISUAL launch): the
// augmented (mu, Sigma) stays in LDS from the first row to the last, so without
// a failure an instance reads its packed Sigma once and writes it once.  Each
// row calls aug::visual_loop, the same function k_pose_visual calls, so both
// kernels compile the same expressions (the note above k_ipose_run,
// uwvk_small.hip): the result is bitwise that of one k_pose_visual launch per
// row.  Between two rows the LDS state is re-formed as a store and a reload
// would leave it: the leading block's lower triangle (what k_pose_visual
// stores) over its upper one (pidx makes the reload symmetric), the marker
// block cov_marker_pose, the cross blocks zero, mu's tail the row's marker pose.
// One instance per workgroup: screening and failure are uniform over the
// block, and every lane takes every barrier (a skipped row runs visual_loop
// with the engine's `live` flag off, which leaves mu and Sigma as they are).
// A row whose update fails has already changed Sigma: the instance reloads the
// state the launch started from and runs the rows again without the failed
// ones (`skip`), which gives, bit for bit, the state before the failed row.
template <int DOF, int SR>
__global__ __launch_bounds__((aug::Engine<PoseMarkerM<DOF, SR>>::BLOCK)) void k_pose_visual_run(PoseBufs b,
                                                                                             aug::VisRunArgs a) {
  using E = aug::Engine<PoseMarkerM<DOF, SR>>;
  static_assert(E::IPB == 1, "one instance per workgroup");
  constexpr int n = DOF, na = E::n, S = Lay<DOF>::store;
  __shared__ double smem[E::words];
  const int64_t inst = blockIdx.x;
  const bool in = inst < b.batch;
  E e;
  e.g = threadIdx.x;
  e.sm = smem;
  uint32_t st = 0, n_applied = 0;
  uint64_t skip = 0;  // rows of this launch that failed for this instance
  for (bool again = true; again;) {  // uniform
    again = false;
    n_applied = 0;
    if (in) {
      for (int i = e.g; i < n * n; i += E::G) {
        const int r = i / n, c = i % n;
        e.sm[E::o_sig + r * na + c] = b.sigma[inst * tri_n<n>() + pidx(r, c)];
      }
      for (int k = e.g; k < S; k += E::G) e.sm[E::o_mu + k] = b.mu[inst * S + k];
    }
    bool formed = true;  // the leading block is as a reload leaves it
    for (int32_t t = 0; t < a.rows; t++) {  // uniform
      const int64_t row = a.row + t;
      aug::VisArgs vr = a.va;
      vr.features = a.va.features + row * b.batch * vr.nf * 2;
      if (vr.fcov_stride) vr.fcov = a.va.fcov + row * b.batch * vr.fcov_stride;
      vr.marker = vr.marker_stride ? a.va.marker + row * b.batch * 7 : a.marker_rows + (row - a.row_base) * 7;
      bool bad = false;
      if (in) {  // what the single call refuses on the host (stage_visual), per instance
        const double* f = vr.features + inst * vr.nf * 2;
        for (int i = e.g; i < vr.nf * 2; i += E::G) bad |= !aug::finite_dev(f[i]);
        if (vr.fcov_stride) {
          const double* c = vr.fcov + inst * vr.fcov_stride;
          for (int i = e.g; i < vr.nf * 4; i += E::G) bad |= !aug::finite_dev(c[i]);
        }
        if (vr.marker_stride && e.g < 7) bad |= !aug::finite_dev(vr.marker[inst * 7 + e.g]);
      }
      bad = __syncthreads_or(bad);  // also: the state of the row before is complete
      if (bad) st |= UWVK_ST_NAN;
      e.live = in && !bad && !((skip >> t) & 1u);
      if (in) {
        // augmented_state_cov: blockdiag(Sigma, cov_marker_pose) (PoseUKF.cpp:624-627)
        for (int i = e.g; i < na * na; i += E::G) {
          const int r = i / na, c = i % na;
          if (r < n && c < n) {
            if (!formed && r < c) e.sm[E::o_sig + i] = e.sm[E::o_sig + c * na + r];
          } else {
            e.sm[E::o_sig + i] = (r >= n && c >= n) ? a.va.cov_marker[(r - n) * 6 + (c - n)] : 0.0;
          }
        }
        for (int k = e.g; k < E::S - S; k += E::G) e.sm[E::o_mu + S + k] = vr.marker[inst * vr.marker_stride + k];
      }
      __syncthreads();
      const bool ok = aug::visual_loop<E, S, false>(e, vr, inst);
      if (e.live && ok) {
        n_applied++;
        formed = false;
      }
      if (e.live && !ok) {  // discard the row: back to the launch's state, then the rows before it again
        st |= UWVK_ST_NOTPD;
        skip |= (uint64_t)1 << t;
        again = true;
        break;
      }
    }
    __syncthreads();
  }
  // ukf.reset(new MTK_UKF(mu.filter_state, sigma.block(0, 0, n, n))) (PoseUKF.cpp:652)
  if (in && n_applied > 0) {
    for (int i = e.g; i < tri_n<n>(); i += E::G) {
      int r, c;
      unpack(i, r, c);
      b.sigma[inst * tri_n<n>() + i] = e.sm[E::o_sig + r * na + c];
    }
    for (int k = e.g; k < S; k += E::G) b.mu[inst * S + k] = e.sm[E::o_mu + k];
  }
  if (in && e.g == 0) {
    if (st) b.status[inst] |= st;
    if (a.applied) a.applied[inst] += n_applied;
  }
}

}  // namespace

template <int SR>
static void launch_pose_visual_sr(int dof, hipStream_t st, const PoseBufs& b, const aug::VisArgs& va) {
  const dim3 g((unsigned)b.batch);
  if (dof == 53)
    hipLaunchKernelGGL((k_pose_visual<53, SR>), g, dim3(aug::Engine<PoseMarkerM<53, SR>>::BLOCK), 0, st, b, va);
  else
    hipLaunchKernelGGL((k_pose_visual<26, SR>), g, dim3(aug::Engine<PoseMarkerM<26, SR>>::BLOCK), 0, st, b, va);
}

hipError_t launch_pose_visual(int dof, int right, hipStream_t st, const PoseBufs& b, const aug::VisArgs& va) {
  if (right) launch_pose_visual_sr<1>(dof, st, b, va);
  else launch_pose_visual_sr<0>(dof, st, b, va);
  return hipGetLastError();
}

template <int SR>
static void launch_pose_visual_run_sr(int dof, hipStream_t st, const PoseBufs& b, const aug::VisRunArgs& a) {
  const dim3 g((unsigned)b.batch);
  if (dof == 53)
    hipLaunchKernelGGL((k_pose_visual_run<53, SR>), g, dim3(aug::Engine<PoseMarkerM<53, SR>>::BLOCK), 0, st, b, a);
  else
    hipLaunchKernelGGL((k_pose_visual_run<26, SR>), g, dim3(aug::Engine<PoseMarkerM<26, SR>>::BLOCK), 0, st, b, a);
}

hipError_t launch_pose_visual_run(int dof, int right, hipStream_t st, const PoseBufs& b, const aug::VisRunArgs& a) {
  if (a.rows < 1 || a.rows > aug::kVisRunRows || a.va.nf < 1) return hipErrorInvalidValue;
  if (right) launch_pose_visual_run_sr<1>(dof, st, b, a);
  else launch_pose_visual_run_sr<0>(dof, st, b, a);
  return hipGetLastError();
}

}  // namespace uwvk
