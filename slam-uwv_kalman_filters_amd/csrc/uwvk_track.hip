// uwvk_track.hip — the track recorder's snapshot kernel (uwvk_pose_run_log_track).
//
// A record is taken between two launches of run_log, from what the launch
// before it stored to HBM: PoseBufs::mu ([batch][store]) and the packed lower
// triangle PoseBufs::sigma ([batch][dof (dof + 1) / 2]), the arrays
// uwvk_pose_get_state reads.  One pass over flat element indices writes both
// outputs: element i of the record's mean row is mu's element i (both sides
// coalesced), and element i = b dof + d of its variance row is instance b's
// packed entry d (d + 3) / 2, a strided gather on the read side (one 64-B
// sector per entry) with consecutive lanes writing consecutive doubles.  No
// LDS, no atomics, a handful of registers.
#include "uwvk_dev.hpp"
#include "uwvk_track.hpp"

namespace uwvk {

constexpr int kTrackThreads = 256;

template <int DOF>
__global__ __launch_bounds__(kTrackThreads) void k_pose_track(const double* __restrict__ mu,
                                                              const double* __restrict__ sigma, int64_t batch,
                                                              double* __restrict__ mean,
                                                              double* __restrict__ variance) {
  const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (mean && i < batch * Lay<DOF>::store) mean[i] = mu[i];
  if (variance && i < batch * DOF) {
    const int64_t b = i / DOF;
    const int d = (int)(i - b * DOF);
    variance[i] = sigma[b * tri_n<DOF>() + d * (d + 3) / 2];
  }
}

hipError_t launch_pose_track(int dof, hipStream_t st, const double* mu, const double* sigma, int64_t batch,
                             double* mean, double* variance) {
  if ((dof != 53 && dof != 26) || batch <= 0 || (!mean && !variance)) return hipErrorInvalidValue;
  // the longer row (store = dof + 1) sizes the grid; a null output costs its lanes nothing
  const int64_t blocks = (batch * (dof + 1) + kTrackThreads - 1) / kTrackThreads;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (dof == 53)
    hipLaunchKernelGGL(k_pose_track<53>, dim3((unsigned)blocks), dim3(kTrackThreads), 0, st, mu, sigma, batch, mean,
                       variance);
  else
    hipLaunchKernelGGL(k_pose_track<26>, dim3((unsigned)blocks), dim3(kTrackThreads), 0, st, mu, sigma, batch, mean,
                       variance);
  return hipGetLastError();
}

// the literal path of uwvk_pose_run_log_fixes: k_pose_update's accepted bytes
// of one fix kind added to the fix accept counts [batch][3]
__global__ __launch_bounds__(kTrackThreads) void k_fix_count(const uint8_t* __restrict__ accepted, int64_t batch,
                                                             int kind, uint32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i < batch) counts[i * 3 + kind] += accepted[i] ? 1u : 0u;
}

hipError_t launch_fix_count(hipStream_t st, const uint8_t* accepted, int64_t batch, int kind, uint32_t* counts) {
  if (!accepted || !counts || batch <= 0 || kind < 0 || kind > 2) return hipErrorInvalidValue;
  const int64_t blocks = (batch + kTrackThreads - 1) / kTrackThreads;
  hipLaunchKernelGGL(k_fix_count, dim3((unsigned)blocks), dim3(kTrackThreads), 0, st, accepted, batch, kind, counts);
  return hipGetLastError();
}

}  // namespace uwvk
