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

// the literal path of uwvk_pose_run_log_fixes / _delayed: k_pose_update's
// accepted bytes of one fix kind added to accept counts [batch][width]
__global__ __launch_bounds__(kTrackThreads) void k_fix_count(const uint8_t* __restrict__ accepted, int64_t batch,
                                                             int width, int kind, uint32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i < batch) counts[i * width + kind] += accepted[i] ? 1u : 0u;
}

static hipError_t launch_count(hipStream_t st, const uint8_t* accepted, int64_t batch, int width, int kind,
                               uint32_t* counts) {
  if (!accepted || !counts || batch <= 0 || kind < 0 || kind >= width) return hipErrorInvalidValue;
  const int64_t blocks = (batch + kTrackThreads - 1) / kTrackThreads;
  hipLaunchKernelGGL(k_fix_count, dim3((unsigned)blocks), dim3(kTrackThreads), 0, st, accepted, batch, width, kind,
                     counts);
  return hipGetLastError();
}

hipError_t launch_fix_count(hipStream_t st, const uint8_t* accepted, int64_t batch, int kind, uint32_t* counts) {
  return launch_count(st, accepted, batch, 3, kind, counts);
}

hipError_t launch_delayed_count(hipStream_t st, const uint8_t* accepted, int64_t batch, uint32_t* counts) {
  return launch_count(st, accepted, batch, 1, 0, counts);
}

// The position latch of uwvk_pose_run_log_delayed: after all updates of an
// epoch, from the state the launch before it stored, every instance's own XY
// position mu[b store + 0 .. 1] into the rows of `latched` ([n][batch][2]) that
// latch at this epoch.  Lane i handles double i of a row (instance i / 2,
// component i % 2): one read of mu per lane (two of every `store` doubles, a
// strided gather), consecutive lanes writing consecutive doubles of each row.
// The row numbers travel by value (LatchRows); no LDS, no atomics.
template <int DOF>
__global__ __launch_bounds__(kTrackThreads) void k_pose_latch(const double* __restrict__ mu, int64_t batch,
                                                              double* __restrict__ latched, LatchRows rows) {
  const int64_t i = (int64_t)blockIdx.x * kTrackThreads + threadIdx.x;
  if (i >= batch * 2) return;
  const double v = mu[(i >> 1) * Lay<DOF>::store + Lay<DOF>::s_pos + (i & 1)];
  for (int k = 0; k < rows.n; k++) latched[(int64_t)rows.row[k] * batch * 2 + i] = v;
}

hipError_t launch_pose_latch(int dof, hipStream_t st, const double* mu, int64_t batch, double* latched,
                             const LatchRows& rows) {
  if ((dof != 53 && dof != 26) || batch <= 0 || !mu || !latched || rows.n < 1 || rows.n > kLatchRows)
    return hipErrorInvalidValue;
  for (int k = 0; k < rows.n; k++)
    if (rows.row[k] < 0) return hipErrorInvalidValue;
  const int64_t blocks = (batch * 2 + kTrackThreads - 1) / kTrackThreads;
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  if (dof == 53)
    hipLaunchKernelGGL(k_pose_latch<53>, dim3((unsigned)blocks), dim3(kTrackThreads), 0, st, mu, batch, latched, rows);
  else
    hipLaunchKernelGGL(k_pose_latch<26>, dim3((unsigned)blocks), dim3(kTrackThreads), 0, st, mu, batch, latched, rows);
  return hipGetLastError();
}

}  // namespace uwvk
