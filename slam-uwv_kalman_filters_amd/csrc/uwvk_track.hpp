// uwvk_track.hpp — the snapshot kernel of uwvk_pose_run_log_track (uwvk_track.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uwvk {

// One record of all instances, from the state the last launch stored to HBM:
// mean [batch][store] = mu, variance [batch][dof] = the diagonal of the packed
// lower triangle sigma.  Either output may be null (not both).
hipError_t launch_pose_track(int dof, hipStream_t st, const double* mu, const double* sigma, int64_t batch,
                             double* mean, double* variance);

// counts[i][kind] += accepted[i] != 0 (the literal path's fix accept counts, [batch][3])
hipError_t launch_fix_count(hipStream_t st, const uint8_t* accepted, int64_t batch, int kind, uint32_t* counts);
// counts[i] += accepted[i] != 0 (the literal path's delayed XY accept counts, [batch])
hipError_t launch_delayed_count(hipStream_t st, const uint8_t* accepted, int64_t batch, uint32_t* counts);

// The position latch of uwvk_pose_run_log_delayed (k_pose_latch): mu's XY
// position of all instances into rows.row[0 .. rows.n) of latched
// ([rows][batch][2]).  Rows that share a latch epoch go in one launch, up to
// kLatchRows; the caller has range-checked the row numbers against the buffer.
constexpr int kLatchRows = 8;
struct LatchRows {
  int32_t row[kLatchRows];
  int n;
};
hipError_t launch_pose_latch(int dof, hipStream_t st, const double* mu, int64_t batch, double* latched,
                             const LatchRows& rows);

}  // namespace uwvk
