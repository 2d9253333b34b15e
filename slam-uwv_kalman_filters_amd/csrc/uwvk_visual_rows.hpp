// uwvk_visual_rows.hpp — the one host path of the visual rows of a run call
// (uwvk_pose_run_log_visual, uwvk_ipose_run_log): the checks of the visual
// fields (uwvk_pose_visual_check, uwvk_ipose_log_check) and the staging of the
// rows' shared host inputs into the words of an acquired slot (uwvk_stage.hpp)
// with the aug::VisArgs that point at them.  Host code only.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/uwvk.h"
#include "uwvk_aug_dev.hpp"  // aug::VisArgs
#include "uwvk_dev.hpp"      // finite_all

namespace uwvk {

// One view of the two argument structs, which name the same fields except the
// camera mounting (camera_in_imu / camera_in_body).
struct VisualRows {
  const int64_t* visual_offset;
  int64_t n_visual;
  int32_t n_features;
  const double *features, *feature_cov, *shared_feature_cov, *feature_positions, *marker_pose, *shared_marker_pose,
      *cov_marker_pose, *camera, *camera_in;
  explicit VisualRows(const uwvk_pose_visual& v)
      : visual_offset(v.visual_offset), n_visual(v.n_visual), n_features(v.n_features), features(v.features),
        feature_cov(v.feature_cov), shared_feature_cov(v.shared_feature_cov), feature_positions(v.feature_positions),
        marker_pose(v.marker_pose), shared_marker_pose(v.shared_marker_pose), cov_marker_pose(v.cov_marker_pose),
        camera(v.camera), camera_in(v.camera_in_imu) {}
  explicit VisualRows(const uwvk_ipose_log& l)
      : visual_offset(l.visual_offset), n_visual(l.n_visual), n_features(l.n_features), features(l.features),
        feature_cov(l.feature_cov), shared_feature_cov(l.shared_feature_cov), feature_positions(l.feature_positions),
        marker_pose(l.marker_pose), shared_marker_pose(l.shared_marker_pose), cov_marker_pose(l.cov_marker_pose),
        camera(l.camera), camera_in(l.camera_in_body) {}
};

// The UWVK_EINVAL rules of the visual fields over epochs [first, first + count)
// (a valid range of the log): the offsets of the range and, if it holds a row,
// the arrays a row needs.  *row0 .. *row1 are the range's rows.
inline bool visual_rows_valid(const VisualRows& v, int64_t first, int64_t count, int64_t* row0, int64_t* row1) {
  *row0 = *row1 = 0;
  if (v.visual_offset) {
    for (int64_t e = first; e <= first + count; e++) {
      const int64_t o = v.visual_offset[e];
      if (o < 0 || o > v.n_visual || (e > first && o < v.visual_offset[e - 1])) return false;
    }
    *row0 = v.visual_offset[first];
    *row1 = v.visual_offset[first + count];
  }
  if (*row1 <= *row0) return true;
  if (v.n_features < 1 || !v.features || !v.feature_positions) return false;
  return (v.feature_cov || v.shared_feature_cov) && (v.marker_pose || v.shared_marker_pose);
}

// The UWVK_ENAN rule of rows [row0, row1), row1 > row0: the shared host values
// they use are finite (checkMeasurment of the single call)
inline bool visual_rows_finite(const VisualRows& v, int64_t row0, int64_t row1) {
  const size_t nf = (size_t)v.n_features;
  if (!v.feature_cov && !finite_all(v.shared_feature_cov, nf * 4)) return false;
  if (!finite_all(v.feature_positions, nf * 3)) return false;
  if (!v.marker_pose && !finite_all(v.shared_marker_pose + row0 * 7, (size_t)(row1 - row0) * 7)) return false;
  return finite_all(v.cov_marker_pose, 36) && finite_all(v.camera, 4) && finite_all(v.camera_in, 7);
}

// the 8-byte words visual_rows_stage writes for `rows` rows
inline size_t visual_rows_words(const VisualRows& v, int64_t rows) {
  if (rows <= 0) return 0;
  const size_t nf = (size_t)v.n_features;
  return nf * 3 + (v.feature_cov ? 0 : nf * 4) + (v.marker_pose ? 0 : (size_t)rows * 7);
}

// Writes the shared host inputs of rows [row0, row0 + rows) into an acquired
// slot's words hw (device address dw): the feature positions, the shared
// feature covariance and the rows' shared marker poses, each only if used;
// fills *va for them and *marker_rows (device, NULL = per instance).  Returns
// visual_rows_words: the caller queues the one copy of its slot.  rows == 0
// writes nothing and leaves *va as it is.
inline size_t visual_rows_stage(const VisualRows& v, int64_t row0, int64_t rows, double* hw, const double* dw,
                                aug::VisArgs* va, const double** marker_rows) {
  *marker_rows = nullptr;
  if (rows <= 0) return 0;
  const size_t nf = (size_t)v.n_features;
  const size_t w_pos = nf * 3, w_cov = v.feature_cov ? 0 : nf * 4, w_mk = v.marker_pose ? 0 : (size_t)rows * 7;
  std::memcpy(hw, v.feature_positions, w_pos * 8);
  if (w_cov) std::memcpy(hw + w_pos, v.shared_feature_cov, w_cov * 8);
  if (w_mk) std::memcpy(hw + w_pos + w_cov, v.shared_marker_pose + row0 * 7, w_mk * 8);
  va->nf = v.n_features;
  va->features = v.features;
  va->fcov = v.feature_cov ? v.feature_cov : dw + w_pos;
  va->fcov_stride = v.feature_cov ? (int64_t)nf * 4 : 0;
  va->fpos = dw;
  va->marker = v.marker_pose;
  va->marker_stride = v.marker_pose ? 7 : 0;
  std::memcpy(va->cov_marker, v.cov_marker_pose, sizeof(va->cov_marker));
  std::memcpy(va->cam, v.camera, sizeof(va->cam));
  std::memcpy(va->cam_in, v.camera_in, sizeof(va->cam_in));
  if (w_mk) *marker_rows = dw + w_pos + w_cov;
  return w_pos + w_cov + w_mk;
}

}  // namespace uwvk
