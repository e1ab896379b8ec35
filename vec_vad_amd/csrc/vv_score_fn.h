// The z-normalised, weighted score of a cube (test.py:338-348): THE one place the expression lives.  vv_score.hip (vv_frame_scores,
// vv_cube_scores, vv_error_zmaps and what is painted from them) and vv_stream.hip (vv_stream_scores) include it, so a box scored on
// the stream and a cube scored on the batch route agree to the bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Products and sums are rounded separately like numpy's: no FMA contraction from here to the end of the translation unit.
#pragma clang fp contract(off)

namespace vv_score_fn {

// cube m against one row st = (mu_r, sd_r, mu_o, sd_o) of training statistics, float64 like numpy's (float32 error - float64 mean) /
// float64 std; of == nullptr drops the flow term
__device__ __forceinline__ double cube_score_row(const float* __restrict__ raw, const float* __restrict__ of,
                                                 const double* __restrict__ st, double w_raw, double w_of, int m) {
  double sc = w_raw * (((double)raw[m] - st[0]) / st[1]);
  if (of) sc = sc + w_of * (((double)of[m] - st[2]) / st[3]);
  return sc;
}

__device__ __forceinline__ double cube_score(const float* __restrict__ raw, const float* __restrict__ of,
                                             const int32_t* __restrict__ cube_stat, const double* __restrict__ stats,
                                             double w_raw, double w_of, double big, int m) {
  const int s = cube_stat[m];
  if (s < 0) return big;                            // no model for this block: anomaly by construction (test.py:346-348)
  return cube_score_row(raw, of, stats + 4 * (int64_t)s, w_raw, w_of, m);
}

}  // namespace vv_score_fn
