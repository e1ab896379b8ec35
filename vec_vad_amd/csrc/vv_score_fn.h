// The z-normalised, weighted score of a cube (test.py:338-348): THE one place the expression lives.  vv_score.hip (vv_frame_scores,
// vv_cube_scores, vv_error_zmaps and what is painted from them) and vv_stream.hip (vv_stream_scores, vv_stream_zpaint) include it, so a
// box scored on the stream and a cube scored on the batch route agree to the bit.  zmap_src, the patch pixel a frame pixel of a painted
// rectangle reads, lives here for the same reason (vv_paint_zmaps, vv_stream_zpaint).
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

// ---- per-pixel maps: a cube's 32 x 32 patch of errors scored pixel by pixel (vv_error_zmaps / vv_paint_zmaps, vv_stream_zpaint)
constexpr int ZMAP_PIX = 1024;               // pixels of a patch (32 x 32)
constexpr int ZMAP_SIDE = 32;

// nearest source row / column of a patch stretched over [lo, hi): ((2 (v - lo) + 1) * 32) / (2 (hi - lo)) in integers, 0..31 for
// lo <= v < hi, the identity when hi - lo == 32
__device__ __forceinline__ int zmap_src(int v, int lo, int hi) { return ((2 * (v - lo) + 1) * ZMAP_SIDE) / (2 * (hi - lo)); }

}  // namespace vv_score_fn
