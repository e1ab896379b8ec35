// Several cameras in one scorer (vec_vad_amd/multistream.py): vv_stream_cut and vv_stream_scores (vv_stream.hip) over a camera dimension,
// so that a tick of `cams` cameras is ONE launch of each instead of `cams`.  Camera k's frames live in slots k*R .. k*R+R-1 of one raw
// ring and its fields in slots k*Rf .. of one flow ring; its boxes go to slots k*cap .. k*cap+cap-1 of one store, which a scoring
// launch then covers whole.  Every per-camera quantity (box count, crops, window slots, masks) is read from device tables, so the launch
// arguments do not change from tick to tick.  The arithmetic is that of the single-camera kernels through the same shared headers:
// the same bytes, energies and scores, bit for bit.  Small and latency-bound, like their counterparts: the point is the launch count.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

#include "vv_resize.h"        // resize_pixel / crop_ok / box_energy, shared with vv_extract.hip and vv_stream.hip; FMA contraction off
#include "vv_score_fn.h"      // cube_score_row, shared with vv_score.hip and vv_stream.hip

namespace {

using namespace vv_resize;
using namespace vv_score_fn;

// One workgroup per (camera k, slot b) = store slot k*cap + b; slots at or above n[k] leave at once and write nothing.  The body is
// stream_cut_kernel's with the camera's tables: the flow cube is stored by the loop that sums its squares, then the raw cube is cut.
// The window tables hold absolute ring slots, clamped into the whole ring.
__global__ void __launch_bounds__(256) stream_cut_multi_kernel(const uint8_t* __restrict__ raw_ring, int R_all,
                                                               const float* __restrict__ flow_ring, int Rf_all, int H, int W, int C,
                                                               const int32_t* __restrict__ n_ptr, const int32_t* __restrict__ crops,
                                                               const int32_t* __restrict__ raw_win, const int32_t* __restrict__ flow_win,
                                                               int cap, int T, int Tf, int P, double thr,
                                                               uint8_t* __restrict__ raw_store, float* __restrict__ flow_store,
                                                               uint8_t* __restrict__ keep, double* __restrict__ energy) {
  __shared__ double part[256];
  const int b = blockIdx.x, k = blockIdx.y;
  const int n = min(max(n_ptr[k], 0), cap);
  if (b >= n) return;                                    // the same for every thread of the workgroup
  const int64_t s = (int64_t)k * cap + b;                // the store slot
  const int32_t* crop = crops + 4 * s;
  const int x_min = crop[0], y_min = crop[1], x_max = crop[2], y_max = crop[3];
  if (!crop_ok(x_min, y_min, x_max, y_max, H, W)) {      // a wrong table: the box is dropped, nothing is read
    if (threadIdx.x == 0) {
      keep[s] = 0;
      if (energy) energy[s] = 0.0;
    }
    return;
  }
  const int64_t per_f = (int64_t)Tf * P * P, per_r = (int64_t)T * P * P;
  const double e = box_energy(flow_ring, Rf_all, H, W, 2, x_min, y_min, x_max, y_max, flow_win + (int64_t)k * Tf, Tf, P, part,
                              flow_store + s * per_f * 2);
  if (threadIdx.x == 0) {
    keep[s] = e > thr ? 1 : 0;
    if (energy) energy[s] = e;
  }
  const int32_t* win = raw_win + (int64_t)k * T;
  for (int j = threadIdx.x; j < (int)per_r; j += 256) {
    const int dx = j % P, dy = (j / P) % P, t = j / (P * P);
    const int f = min(max(win[t], 0), R_all - 1);
    const uint8_t* src = raw_ring + (((int64_t)f * H + y_min) * W + x_min) * C;
    uint8_t* dst = raw_store + (s * per_r + j) * C;
    resize_pixel(src, (int64_t)W * C, C, x_max - x_min, y_max - y_min, P, P, dy, dx, [dst](int c, uint8_t v) { dst[c] = v; });
  }
}

// One workgroup per camera k, over slots k*cap .. of the scoring launch.  Per camera the rule is stream_scores_kernel's: box b counts
// iff b < n[k], keep and mask; only then is its error read.  A camera with n[k] = 0 reads and writes nothing but its own cell, which
// keeps its value (fmax with -inf).  Cameras write disjoint rows and cells: no atomics.
__global__ void __launch_bounds__(256) stream_scores_multi_kernel(const float* __restrict__ raw, const float* __restrict__ of,
                                                                  const double* __restrict__ stats, double w_raw, double w_of,
                                                                  double big, const uint8_t* __restrict__ keep,
                                                                  const int32_t* __restrict__ n_ptr, const uint8_t* __restrict__ mask,
                                                                  int cap, double* __restrict__ box_scores, int64_t box_stride,
                                                                  double* __restrict__ frame_score, int64_t frame_stride) {
  __shared__ double part[256];
  const int k = blockIdx.x;
  const int n = min(max(n_ptr[k], 0), cap);
  if (n == 0) return;                                    // the same for every thread: the camera's cell stays as it was
  const int base = k * cap;                              // fits: the entry point refuses cams * cap > INT32_MAX
  double* row = box_scores + (int64_t)k * box_stride;
  double best = -INFINITY;
  for (int b = threadIdx.x; b < n; b += 256) {
    double s = -big;
    if (keep[base + b] && mask[base + b]) {
      s = stats ? cube_score_row(raw, of, stats, w_raw, w_of, base + b) : big;
      best = fmax(best, s);
    }
    row[b] = s;
  }
  part[threadIdx.x] = best;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = fmax(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double* cell = frame_score + (int64_t)k * frame_stride;
    cell[0] = fmax(cell[0], part[0]);
  }
}

}  // namespace

extern "C" int vv_stream_cut_multi(const uint8_t* raw_ring, int32_t R, const float* flow_ring, int32_t Rf, int32_t H, int32_t W,
                                   int32_t C, int32_t cams, const int32_t* n, const int32_t* crops, const int32_t* raw_win,
                                   const int32_t* flow_win, int32_t cap, int32_t T, int32_t Tf, int32_t P, double thr,
                                   uint8_t* raw_store, float* flow_store, uint8_t* keep, double* energy, vv_stream stream) {
  if (cams <= 0 || cams > 65535) return VV_ERR_BAD_ARG;                                 // a camera is a row of the launch grid
  if (R <= 0 || Rf <= 0 || H <= 0 || W <= 0 || C <= 0 || cap < 0 || T <= 0 || Tf <= 0 || P <= 0 || P > 1024) return VV_ERR_BAD_ARG;
  if ((int64_t)T * P * P > 0x7fffffff || (int64_t)Tf * P * P > 0x7fffffff) return VV_ERR_BAD_ARG;      // a box's patch is indexed with an int
  if ((int64_t)cams * R > 0x7fffffff || (int64_t)cams * Rf > 0x7fffffff || (int64_t)cams * cap > 0x7fffffff) return VV_ERR_BAD_ARG;
  if (cap == 0) return VV_OK;
  if (!raw_ring || !flow_ring || !n || !crops || !raw_win || !flow_win || !raw_store || !flow_store || !keep) return VV_ERR_BAD_ARG;
  VV_LAUNCH(stream_cut_multi_kernel, dim3((unsigned)cap, (unsigned)cams), dim3(256), 0, (hipStream_t)stream, raw_ring, cams * R,
            flow_ring, cams * Rf, H, W, C, n, crops, raw_win, flow_win, cap, T, Tf, P, thr, raw_store, flow_store, keep, energy);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_stream_scores_multi(const float* raw, const float* of, const double* stats, double w_raw, double w_of, double big,
                                      const uint8_t* keep, const int32_t* n, const uint8_t* mask, int32_t cams, int32_t cap,
                                      double* box_scores, int64_t box_stride, double* frame_score, int64_t frame_stride,
                                      vv_stream stream) {
  if (cams <= 0 || cap < 0 || (int64_t)cams * cap > 0x7fffffff) return VV_ERR_BAD_ARG;
  if (cap == 0) return VV_OK;
  if (box_stride < cap || frame_stride < 1) return VV_ERR_BAD_ARG;                      // the cameras' rows and cells must not overlap
  if (!keep || !n || !mask || !box_scores || !frame_score || (stats && !raw)) return VV_ERR_BAD_ARG;
  VV_LAUNCH(stream_scores_multi_kernel, dim3((unsigned)cams), dim3(256), 0, (hipStream_t)stream, raw, of, stats, w_raw, w_of, big, keep,
            n, mask, cap, box_scores, box_stride, frame_score, frame_stride);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
