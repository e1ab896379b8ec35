// Frame-by-frame scoring (vec_vad_amd/stream.py): the two launches that stand between a ring of recent frames and a frame score without
// a host decision in between.  vv_stream_cut cuts the raw and the flow cube of every box of ONE frame into fixed store slots and applies
// the motion test; vv_stream_scores turns the error sums of a fixed-size scoring launch into box scores and max-accumulates the frame
// score under a validity mask.  Both read the number of boxes, the crops, the window slots and the masks from device memory, so their
// launch arguments never change from frame to frame (they can sit in a captured graph).  Both are small and latency-bound (5-30 boxes a
// frame): the point is one launch each.  The arithmetic is that of vv_cube_cut / vv_cube_energy / vv_cube_scores, through the shared
// headers: the same bits.  Both kernels have a camera dimension (vec_vad_amd/multistream.py: camera k's frames in slots k*R .. of one raw
// ring, its fields in slots k*Rf .. of one flow ring, its boxes in store slots k*cap ..), so that a tick of `cams` cameras is ONE launch
// of each (vv_stream_cut_multi, vv_stream_scores_multi); the single-camera entry points are that launch at cams = 1.
// vv_stream_boxes is the third: for a scorer that finds its own motion boxes (vv_motion_mask + vv_mask_boxes leave
// them on the device) it forms the crops, the box count and the per-block masks the host forms for boxes it is given.  vv_stream_paint is
// the fourth: the frame's box-score rows painted into its score mask, with the box count and the motion boxes still on the device.
// vv_stream_tracks is the fifth: over the same tables, the frame's boxes linked to the tracks of the frames before, in one workgroup.
// vv_stream_zpaint is the sixth: behind a block's vv_stream_scores, the per-pixel errors of that scoring launch painted into the frame's
// error mask under the same keep flags and mask row -- vv_error_zmaps + vv_paint_zmaps of the batch route, the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

#include "vv_resize.h"        // resize_pixel / crop_ok / box_energy, shared with vv_extract.hip; switches FMA contraction off
#include "vv_score_fn.h"      // cube_score_row, shared with vv_score.hip

namespace {

using namespace vv_resize;
using namespace vv_score_fn;

// One workgroup per (camera k, slot b) = store slot k*cap + b; slots at or above n[k] leave at once and write nothing.  The flow cube is
// stored by the loop that sums its squares (box_energy: the order and the bits of vv_cube_energy), then the raw cube is cut, thread j
// taking pixels j, j + 256, ... of the [T][P][P] patch.  A camera's boxes share its two windows; the window tables hold absolute ring
// slots, clamped into the whole ring.  One camera (vv_stream_cut) is the grid (cap, 1).
__global__ void __launch_bounds__(256) stream_cut_kernel(const uint8_t* __restrict__ raw_ring, int R_all, const float* __restrict__ flow_ring,
                                                         int Rf_all, int H, int W, int C, const int32_t* __restrict__ n_ptr,
                                                         const int32_t* __restrict__ crops, const int32_t* __restrict__ raw_win,
                                                         const int32_t* __restrict__ flow_win, int cap, int T, int Tf, int P, double thr,
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

// One workgroup per camera k, over slots k*cap .. of the scoring launch.  Box b counts iff b < n[k], keep and mask: only then is its
// error read at all, so whatever the padded slots of the scoring launch, a dropped box or a box of another block hold (NaN, Inf) cannot
// reach the maximum.  A counted box gets the score of vv_cube_scores (stats == nullptr: the block has no model, +big), another box below
// n[k] gets -big, slots >= n[k] are not written.  The maximum of the counted scores meets in an LDS tree and is max-accumulated into the
// camera's cell (launches on one stream are ordered, a cell has one writer at a time).  A camera with n[k] = 0 reads and writes nothing:
// its cell keeps its value, as under fmax with -inf.  Cameras write disjoint rows and cells: no atomics.
__global__ void __launch_bounds__(256) stream_scores_kernel(const float* __restrict__ raw, const float* __restrict__ of,
                                                            const double* __restrict__ stats, double w_raw, double w_of, double big,
                                                            const uint8_t* __restrict__ keep, const int32_t* __restrict__ n_ptr,
                                                            const uint8_t* __restrict__ mask, int cap, double* __restrict__ box_scores,
                                                            int64_t box_stride, double* __restrict__ frame_score, int64_t frame_stride) {
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

// Python's slice(a, b).indices(len)[:2] for step 1: a negative bound counts from the end, then both clip to [0, len].
__device__ __forceinline__ int slice_bound(int v, const int len) {
  if (v < 0) v = max(v + len, 0);
  return min(v, len);
}

// int(q) of a cell quotient lies in [0, cells): the truncation towards zero of Python's int(), decided on the double so that no
// out-of-range conversion happens.  Returns the cell or -1.
__device__ __forceinline__ int cell_of(const double q, const int cells) {
  return (q > -1.0 && q < (double)cells) ? (int)q : -1;
}

// One workgroup; thread j takes motion slots n_ap + j, n_ap + j + 256, ... and owns the whole mask column of each, so no two threads
// write one byte.  For the boxes vv_mask_boxes left on the device this is StreamScorer._prepare: boxes_to_crops, box_paints and
// calc_block_idx, the last in float64 in the order utils.py writes it (contraction is off in this file: every operation rounds on its
// own, as in Python).  Slots below n_ap belong to the host's appearance boxes and are not touched.
__global__ void __launch_bounds__(256) stream_boxes_kernel(const int32_t* __restrict__ count_ptr, const int32_t* __restrict__ boxes,
                                                           int mcap, int n_ap, int cap, int H, int W, int grid_h, int grid_w, int hb,
                                                           int wb, double h_step, double w_step, int block_mode,
                                                           int32_t* __restrict__ n_ptr, int32_t* __restrict__ dropped,
                                                           int32_t* __restrict__ crops, uint8_t* __restrict__ masks,
                                                           int32_t* __restrict__ boxes_out) {
  const int count = max(count_ptr[0], 0);
  const int m = min(min(count, mcap), cap - n_ap);
  if (threadIdx.x == 0) {
    n_ptr[0] = n_ap + m;
    dropped[0] = count - m;
  }
  const int npts = block_mode >= 9 ? 9 : (block_mode > 1 ? 5 : 1);
  for (int s = n_ap + (int)threadIdx.x; s < cap; s += 256) {
    const int j = s - n_ap;
    int hi[9], wi[9];
    int used = 0;
    if (j < m) {
      const int x1 = boxes[4 * j + 0], y1 = boxes[4 * j + 1], x2 = boxes[4 * j + 2], y2 = boxes[4 * j + 3];
      boxes_out[4 * s + 0] = x1, boxes_out[4 * s + 1] = y1, boxes_out[4 * s + 2] = x2, boxes_out[4 * s + 3] = y2;
      crops[4 * s + 0] = max(x1, 0), crops[4 * s + 1] = max(y1, 0), crops[4 * s + 2] = min(x2, W), crops[4 * s + 3] = min(y2, H);
      const bool paints = slice_bound(y2, grid_h) > slice_bound(y1, grid_h) && slice_bound(x2, grid_w) > slice_bound(x1, grid_w);
      if (paints) {
        const double x_min = x1, x_max = x2, y_min = y1, y_max = y2;
        const double cy = (y_min + y_max) / 2.0, cx = (x_min + x_max) / 2.0;
        // calc_block_idx's probe points: centre | edge mid-points | corners
        const double py[9] = {cy, y_min, y_max, cy, cy, y_min, y_max, y_max, y_min};
        const double px[9] = {cx, cx, cx, x_min, x_max, x_min, x_max, x_min, x_max};
        for (int p = 0; p < npts; ++p) {
          const int h = cell_of(((py[p] + cy) / 2.0) / h_step, hb), w = cell_of(((px[p] + cx) / 2.0) / w_step, wb);
          if (h >= 0 && w >= 0) hi[used] = h, wi[used] = w, ++used;      // a cell outside the grid gets no bit
        }
      }
    }
    for (int r = 0; r < hb * wb; ++r) {
      uint8_t bit = 0;
      for (int p = 0; p < used; ++p) bit |= (uint8_t)(hi[p] * wb + wi[p] == r);
      masks[(int64_t)r * cap + s] = bit;
    }
  }
}

// ---- the issued frame's score mask (vv_stream_paint) -----------------------------------------------------------------------------------
constexpr int SP_STAGE = VV_STREAM_PAINT_STAGE;      // boxes per LDS pass = threads of the workgroup
constexpr int SP_PIX = 2;                            // consecutive pixels per thread: one 16-byte store
constexpr int SP_TILE = SP_PIX * 256;                // pixels per workgroup
constexpr double SP_BG = VV_STREAM_UNPAINTED;

// vv_paint_masks' layout for ONE frame whose box count lives on the device: a thread owns two consecutive pixels of the flat h*w mask
// and walks the boxes, staged in LDS SP_STAGE at a time (every lane reads the same box: broadcast).  Staging box b, a thread takes the
// maximum of its column of the [rows][width] score rows and its rectangle -- the host's for b < n_host, else Python's slicing of the
// device's box on integers -- so every workgroup forms the same table; workgroup 0 also leaves it in box_max / rects for the overlay.
// Rows >= n_host of rects are read by nobody (their rectangles come from `boxes`), so that write races with no read.  The mask is
// written whole, background included: no fill launch, no atomics.
__global__ void __launch_bounds__(256) stream_paint_kernel(const double* __restrict__ scores, int rows, int width,
                                                           const int32_t* __restrict__ n_ptr, int n_host, int4* rects,
                                                           const int32_t* __restrict__ boxes, int h, int w, double* __restrict__ mask,
                                                           double* __restrict__ box_max, int32_t* __restrict__ frame_off) {
  __shared__ int4 srect[SP_STAGE];
  __shared__ double ssc[SP_STAGE];
  const int n = min(max(n_ptr[0], 0), width);
  const int nh = boxes ? min(max(n_host, 0), n) : n;     // without a box table every rectangle is the host's
  const int hw = h * w;
  const int p0 = (blockIdx.x * 256 + (int)threadIdx.x) * SP_PIX;
  const bool in0 = p0 < hw, in1 = p0 + 1 < hw;
  const int ya = in0 ? p0 / w : -1, xa = in0 ? p0 - ya * w : -1;      // a pixel past the frame lies in no box
  const int yb = in1 ? (p0 + 1) / w : -1, xb = in1 ? p0 + 1 - yb * w : -1;
  double v0 = SP_BG, v1 = SP_BG;
  for (int base = 0; base < n; base += SP_STAGE) {
    const int cnt = min(SP_STAGE, n - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const int b = base + (int)threadIdx.x;
      int4 r;
      if (b < nh) {
        r = rects[b];
      } else {
        const int x1 = boxes[4 * b + 0], y1 = boxes[4 * b + 1], x2 = boxes[4 * b + 2], y2 = boxes[4 * b + 3];
        r = make_int4(slice_bound(y1, h), slice_bound(y2, h), slice_bound(x1, w), slice_bound(x2, w));
      }
      double s = SP_BG;
      for (int i = 0; i < rows; ++i) s = fmax(s, scores[(int64_t)i * width + b]);
      srect[threadIdx.x] = r;
      ssc[threadIdx.x] = s;
      if (blockIdx.x == 0) {
        box_max[b] = s;
        if (b >= nh) rects[b] = r;
      }
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const int4 r = srect[k];                // y0, y1, x0, x1
      const double s = ssc[k];
      if (ya >= r.x && ya < r.y && xa >= r.z && xa < r.w) v0 = fmax(v0, s);
      if (yb >= r.x && yb < r.y && xb >= r.z && xb < r.w) v1 = fmax(v1, s);
    }
  }
  if (in1 && (reinterpret_cast<uintptr_t>(mask + p0) & 15) == 0) {
    *reinterpret_cast<double2*>(mask + p0) = make_double2(v0, v1);
  } else {
    if (in0) mask[p0] = v0;
    if (in1) mask[p0 + 1] = v1;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    frame_off[0] = 0;
    frame_off[1] = n;
  }
}

// ---- the issued frame's per-pixel error mask (vv_stream_zpaint) --------------------------------------------------------------------------
// stream_paint_kernel's layout with the value read from the box's error maps instead of one score per box: vv_error_zmaps and
// vv_paint_zmaps of the batch route in one launch, for ONE block's share of ONE round.  Staging slot b of the round, a thread writes its
// rectangle -- row slot0 + b of the frame's table, the host's below n_host, else Python's slicing of the device's box -- and one flag:
// the slot counts (b < n, keep[b], mask[b]: the rule of stream_scores_kernel) and its rectangle holds a pixel.  Every lane reads the same
// entry (broadcast); the maps of a slot whose flag is 0 are never read, and those of a counted slot only where a pixel lies in its
// rectangle, through L2.  first: the mask is written whole from the background -big; else the launch max-accumulates into what it holds.
// The value of pixel (y, x) inside the rectangle r = (y0, y1, x0, x1) of the slot whose maps start at m0: vv_error_zmaps' expression at
// the patch pixel vv_paint_zmaps reads.  The index is clamped into the patch, so that a rectangle that is no row of scoring.box_rects
// cannot make the kernel read outside the maps.
__device__ __forceinline__ double zpaint_value(const float* __restrict__ e_raw, const float* __restrict__ e_of, const double* st,
                                               const double w_raw, const double w_of, const int64_t m0, const int y, const int x,
                                               const int4 r) {
  const int qy = min(max(zmap_src(y, r.x, r.y), 0), ZMAP_SIDE - 1), qx = min(max(zmap_src(x, r.z, r.w), 0), ZMAP_SIDE - 1);
  const int64_t q = m0 + qy * ZMAP_SIDE + qx;
  const float er = 1024.f * e_raw[q];
  if (!e_of) return cube_score_row(&er, nullptr, st, w_raw, w_of, 0);
  const float eo = 1024.f * e_of[q];
  return cube_score_row(&er, &eo, st, w_raw, w_of, 0);      // two calls, so that neither operand's address is a run-time choice: no scratch
}

__global__ void __launch_bounds__(256) stream_zpaint_kernel(const float* __restrict__ e_raw, const float* __restrict__ e_of,
                                                            const double* __restrict__ stats, double w_raw, double w_of, double big,
                                                            const uint8_t* __restrict__ keep, const uint8_t* __restrict__ mask,
                                                            const int32_t* __restrict__ n_ptr, int cap, int slot0,
                                                            const int32_t* __restrict__ rects, int n_host,
                                                            const int32_t* __restrict__ boxes, int h, int w, double* __restrict__ out,
                                                            int first) {
  __shared__ int4 srect[SP_STAGE];
  __shared__ int sflag[SP_STAGE];
  const int n = min(max(n_ptr[0], 0), cap);
  const int hw = h * w;
  const int p0 = (blockIdx.x * 256 + (int)threadIdx.x) * SP_PIX;
  const bool in0 = p0 < hw, in1 = p0 + 1 < hw;
  const int ya = in0 ? p0 / w : -1, xa = in0 ? p0 - ya * w : -1;      // a pixel past the frame lies in no box
  const int yb = in1 ? (p0 + 1) / w : -1, xb = in1 ? p0 + 1 - yb * w : -1;
  const bool wide = in1 && (reinterpret_cast<uintptr_t>(out + p0) & 15) == 0;
  double v0 = -big, v1 = -big;
  if (!first) {
    if (wide) {
      const double2 v = *reinterpret_cast<const double2*>(out + p0);
      v0 = v.x, v1 = v.y;
    } else {
      if (in0) v0 = out[p0];
      if (in1) v1 = out[p0 + 1];
    }
  }
  double st[4] = {0.0, 1.0, 0.0, 1.0};
  if (stats) st[0] = stats[0], st[1] = stats[1], st[2] = stats[2], st[3] = stats[3];
  for (int base = 0; base < n; base += SP_STAGE) {
    const int cnt = min(SP_STAGE, n - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      const int b = base + (int)threadIdx.x, g = slot0 + b;
      int4 r = make_int4(0, 0, 0, 0);
      int counts = 0;
      if (keep[b] && mask[b]) {
        if (!boxes || g < n_host) {
          r = make_int4(rects[4 * g + 0], rects[4 * g + 1], rects[4 * g + 2], rects[4 * g + 3]);
        } else {
          const int x1 = boxes[4 * g + 0], y1 = boxes[4 * g + 1], x2 = boxes[4 * g + 2], y2 = boxes[4 * g + 3];
          r = make_int4(slice_bound(y1, h), slice_bound(y2, h), slice_bound(x1, w), slice_bound(x2, w));
        }
        counts = r.y > r.x && r.w > r.z;
      }
      srect[threadIdx.x] = r;
      sflag[threadIdx.x] = counts;
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      if (!sflag[k]) continue;                // the same for every lane
      const int4 r = srect[k];                // y0, y1, x0, x1
      const int64_t m0 = (int64_t)(base + k) * ZMAP_PIX;
      const bool hit0 = ya >= r.x && ya < r.y && xa >= r.z && xa < r.w;
      const bool hit1 = yb >= r.x && yb < r.y && xb >= r.z && xb < r.w;
      if (hit0) v0 = fmax(v0, stats ? zpaint_value(e_raw, e_of, st, w_raw, w_of, m0, ya, xa, r) : big);
      if (hit1) v1 = fmax(v1, stats ? zpaint_value(e_raw, e_of, st, w_raw, w_of, m0, yb, xb, r) : big);
    }
  }
  if (wide) {
    *reinterpret_cast<double2*>(out + p0) = make_double2(v0, v1);
  } else {
    if (in0) out[p0] = v0;
    if (in1) out[p0 + 1] = v1;
  }
}

// ---- the issued frame's boxes linked into tracks (vv_stream_tracks) ---------------------------------------------------------------------
constexpr int ST_STAGE = VV_STREAM_TRACK_STAGE;      // detections per LDS pass = threads of the workgroup
constexpr int ST_MAX = VV_STREAM_MAX_TRACKS;
constexpr int ST_PER = ST_MAX / 256;                 // consecutive slots a thread takes in the scan over free slots
static_assert(ST_STAGE == 256 && ST_MAX % 256 == 0, "one detection of a stage per thread, whole slots per thread");

// Rectangles are int4 (y0, y1, x0, x1), clipped to the h x w mask: an intersection is then at most h * w <= INT32_MAX.
__device__ __forceinline__ int4 st_clip(const int y0, const int y1, const int x0, const int x1, const int h, const int w) {
  return make_int4(min(max(y0, 0), h), min(max(y1, 0), h), min(max(x0, 0), w), min(max(x1, 0), w));
}

// The rectangle of box b as vv_stream_paint resolves it.
__device__ __forceinline__ int4 st_box_rect(const int b, const int nh, const int32_t* __restrict__ rects,
                                            const int32_t* __restrict__ boxes, const int h, const int w) {
  if (b < nh) return st_clip(rects[4 * b + 0], rects[4 * b + 1], rects[4 * b + 2], rects[4 * b + 3], h, w);
  const int x1 = boxes[4 * b + 0], y1 = boxes[4 * b + 1], x2 = boxes[4 * b + 2], y2 = boxes[4 * b + 3];
  return make_int4(slice_bound(y1, h), slice_bound(y2, h), slice_bound(x1, w), slice_bound(x2, w));
}

__device__ __forceinline__ int64_t st_area(const int4 r) { return (int64_t)(r.y - r.x) * (r.w - r.z); }

__device__ __forceinline__ int st_inter(const int4 a, const int4 b) {
  const int iy = min(a.y, b.y) - max(a.x, b.x), ix = min(a.w, b.w) - max(a.z, b.z);
  return (iy > 0 && ix > 0) ? iy * ix : 0;
}

// Exclusive scan of one int per thread over the workgroup, through LDS; *total = the sum.  Every thread calls it.
__device__ __forceinline__ int st_scan(const int v, int* buf, int* total) {
  const int tid = (int)threadIdx.x;
  buf[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int add = tid >= off ? buf[tid - off] : 0;
    __syncthreads();
    buf[tid] += add;
    __syncthreads();
  }
  const int incl = buf[tid];
  *total = buf[255];
  __syncthreads();
  return incl - v;
}

__device__ __forceinline__ void st_free(int32_t* meta, double* hist, const int window) {
  for (int k = 0; k < 8; ++k) meta[k] = 0;
  for (int k = 0; k < window; ++k) hist[k] = 0.0;
}

// One workgroup.  Slot t is owned by thread t % 256: only its owner touches its row of t_meta and t_hist until the matching is over,
// and the rectangles and flags (0 free, 1 live and unmatched, 2 matched) of all slots lie in LDS.  Box b's detection state lives in
// box_track[b][0] (-1 no detection, 0 unmatched, slot + 1 matched) and its score in box_track_score[b] until the last pass puts the
// outputs there; thread b % 256 alone reads and writes them.  A round of the matching: every unmatched track finds its best unmatched
// detection over all stages (ties: the lower box), then every unmatched detection its best unmatched track (ties: the lower slot); a
// pair that chose each other is matched.  The best pair of the whole order always is one, and a mutual-best pair is in the greedy
// matching, since every pair ahead of it in the order holds neither of its two.  Flags and rectangles change only between rounds.
__global__ void __launch_bounds__(256) stream_tracks_kernel(int32_t* t_meta, double* t_hist, int32_t* __restrict__ next_id,
                                                            int max_tracks,
                                                            const double* __restrict__ scores, int rows, int width,
                                                            const int32_t* __restrict__ n_ptr, int n_host,
                                                            const int32_t* __restrict__ rects, const int32_t* __restrict__ boxes, int h,
                                                            int w, int reset, int iou_pct, int max_age, int window, int min_hits,
                                                            double big, int32_t* box_track, double* box_track_score,
                                                            double* __restrict__ frame_track_score, int32_t* __restrict__ counts) {
  __shared__ int4 trect[ST_MAX];
  __shared__ int tflag[ST_MAX];
  __shared__ int tbi[ST_MAX];            // a track's best candidate of the round: intersection, union, box (-1: none)
  __shared__ unsigned tbu[ST_MAX];
  __shared__ int tbd[ST_MAX];            // ... and, once the matching is over, the free slots in ascending order
  __shared__ int tnew[ST_MAX];           // the box a track was matched with in this round, or -1
  __shared__ int4 srect[ST_STAGE];
  __shared__ int sstate[ST_STAGE];
  __shared__ int scan[256];
  __shared__ double part[256];
  __shared__ int s_live, s_det, s_match;          // s_match: the pairs matched so far in this launch
  const int tid = (int)threadIdx.x;
  const int n = min(max(n_ptr[0], 0), width);
  const int nh = boxes ? min(max(n_host, 0), n) : n;
  const int next0 = next_id[0];
  if (tid == 0) s_live = 0, s_det = 0, s_match = 0;
  __syncthreads();
  // steps 0 and 2: reset, ageing; the live tracks' rectangles into LDS
  for (int t = tid; t < ST_MAX; t += 256) {
    int flag = 0;
    if (t < max_tracks) {
      int32_t* m = t_meta + 8 * t;
      if (reset) {
        st_free(m, t_hist + (int64_t)t * window, window);
      } else if (m[0] > 0) {
        m[1] += 1;
        flag = 1;
        trect[t] = st_clip(m[3], m[4], m[5], m[6], h, w);
        atomicAdd(&s_live, 1);
      }
    }
    tflag[t] = flag;
  }
  // step 1: detections
  for (int b = tid; b < n; b += 256) {
    double s = -big;
    for (int i = 0; i < rows; ++i) s = fmax(s, scores[(int64_t)i * width + b]);
    const int4 r = st_box_rect(b, nh, rects, boxes, h, w);
    const bool det = r.y > r.x && r.w > r.z && s > -big;
    box_track_score[b] = s;
    box_track[2 * b + 0] = det ? 0 : -1;
    box_track[2 * b + 1] = 0;
    if (det) atomicAdd(&s_det, 1);
  }
  __syncthreads();
  // step 3: matching
  const int max_rounds = min(s_live, s_det);
  __syncthreads();                     // s_live is counted anew below
  for (int round = 0, matched = 0; round < max_rounds; ++round) {
    for (int t = tid; t < ST_MAX; t += 256) tbi[t] = 0, tbu[t] = 1u, tbd[t] = -1, tnew[t] = -1;
    for (int pass = 0; pass < 2; ++pass) {
      for (int base = 0; base < n; base += ST_STAGE) {
        const int cnt = min(ST_STAGE, n - base);
        __syncthreads();
        if (tid < cnt) {
          const int b = base + tid;
          srect[tid] = st_box_rect(b, nh, rects, boxes, h, w);
          sstate[tid] = box_track[2 * b];
        }
        __syncthreads();
        if (pass == 0) {               // a thread's tracks against the stage's detections
          for (int t = tid; t < max_tracks; t += 256) {
            if (tflag[t] != 1) continue;
            const int4 rt = trect[t];
            const int64_t at = st_area(rt);
            int bi = tbi[t], bd = tbd[t];
            int64_t bu = tbu[t];
            for (int k = 0; k < cnt; ++k) {
              if (sstate[k] != 0) continue;
              const int4 rd = srect[k];
              const int inter = st_inter(rt, rd);
              if (inter <= 0) continue;
              const int64_t uni = at + st_area(rd) - inter;
              if ((int64_t)100 * inter >= (int64_t)iou_pct * uni && (int64_t)inter * bu > (int64_t)bi * uni) bi = inter, bu = uni, bd = base + k;
            }
            tbi[t] = bi, tbu[t] = (unsigned)bu, tbd[t] = bd;
          }
        } else if (tid < cnt && sstate[tid] == 0) {      // a thread's detection against all tracks
          const int b = base + tid;
          const int4 rd = srect[tid];
          const int64_t ad = st_area(rd);
          int bi = 0, bt = -1;
          int64_t bu = 1;
          for (int t = 0; t < max_tracks; ++t) {
            if (tflag[t] != 1) continue;
            const int4 rt = trect[t];
            const int inter = st_inter(rt, rd);
            if (inter <= 0) continue;
            const int64_t uni = st_area(rt) + ad - inter;
            if ((int64_t)100 * inter >= (int64_t)iou_pct * uni && (int64_t)inter * bu > (int64_t)bi * uni) bi = inter, bu = uni, bt = t;
          }
          if (bt >= 0 && tbd[bt] == b) {
            tnew[bt] = b;
            box_track[2 * b] = bt + 1;
            atomicAdd(&s_match, 1);
          }
        }
      }
      __syncthreads();
    }
    for (int t = tid; t < max_tracks; t += 256) {
      const int d = tnew[t];
      if (tflag[t] != 1 || d < 0) continue;
      const int4 r = st_box_rect(d, nh, rects, boxes, h, w);
      int32_t* m = t_meta + 8 * t;
      const int hits = max(m[2], 0) + 1;
      m[1] = 0, m[2] = hits, m[3] = r.x, m[4] = r.y, m[5] = r.z, m[6] = r.w;
      t_hist[(int64_t)t * window + (hits - 1) % window] = box_track_score[d];
      tflag[t] = 2;
    }
    const int before = matched;
    matched = s_match;                  // counted before the barrier above, counted on behind the one below
    __syncthreads();
    if (matched == before || matched >= max_rounds) break;      // no candidate pair is left, or no track or no detection
  }
  // step 4: deaths
  if (tid == 0) s_live = 0;
  __syncthreads();
  for (int t = tid; t < max_tracks; t += 256) {
    if (tflag[t] == 0) continue;
    int32_t* m = t_meta + 8 * t;
    if (tflag[t] == 1 && m[1] > max_age) {
      st_free(m, t_hist + (int64_t)t * window, window);
      tflag[t] = 0;
    } else {
      atomicAdd(&s_live, 1);
    }
  }
  __syncthreads();
  // the free slots in ascending order
  int nfree = 0;
  {
    int c = 0;
    for (int k = 0; k < ST_PER; ++k) {
      const int t = ST_PER * tid + k;
      c += (t < max_tracks && tflag[t] == 0);
    }
    int at = st_scan(c, scan, &nfree);
    for (int k = 0; k < ST_PER; ++k) {
      const int t = ST_PER * tid + k;
      if (t < max_tracks && tflag[t] == 0) tbd[at++] = t;
    }
  }
  __syncthreads();
  // steps 5 and 6: births in ascending box index, and every box's outputs
  int unmatched = 0;
  double best = -INFINITY;
  for (int base = 0; base < n; base += ST_STAGE) {
    const int b = base + tid;
    const int state = b < n ? box_track[2 * b] : -1;
    int total;
    const int k = unmatched + st_scan(state == 0, scan, &total);
    unmatched += total;
    if (b >= n) continue;
    int id = 0, hits = 0;
    double ts = -big;
    if (state > 0) {
      const int t = state - 1;
      id = t_meta[8 * t + 0], hits = t_meta[8 * t + 2];
      const int m = min(hits, window);
      double acc = 0.0;
      for (int j = 0; j < m; ++j) acc += t_hist[(int64_t)t * window + (hits - m + j) % window];
      ts = acc / (double)m;
    } else if (state == 0 && k < nfree) {
      const int t = tbd[k];
      const int4 r = st_box_rect(b, nh, rects, boxes, h, w);
      const double s = box_track_score[b];
      int32_t* m = t_meta + 8 * t;
      id = next0 + k, hits = 1;
      m[0] = id, m[1] = 0, m[2] = 1, m[3] = r.x, m[4] = r.y, m[5] = r.z, m[6] = r.w, m[7] = 0;
      double* hist = t_hist + (int64_t)t * window;
      hist[0] = s;
      for (int j = 1; j < window; ++j) hist[j] = 0.0;
      ts = (0.0 + s) / 1.0;
    }
    box_track[2 * b + 0] = id;
    box_track[2 * b + 1] = hits;
    box_track_score[b] = ts;
    if (id > 0 && hits >= min_hits) best = fmax(best, ts);
  }
  part[tid] = best;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) part[tid] = fmax(part[tid], part[tid + s]);
    __syncthreads();
  }
  if (tid == 0) {
    const int births = min(unmatched, nfree);
    frame_track_score[0] = part[0] == -INFINITY ? -big : part[0];
    counts[0] = s_live + births;
    counts[1] = unmatched - births;
    counts[2] = next0 + births;
    next_id[0] = next0 + births;
  }
}

}  // namespace

extern "C" int vv_stream_tracks(int32_t* t_meta, double* t_hist, int32_t* next_id, int32_t max_tracks, const double* scores, int32_t rows,
                                int32_t width, const int32_t* n, int32_t n_host, const int32_t* rects, const int32_t* boxes, int32_t h,
                                int32_t w, int32_t reset, int32_t iou_pct, int32_t max_age, int32_t window, int32_t min_hits, double big,
                                int32_t* box_track, double* box_track_score, double* frame_track_score, int32_t* counts,
                                vv_stream stream) {
  if (max_tracks < 1 || max_tracks > ST_MAX || window < 1 || window > VV_STREAM_TRACK_WINDOW || iou_pct < 1 || iou_pct > 100) return VV_ERR_BAD_ARG;
  if (max_age < 0 || min_hits < 1 || rows < 0 || width < 0 || n_host < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX) return VV_ERR_BAD_ARG;
  if (!t_meta || !t_hist || !next_id || !n || !frame_track_score || !counts) return VV_ERR_BAD_ARG;
  if (width > 0 && (!rects || !box_track || !box_track_score || (rows > 0 && !scores))) return VV_ERR_BAD_ARG;
  VV_LAUNCH(stream_tracks_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, t_meta, t_hist, next_id, (int)max_tracks, scores, (int)rows,
            (int)width, n, (int)n_host, rects, boxes, (int)h, (int)w, (int)reset, (int)iou_pct, (int)max_age, (int)window, (int)min_hits,
            big, box_track, box_track_score, frame_track_score, counts);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_stream_paint(const double* scores, int32_t rows, int32_t width, const int32_t* n, int32_t n_host, int32_t* rects,
                               const int32_t* boxes, int32_t h, int32_t w, double* mask, double* box_max, int32_t* frame_off,
                               vv_stream stream) {
  if (rows < 0 || width < 0 || n_host < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX - SP_TILE) return VV_ERR_BAD_ARG;
  if (!n || !frame_off || ((int64_t)h * w > 0 && !mask) || ((uintptr_t)rects & 15)) return VV_ERR_BAD_ARG;
  if (width > 0 && (!rects || !box_max || (rows > 0 && !scores))) return VV_ERR_BAD_ARG;
  const int tiles = max(1, (h * w + SP_TILE - 1) / SP_TILE);      // a frame of no pixels still leaves box_max, rects and frame_off
  VV_LAUNCH(stream_paint_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, scores, (int)rows, (int)width, n, (int)n_host,
            reinterpret_cast<int4*>(rects), boxes, (int)h, (int)w, mask, box_max, frame_off);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_stream_zpaint(const float* e_raw, const float* e_of, const double* stats, double w_raw, double w_of, double big,
                                const uint8_t* keep, const uint8_t* mask, const int32_t* n, int32_t cap, int32_t slot0,
                                const int32_t* rects, int32_t n_host, const int32_t* boxes, int32_t h, int32_t w, double* out,
                                int32_t first, vv_stream stream) {
  if (!out || !n || !rects || cap < 0 || slot0 < 0 || n_host < 0 || h <= 0 || w <= 0 || (stats && !e_raw)) return VV_ERR_BAD_ARG;
  if (cap > 0 && (!keep || !mask)) return VV_ERR_BAD_ARG;
  if ((int64_t)h * w > INT32_MAX / 64 - SP_TILE || (int64_t)slot0 + cap > INT32_MAX / 4) return VV_ERR_BAD_ARG;      // zmap_src: 64 (v - lo) in int32
  const int tiles = (h * w + SP_TILE - 1) / SP_TILE;
  VV_LAUNCH(stream_zpaint_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, e_raw, stats ? e_of : nullptr, stats, w_raw,
            w_of, big, keep, mask, n, (int)cap, (int)slot0, rects, (int)n_host, boxes, (int)h, (int)w, out, (int)first);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_stream_boxes(const int32_t* count, const int32_t* boxes, int32_t mcap, int32_t n_ap, int32_t cap, int32_t H, int32_t W,
                               int32_t grid_h, int32_t grid_w, int32_t hb, int32_t wb, double h_step, double w_step, int32_t block_mode,
                               int32_t* n, int32_t* dropped, int32_t* crops, uint8_t* masks, int32_t* boxes_out, vv_stream stream) {
  if (mcap < 0 || cap <= 0 || n_ap < 0 || n_ap > cap || H <= 0 || W <= 0 || grid_h <= 0 || grid_w <= 0 || hb <= 0 || wb <= 0)
    return VV_ERR_BAD_ARG;
  if (!(h_step > 0.0) || !(w_step > 0.0) || block_mode < 1 || (int64_t)hb * wb * cap > 0x7fffffff) return VV_ERR_BAD_ARG;
  if (!count || (mcap > 0 && !boxes) || !n || !dropped || !crops || !masks || !boxes_out) return VV_ERR_BAD_ARG;
  VV_LAUNCH(stream_boxes_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, count, boxes, mcap, n_ap, cap, H, W, grid_h, grid_w, hb, wb,
            h_step, w_step, block_mode, n, dropped, crops, masks, boxes_out);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

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
  VV_LAUNCH(stream_cut_kernel, dim3((unsigned)cap, (unsigned)cams), dim3(256), 0, (hipStream_t)stream, raw_ring, cams * R,
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
  VV_LAUNCH(stream_scores_kernel, dim3((unsigned)cams), dim3(256), 0, (hipStream_t)stream, raw, of, stats, w_raw, w_of, big, keep,
            n, mask, cap, box_scores, box_stride, frame_score, frame_stride);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

// One camera is the launch above at cams = 1, with the row and the cell of camera 0; no refusal of the multi entries can fire at
// cams = 1 that is not one of these entries' own.
extern "C" int vv_stream_cut(const uint8_t* raw_ring, int32_t R, const float* flow_ring, int32_t Rf, int32_t H, int32_t W, int32_t C,
                             const int32_t* n, const int32_t* crops, const int32_t* raw_win, const int32_t* flow_win, int32_t cap,
                             int32_t T, int32_t Tf, int32_t P, double thr, uint8_t* raw_store, float* flow_store, uint8_t* keep,
                             double* energy, vv_stream stream) {
  return vv_stream_cut_multi(raw_ring, R, flow_ring, Rf, H, W, C, 1, n, crops, raw_win, flow_win, cap, T, Tf, P, thr, raw_store, flow_store,
                             keep, energy, stream);
}

extern "C" int vv_stream_scores(const float* raw, const float* of, const double* stats, double w_raw, double w_of, double big,
                                const uint8_t* keep, const int32_t* n, const uint8_t* mask, int32_t cap, double* box_scores,
                                double* frame_score, vv_stream stream) {
  return vv_stream_scores_multi(raw, of, stats, w_raw, w_of, big, keep, n, mask, 1, cap, box_scores, cap, frame_score, 1, stream);
}
