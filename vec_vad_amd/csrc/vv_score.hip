// Score aggregation on the device:
//   per-cube reconstruction errors -> z-normalised, weighted cube score -> frame score -> frame-level ROC-AUC
// replacing test.py:330-358 (numpy + one 240x360 float64 mask per cube + torch.save/torch.load per frame) and
// utils.py:29-41 (sklearn roc_curve + auc).  Both kernels are tiny and latency-bound; they exist so that the scores never
// leave HBM between the UNet bank and the final AUC.
//   cube scores + boxes -> painted h x w score masks (vv_paint_masks) and the pixel-level criterion (vv_pixel_scores), which
// the reference stores the masks for (test.py:350-358) and never evaluates (test.py:362-365: criterion = 'frame' only).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

#include "vv_score_fn.h"      // cube_score, shared with vv_stream.hip; switches FMA contraction off (products and sums rounded like numpy's)

namespace {

using namespace vv_score_fn;

// The reference paints score m into mask[ceil(y1):ceil(y2), ceil(x1):ceil(x2)] (background -1e5), max-combines the masks
// and later takes mask.max(): that is max over the cubes whose painted rectangle is non-empty, and -1e5 for frames with
// none.  All arithmetic in float64 like numpy's (float32 score - float64 mean) / float64 std.
__global__ void __launch_bounds__(256) frame_score_kernel(const float* __restrict__ raw, const float* __restrict__ of,
                                                          const int32_t* __restrict__ frame_off,
                                                          const int32_t* __restrict__ cube_stat,
                                                          const double* __restrict__ stats,
                                                          const uint8_t* __restrict__ paints, double w_raw, double w_of,
                                                          double big, int n_frames, double* __restrict__ frame_scores) {
  int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  double best = frame_scores[f];
  for (int m = frame_off[f]; m < frame_off[f + 1]; ++m) {
    if (!paints[m]) continue;
    best = fmax(best, cube_score(raw, of, cube_stat, stats, w_raw, w_of, big, m));
  }
  frame_scores[f] = best;
}

__global__ void __launch_bounds__(256) cube_score_kernel(const float* __restrict__ raw, const float* __restrict__ of,
                                                         const int32_t* __restrict__ cube_stat,
                                                         const double* __restrict__ stats, double w_raw, double w_of,
                                                         double big, int n, double* __restrict__ out) {
  int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) out[m] = cube_score(raw, of, cube_stat, stats, w_raw, w_of, big, m);
}

// ---- painted masks: P_f[y,x] = max(out, every score of frame f whose rectangle (y0, y1, x0, x1) holds (y,x)) -----------------
// Gather form: a thread owns two consecutive pixels of the frame taken as a flat h*w array, walks the frame's boxes (staged in
// LDS, PAINT_PASS per pass; every lane reads the same box -> broadcast) and writes its pair back with one 16-byte store.  The
// pairs are aligned on the ADDRESS (a frame of odd h*w starts 8 bytes off every other frame): `mis` shifts the tile by one pixel,
// and a pair that hangs over either end of the frame falls back to the one 8-byte store that is inside.
constexpr int PAINT_PASS = 256;              // boxes per LDS pass = threads of the workgroup
constexpr int PAINT_TILE = 2 * 256;          // pixels per workgroup

__global__ void __launch_bounds__(256) paint_mask_kernel(const double* __restrict__ scores,
                                                         const int32_t* __restrict__ frame_off,
                                                         const int4* __restrict__ rects, int f0, int h, int w,
                                                         double* __restrict__ out) {
  __shared__ int4 srect[PAINT_PASS];
  __shared__ double ssc[PAINT_PASS];
  const int f = f0 + blockIdx.y;
  const int m0 = frame_off[f], m1 = frame_off[f + 1];
  if (m1 <= m0) return;                      // a frame without boxes in this group keeps what it holds
  const int hw = h * w;
  double* fr = out + (int64_t)f * hw;
  const int mis = (int)((reinterpret_cast<uintptr_t>(fr) >> 3) & 1);
  const int p0 = blockIdx.x * PAINT_TILE + 2 * (int)threadIdx.x - mis;
  const bool in0 = p0 >= 0 && p0 < hw, in1 = p0 + 1 < hw;      // p0 + 1 >= 0 always
  double v0 = 0.0, v1 = 0.0;
  if (in0 && in1) {
    const double2 v = *reinterpret_cast<const double2*>(fr + p0);
    v0 = v.x; v1 = v.y;
  } else if (in0) {
    v0 = fr[p0];
  } else if (in1) {
    v1 = fr[p0 + 1];
  }
  const int ya = in0 ? p0 / w : 0, xa = in0 ? p0 - ya * w : 0;
  const int yb = in1 ? (p0 + 1) / w : 0, xb = in1 ? (p0 + 1) - yb * w : 0;
  for (int base = m0; base < m1; base += PAINT_PASS) {
    const int cnt = min(PAINT_PASS, m1 - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      srect[threadIdx.x] = rects[base + threadIdx.x];
      ssc[threadIdx.x] = scores[base + threadIdx.x];
    }
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const int4 r = srect[k];                // y0, y1, x0, x1
      const double s = ssc[k];
      if (ya >= r.x && ya < r.y && xa >= r.z && xa < r.w) v0 = fmax(v0, s);
      if (yb >= r.x && yb < r.y && xb >= r.z && xb < r.w) v1 = fmax(v1, s);
    }
  }
  if (in0 && in1) {
    *reinterpret_cast<double2*>(fr + p0) = make_double2(v0, v1);
  } else if (in0) {
    fr[p0] = v0;
  } else if (in1) {
    fr[p0 + 1] = v1;
  }
}

// ---- pixel-level criterion: one number per frame that carries the whole pixel-level ROC ------------------------------------
// Anomalous frame (|G| > 0 ground-truth pixels): the k-th largest painted value over G, k = ceil(|G| pct / 100); normal frame:
// the largest painted value = the frame score.  The mask is never formed: every ground-truth pixel names the best-scoring box
// that covers it (lowest index among equals) in an int32 LDS histogram with one extra bin for "no box"; integer LDS adds, so
// the totals do not depend on the order.  The k-th largest value is then the largest s_j whose cumulative count
//   cum(j) = sum of hist[i] over boxes i with s_i > s_j, or s_i == s_j and i <= j
// reaches k (the first box to reach k in descending order has hist > 0, and everything after it scores no more), or -big when
// none does.  cum(j) is formed per box by one thread: O(n^2 / 256) per workgroup for n <= PIX_CAP boxes.
constexpr int PIX_CAP = 2048;                // boxes per frame: 32 KB rectangles + 16 KB scores + 8 KB histogram of LDS

__device__ __forceinline__ void pixel_vote(int p, int w, int n, const int4* srect, const double* ssc, int* hist) {
  const int y = p / w, x = p - y * w;
  int best = n;                              // the "no box" bin
  double bs = 0.0;
  for (int k = 0; k < n; ++k) {
    const int4 r = srect[k];
    if (y >= r.x && y < r.y && x >= r.z && x < r.w) {
      const double s = ssc[k];
      if (best == n || s > bs) { best = k; bs = s; }
    }
  }
  atomicAdd(&hist[best], 1);
}

__global__ void __launch_bounds__(256) pixel_score_kernel(const uint8_t* __restrict__ gt, const double* __restrict__ scores,
                                                          const int32_t* __restrict__ frame_off,
                                                          const int4* __restrict__ rects, int pct, double big, int h, int w,
                                                          double* __restrict__ out, int32_t* __restrict__ gt_count) {
  __shared__ int4 srect[PIX_CAP];
  __shared__ double ssc[PIX_CAP];
  __shared__ int hist[PIX_CAP + 1];
  __shared__ double red[4];
  __shared__ int total;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int m0 = frame_off[f];
  const int n = max(0, min(frame_off[f + 1] - m0, PIX_CAP));      // the wrapper refuses more; here only memory is protected
  for (int k = tid; k < n; k += 256) {
    srect[k] = rects[m0 + k];
    ssc[k] = scores[m0 + k];
  }
  for (int k = tid; k <= n; k += 256) hist[k] = 0;
  if (tid == 0) total = 0;
  __syncthreads();

  // ground-truth pixels: single bytes up to the first 16-byte boundary, 16-byte loads, single bytes for the tail
  const int hw = h * w;
  const uint8_t* g = gt + (int64_t)f * hw;
  const int head = min(hw, (int)((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15));
  const int nvec = (hw - head) / 16;
  int mine = 0;
  for (int p = tid; p < head; p += 256) {
    if (g[p]) { ++mine; pixel_vote(p, w, n, srect, ssc, hist); }
  }
  for (int v = tid; v < nvec; v += 256) {
    const int p = head + 16 * v;
    const uint4 q = *reinterpret_cast<const uint4*>(g + p);
    const unsigned word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!word[j]) continue;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if ((word[j] >> (8 * b)) & 0xffu) { ++mine; pixel_vote(p + 4 * j + b, w, n, srect, ssc, hist); }
      }
    }
  }
  for (int p = head + 16 * nvec + tid; p < hw; p += 256) {
    if (g[p]) { ++mine; pixel_vote(p, w, n, srect, ssc, hist); }
  }
  if (mine) atomicAdd(&total, mine);
  __syncthreads();

  const int G = total;
  const long long kth = ((long long)G * pct + 99) / 100;
  double best = -big;
  for (int j = tid; j < n; j += 256) {
    const double sj = ssc[j];
    bool ok;
    if (G == 0) {
      const int4 r = srect[j];
      ok = r.y > r.x && r.w > r.z;           // a non-empty rectangle paints at least one pixel
    } else {
      long long cum = 0;
      for (int i = 0; i < n; ++i) {
        const double si = ssc[i];
        if (si > sj || (si == sj && i <= j)) cum += hist[i];
      }
      ok = cum >= kth;
    }
    if (ok) best = fmax(best, sj);
  }
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_down(best, o));
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    out[f] = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    gt_count[f] = G;
  }
}

// Mann-Whitney form of the ROC-AUC: AUC = (#{(p,n): s_p > s_n} + 0.5 #{s_p == s_n}) / (P N).  Exact integer counts, no
// sort: n^2 compares (n = 2 010 frames for UCSDped2, 40 791 for ShanghaiTech -> < 1 ms).
// out[0] += 2*wins + ties, out[1] = P, out[2] = N (written by block 0).
__global__ void __launch_bounds__(256) auc_count_kernel(const double* __restrict__ scores,
                                                        const uint8_t* __restrict__ labels, int n,
                                                        unsigned long long* __restrict__ out) {
  __shared__ double ss[256];
  __shared__ uint8_t sl[256];
  __shared__ unsigned long long red[4];
  int i = blockIdx.x * 256 + threadIdx.x;
  bool pos = i < n && labels[i] != 0;
  double si = i < n ? scores[i] : 0.0;
  unsigned long long acc = 0, npos = 0;
  for (int base = 0; base < n; base += 256) {
    int j = base + threadIdx.x;
    ss[threadIdx.x] = j < n ? scores[j] : 0.0;
    sl[threadIdx.x] = j < n ? (labels[j] != 0 ? 1 : 0) : 2;
    __syncthreads();
    if (pos) {
      for (int k = 0; k < 256; ++k) {
        if (sl[k] == 0) acc += si > ss[k] ? 2u : (si == ss[k] ? 1u : 0u);
      }
    }
    if (blockIdx.x == 0 && sl[threadIdx.x] == 1) npos += 1;
    __syncthreads();
  }
  // wave reduce, then across the 4 waves
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_down(acc, o);
    npos += __shfl_down(npos, o);
  }
  int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
  __syncthreads();
  if (blockIdx.x == 0) {
    if ((threadIdx.x & 63) == 0) red[wave] = npos;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long p = red[0] + red[1] + red[2] + red[3];
      out[1] = p;
      out[2] = (unsigned long long)n - p;
    }
  }
}

// ---- per-pixel anomaly maps: the per-pixel errors of vv_error_maps -> z-maps -> fine masks -> the pixel criterion on a formed mask --
// z[m][q] = cube_score with 1024 * e[m][q] in place of the cube's error (a 32x32 patch: the cube's error is the sum of its 1024 pixel
// errors, so a cube whose error is spread evenly gets the constant map z = its cube score, to the bit; the scaling by 2^10 is exact).
// ZMAP_PIX, ZMAP_SIDE and zmap_src (the nearest source pixel of a stretched patch) live in vv_score_fn.h, shared with vv_stream.hip.
__global__ void __launch_bounds__(256) error_zmap_kernel(const float* __restrict__ e_raw, const float* __restrict__ e_of,
                                                         const int32_t* __restrict__ cube_stat, const double* __restrict__ stats,
                                                         double w_raw, double w_of, double big, int64_t total,
                                                         double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const float r = 1024.f * e_raw[i];
  const float o = e_of ? 1024.f * e_of[i] : 0.f;
  out[i] = cube_score(&r, e_of ? &o : nullptr, cube_stat + i / ZMAP_PIX, stats, w_raw, w_of, big, 0);
}

// paint_mask_kernel with the value read from the cube's z-map instead of one score per box: same tiles, same pairs, same LDS passes
// over the frame's rectangles (no limit on their number); z is read through L2 only where the pixel lies inside the rectangle.
__global__ void __launch_bounds__(256) paint_zmap_kernel(const double* __restrict__ z, const int32_t* __restrict__ frame_off,
                                                         const int4* __restrict__ rects, int f0, int h, int w,
                                                         double* __restrict__ out) {
  __shared__ int4 srect[PAINT_PASS];
  const int f = f0 + blockIdx.y;
  const int m0 = frame_off[f], m1 = frame_off[f + 1];
  if (m1 <= m0) return;                      // a frame without boxes in this group keeps what it holds
  const int hw = h * w;
  double* fr = out + (int64_t)f * hw;
  const int mis = (int)((reinterpret_cast<uintptr_t>(fr) >> 3) & 1);
  const int p0 = blockIdx.x * PAINT_TILE + 2 * (int)threadIdx.x - mis;
  const bool in0 = p0 >= 0 && p0 < hw, in1 = p0 + 1 >= 0 && p0 + 1 < hw;
  double v0 = 0.0, v1 = 0.0;
  if (in0 && in1) {
    const double2 v = *reinterpret_cast<const double2*>(fr + p0);
    v0 = v.x; v1 = v.y;
  } else if (in0) {
    v0 = fr[p0];
  } else if (in1) {
    v1 = fr[p0 + 1];
  }
  const int ya = in0 ? p0 / w : -1, xa = in0 ? p0 - ya * w : -1;               // -1: inside no rectangle (y0, x0 >= 0)
  const int yb = in1 ? (p0 + 1) / w : -1, xb = in1 ? (p0 + 1) - yb * w : -1;
  for (int base = m0; base < m1; base += PAINT_PASS) {
    const int cnt = min(PAINT_PASS, m1 - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) srect[threadIdx.x] = rects[base + threadIdx.x];
    __syncthreads();
    for (int k = 0; k < cnt; ++k) {
      const int4 r = srect[k];                // y0, y1, x0, x1
      const double* zm = z + (int64_t)(base + k) * ZMAP_PIX;
      if (ya >= r.x && ya < r.y && xa >= r.z && xa < r.w)
        v0 = fmax(v0, zm[zmap_src(ya, r.x, r.y) * ZMAP_SIDE + zmap_src(xa, r.z, r.w)]);
      if (yb >= r.x && yb < r.y && xb >= r.z && xb < r.w)
        v1 = fmax(v1, zm[zmap_src(yb, r.x, r.y) * ZMAP_SIDE + zmap_src(xb, r.z, r.w)]);
    }
  }
  if (in0 && in1) {
    *reinterpret_cast<double2*>(fr + p0) = make_double2(v0, v1);
  } else if (in0) {
    fr[p0] = v0;
  } else if (in1) {
    fr[p0 + 1] = v1;
  }
}

// The pixel criterion on a formed mask: per frame the k-th largest mask value over the ground-truth pixels, k = ceil(|G| pct / 100),
// or the largest value of the whole mask for a frame without ground truth (= k-th largest with k = 1 over every pixel).  Exact
// radix select, most significant digit first, on the order-preserving 64-bit integer image of the doubles: per pass every selected
// pixel whose key continues the prefix found so far adds 1 to the int32 LDS histogram of its next digit (integer adds: the totals do
// not depend on the order), the digit that holds the k-th largest is read off the histogram from the top, and k is reduced by what
// lies above it.  11-bit digits (8 KB histogram): 5 passes of 11 bits and one of 9.  A NaN is outside the domain.
constexpr int KTH_BITS = 11, KTH_BINS = 1 << KTH_BITS;

__device__ __forceinline__ unsigned long long kth_key(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void __launch_bounds__(256) mask_kth_kernel(const uint8_t* __restrict__ gt, const double* __restrict__ masks, int pct,
                                                       double big, int hw, double* __restrict__ out,
                                                       int32_t* __restrict__ gt_count) {
  __shared__ int hist[KTH_BINS];
  __shared__ int chunk[256];
  __shared__ int total;
  __shared__ int sel_digit, sel_rest;
  const int f = blockIdx.x, tid = threadIdx.x;
  const uint8_t* g = gt + (int64_t)f * hw;
  const double* mk = masks + (int64_t)f * hw;
  if (tid == 0) total = 0;
  __syncthreads();
  int mine = 0;
  for (int p = tid; p < hw; p += 256) mine += g[p] != 0;
  if (mine) atomicAdd(&total, mine);
  __syncthreads();
  const int G = total;
  const bool all = G == 0;                   // a normal frame: the maximum over every pixel
  const int n_sel = all ? hw : G;
  if (n_sel == 0) {                          // a frame without pixels
    if (tid == 0) { out[f] = -big; gt_count[f] = 0; }
    return;
  }
  int k = all ? 1 : (int)(((long long)G * pct + 99) / 100);      // 1 <= k <= n_sel
  unsigned long long prefix = 0;             // the digits found so far, at their place in the key
  int done = 0;                              // bits of the key found so far
  while (done < 64) {
    const int width = min(KTH_BITS, 64 - done), shift = 64 - done - width;
    for (int b = tid; b < KTH_BINS; b += 256) hist[b] = 0;
    __syncthreads();
    for (int p = tid; p < hw; p += 256) {
      if (!all && !g[p]) continue;
      const unsigned long long key = kth_key(mk[p]);
      if (done && (key >> (64 - done)) != (prefix >> (64 - done))) continue;
      atomicAdd(&hist[(int)((key >> shift) & ((1u << width) - 1))], 1);
    }
    __syncthreads();
    // 256 chunks of 8 bins; thread 0 walks the chunk sums from the top, then the 8 bins of the chunk that reaches k
    int s = 0;
#pragma unroll
    for (int j = 0; j < KTH_BINS / 256; ++j) s += hist[tid * (KTH_BINS / 256) + j];
    chunk[tid] = s;
    __syncthreads();
    if (tid == 0) {
      int above = 0, c = 255;
      while (c > 0 && above + chunk[c] < k) { above += chunk[c]; --c; }
      int d = c * (KTH_BINS / 256) + (KTH_BINS / 256) - 1;
      while (d > c * (KTH_BINS / 256) && above + hist[d] < k) { above += hist[d]; --d; }
      sel_digit = d;
      sel_rest = k - above;
    }
    __syncthreads();
    prefix |= (unsigned long long)sel_digit << shift;
    k = sel_rest;
    done += width;
    __syncthreads();                         // sel_digit / sel_rest are read before the next pass rewrites them
  }
  if (tid == 0) {
    const unsigned long long u = (prefix >> 63) ? (prefix & 0x7fffffffffffffffull) : ~prefix;
    out[f] = __longlong_as_double((long long)u);
    gt_count[f] = G;
  }
}

}  // namespace

extern "C" int vv_frame_scores(const float* raw, const float* of, const int32_t* frame_off, const int32_t* cube_stat,
                               const double* stats, const uint8_t* paints, double w_raw, double w_of, double big,
                               int32_t n_frames, double* frame_scores, vv_stream stream) {
  if (!raw || !frame_off || !cube_stat || !stats || !paints || !frame_scores || n_frames < 0) return VV_ERR_BAD_ARG;
  if (n_frames == 0) return VV_OK;
  VV_LAUNCH(frame_score_kernel, dim3((n_frames + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw, of, frame_off,
            cube_stat, stats, paints, w_raw, w_of, big, n_frames, frame_scores);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_roc_auc_counts(const double* scores, const uint8_t* labels, int32_t n, uint64_t* out3,
                                 vv_stream stream) {
  if (!scores || !labels || !out3 || n < 0) return VV_ERR_BAD_ARG;
  {
    const hipError_t e = hipMemsetAsync(out3, 0, 3 * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) return VV_HIP_STATUS(e);
  }
  if (n == 0) return VV_OK;
  VV_LAUNCH(auc_count_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, labels, n,
            (unsigned long long*)out3);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_cube_scores(const float* raw, const float* of, const int32_t* cube_stat, const double* stats, double w_raw,
                              double w_of, double big, int32_t n, double* out, vv_stream stream) {
  if (n < 0) return VV_ERR_BAD_ARG;
  if (n == 0) return VV_OK;
  if (!raw || !cube_stat || !stats || !out) return VV_ERR_BAD_ARG;
  VV_LAUNCH(cube_score_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, raw, of, cube_stat, stats, w_raw,
            w_of, big, n, out);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_paint_masks(const double* scores, const int32_t* frame_off, const int32_t* rects, int32_t n_frames,
                              int32_t h, int32_t w, double* out, vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX - PAINT_TILE) return VV_ERR_BAD_ARG;
  if (n_frames == 0 || h == 0 || w == 0) return VV_OK;
  if (!scores || !frame_off || !rects || !out) return VV_ERR_BAD_ARG;
  const int tiles = (h * w + 1 + PAINT_TILE - 1) / PAINT_TILE;      // + 1: a frame that starts 8 bytes off a 16-byte boundary
  for (int f0 = 0; f0 < n_frames; f0 += 65535) {                    // gridDim.y
    VV_LAUNCH(paint_mask_kernel, dim3(tiles, min(65535, n_frames - f0)), dim3(256), 0, (hipStream_t)stream, scores,
              frame_off, reinterpret_cast<const int4*>(rects), f0, h, w, out);
    VV_CHECK_LAUNCH();
  }
  return VV_OK;
}

extern "C" int vv_pixel_scores(const uint8_t* gt, const double* scores, const int32_t* frame_off, const int32_t* rects,
                               int32_t pct, double big, int32_t n_frames, int32_t h, int32_t w, int32_t max_boxes, double* out,
                               int32_t* gt_count, vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || max_boxes < 0 || pct < 1 || pct > 100 || (int64_t)h * w > INT32_MAX) return VV_ERR_BAD_ARG;
  if (max_boxes > PIX_CAP) return VV_ERR_UNSUPPORTED;
  if (n_frames == 0) return VV_OK;
  if (!frame_off || !out || !gt_count || (!gt && h * w > 0) || ((!scores || !rects) && max_boxes > 0)) return VV_ERR_BAD_ARG;
  VV_LAUNCH(pixel_score_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, gt, scores, frame_off,
            reinterpret_cast<const int4*>(rects), pct, big, h, w, out, gt_count);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_error_zmaps(const float* e_raw, const float* e_of, const int32_t* cube_stat, const double* stats, double w_raw,
                              double w_of, double big, int32_t n, double* out, vv_stream stream) {
  if (n < 0) return VV_ERR_BAD_ARG;
  if (n == 0) return VV_OK;
  if (!e_raw || !cube_stat || !stats || !out) return VV_ERR_BAD_ARG;
  const int64_t total = (int64_t)n * ZMAP_PIX;
  if (total / 256 > INT32_MAX) return VV_ERR_BAD_ARG;
  VV_LAUNCH(error_zmap_kernel, dim3((unsigned)(total / 256)), dim3(256), 0, (hipStream_t)stream, e_raw, e_of, cube_stat, stats,
            w_raw, w_of, big, total, out);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_paint_zmaps(const double* z, const int32_t* frame_off, const int32_t* rects, int32_t n_frames, int32_t h,
                              int32_t w, double* out, vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX / 64 - PAINT_TILE) return VV_ERR_BAD_ARG;      // zmap_src: 64 (v - lo) in int32
  if (n_frames == 0 || h == 0 || w == 0) return VV_OK;
  if (!z || !frame_off || !rects || !out) return VV_ERR_BAD_ARG;
  const int tiles = (h * w + 1 + PAINT_TILE - 1) / PAINT_TILE;      // + 1: a frame that starts 8 bytes off a 16-byte boundary
  for (int f0 = 0; f0 < n_frames; f0 += 65535) {                    // gridDim.y
    VV_LAUNCH(paint_zmap_kernel, dim3(tiles, min(65535, n_frames - f0)), dim3(256), 0, (hipStream_t)stream, z, frame_off,
              reinterpret_cast<const int4*>(rects), f0, h, w, out);
    VV_CHECK_LAUNCH();
  }
  return VV_OK;
}

extern "C" int vv_mask_kth(const uint8_t* gt, const double* masks, int32_t pct, double big, int32_t n_frames, int32_t h, int32_t w,
                           double* out, int32_t* gt_count, vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || pct < 1 || pct > 100 || (int64_t)h * w > INT32_MAX - 256) return VV_ERR_BAD_ARG;
  if (n_frames == 0) return VV_OK;
  if (!out || !gt_count || ((!gt || !masks) && h * w > 0)) return VV_ERR_BAD_ARG;
  VV_LAUNCH(mask_kth_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, gt, masks, pct, big, h * w, out, gt_count);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
