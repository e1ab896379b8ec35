// Spatio-temporal mean filter of a score-mask volume ([mi355x] smooth_masks): the three separable passes of include/vecvad_hip.h
// (vv_smooth_masks), each sum taken term by term in ascending offset order in float64 from +0.0 -- no running sums, no tree, so the
// result is the one the plain-numpy restatement (tests/smooth_restatement.py) gives, to the bit.
//   smooth_xy_kernel: a 32x32 pixel tile of one frame plus a halo of rs = ks/2 pixels in LDS as value-or-zero and painted byte
//     (zeros past the image edge: x + (+0.0) == x for every partial sum, which starts at +0.0 and so is never -0.0, hence a term that
//     is "left out" and a term that is +0.0 give the same bits).  X sums A / a for the (32 + 2 rs) x 32 positions the tile's Y sums
//     read, then the Y sums B / b, stored as double and uint16 (b <= 33 * 33).  Lanes walk x: consecutive 8-byte LDS words in both
//     passes and full 256-byte rows to global memory.
//   smooth_t_kernel: one pixel per thread: the dt loop over the frames of the buffer that belong to the frame's video, one IEEE
//     division, the store, and the workgroup's maximum (wave shuffle, then LDS) as one partial per workgroup -- no atomics.
//   smooth_fmax_kernel: one workgroup per frame takes the maximum of the frame's partials.  A maximum does not round: exact.
//   stream_smooth_xy_kernel / stream_smooth_t_kernel (vv_stream_smooth): the same filter with a TRAILING window over a ring of the last
//     kt masks of a stream.  Only the issued frame's X/Y sums are formed (smooth_xy_tile, the device function smooth_xy_kernel calls:
//     the same bits); those of the window's earlier frames wait in their ring slots, 1/kt of the X/Y work of filtering the window
//     anew.  The window is a table in device memory, so the launch arguments do not change from frame to frame.
// The job is memory bound: per output frame the mask is read twice (tile with halo; painted test), B / b are written once and read kt
// times (the frames of a window are neighbours in time, so those reads mostly hit the L2 / MALL), and the output is written once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

constexpr int SM_T = 32;                       // output tile side
constexpr int SM_RMAX = VV_SMOOTH_MAX / 2;     // 16: the widest halo
constexpr double SM_BG = VV_SMOOTH_UNPAINTED;  // the background of a painted mask

__host__ __device__ constexpr int64_t sm_align8(int64_t v) { return (v + 7) & ~(int64_t)7; }

// dynamic LDS of smooth_xy_kernel for a halo of rs: V and A as doubles first (8-byte aligned), then a (uint16), then P (bytes)
__host__ __device__ constexpr int sm_lds_bytes(int rs) {
  const int tw = SM_T + 2 * rs;
  return tw * tw * 8 + tw * SM_T * 8 + tw * SM_T * 2 + tw * tw;
}

// The X/Y sums of tile `tile` of ONE h x w frame `m`, stored at the frame's Bsum / bcnt.  smooth_xy_kernel (a buffer of frames) and
// stream_smooth_xy_kernel (the one frame a stream issues) both call it: the same operations in the same order, the same bits.
__device__ __forceinline__ void smooth_xy_tile(const double* __restrict__ m, const int h, const int w, const int tile, const int tiles_x,
                                               const int rs, double* __restrict__ Bsum, uint16_t* __restrict__ bcnt, double* sm_lds) {
  const int tw = SM_T + 2 * rs;                // side of the tile with its halo
  double* V = sm_lds;                          // [tw][tw]   value or +0.0
  double* A = V + tw * tw;                     // [tw][32]   X sums
  uint16_t* an = reinterpret_cast<uint16_t*>(A + tw * SM_T);        // [tw][32]   X counts
  uint8_t* P = reinterpret_cast<uint8_t*>(an + tw * SM_T);          // [tw][tw]   painted
  const int tid = threadIdx.x;
  const int y0 = (tile / tiles_x) * SM_T, x0 = (tile % tiles_x) * SM_T;
  for (int i = tid; i < tw * tw; i += VV_WG) {
    const int ly = i / tw, lx = i - ly * tw;
    const int y = y0 - rs + ly, x = x0 - rs + lx;
    double v = 0.0;
    uint8_t p = 0;
    if (y >= 0 && y < h && x >= 0 && x < w) {
      const double mv = m[(int64_t)y * w + x];
      p = mv != SM_BG;
      v = p ? mv : 0.0;
    }
    V[i] = v;
    P[i] = p;
  }
  __syncthreads();
  for (int i = tid; i < tw * SM_T; i += VV_WG) {       // A[ly][tx] = sum over dx = -rs..rs of V[ly][tx + rs + dx], ascending dx
    const int ly = i / SM_T, tx = i % SM_T;
    const double* row = V + ly * tw + tx;
    const uint8_t* prow = P + ly * tw + tx;
    double s = 0.0;
    int c = 0;
    for (int k = 0; k <= 2 * rs; ++k) {
      s += row[k];
      c += prow[k];
    }
    A[i] = s;
    an[i] = (uint16_t)c;
  }
  __syncthreads();
  for (int i = tid; i < SM_T * SM_T; i += VV_WG) {     // B[ty][tx] = sum over dy = -rs..rs of A[ty + rs + dy][tx], ascending dy
    const int ty = i / SM_T, tx = i % SM_T;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= h || x >= w) continue;
    double s = 0.0;
    int c = 0;
    for (int k = 0; k <= 2 * rs; ++k) {
      s += A[(ty + k) * SM_T + tx];
      c += an[(ty + k) * SM_T + tx];
    }
    const int64_t o = (int64_t)y * w + x;
    Bsum[o] = s;
    bcnt[o] = (uint16_t)c;
  }
}

__global__ void __launch_bounds__(VV_WG)
smooth_xy_kernel(const double* __restrict__ masks, const int h, const int w, const int fa, const int tiles_x, const int tiles,
                 const int rs, double* __restrict__ Bsum, uint16_t* __restrict__ bcnt) {
  extern __shared__ double sm_lds[];
  const int64_t fo = (int64_t)(fa + blockIdx.x / tiles) * h * w;
  smooth_xy_tile(masks + fo, h, w, blockIdx.x % tiles, tiles_x, rs, Bsum + fo, bcnt + fo, sm_lds);
}

// ---- the trailing window of a stream (vv_stream_smooth) ------------------------------------------------------------------------------
// win int32 [1 + kt] in device memory: the number of frames of the window (clamped to 1..kt), then their ring slots in ascending
// frame order (clamped to the ring), the last one being the issued frame.  Entries behind the count are not read.
struct StreamWin { int count, cur; };
__device__ __forceinline__ int sm_slot(const int32_t* __restrict__ win, const int j, const int K) { return min(max(win[j], 0), K - 1); }
__device__ __forceinline__ StreamWin sm_window(const int32_t* __restrict__ win, const int kt, const int K) {
  StreamWin s;
  s.count = min(max(win[0], 1), kt);
  s.cur = sm_slot(win, s.count, K);
  return s;
}

// step (a): the X/Y sums of the issued frame's slot alone; the sums of the window's earlier frames stay in their slots
__global__ void __launch_bounds__(VV_WG)
stream_smooth_xy_kernel(const double* __restrict__ ring, const int h, const int w, const int K, const int32_t* __restrict__ win,
                        const int kt, const int tiles_x, const int rs, double* __restrict__ Bsum, uint16_t* __restrict__ bcnt) {
  extern __shared__ double sm_lds[];
  const int64_t fo = (int64_t)sm_window(win, kt, K).cur * h * w;
  smooth_xy_tile(ring + fo, h, w, blockIdx.x, tiles_x, rs, Bsum + fo, bcnt + fo, sm_lds);
}

// step (b): one pixel per thread: the T sums over the window's slots in the table's order, one IEEE division, the store, and the
// workgroup's maximum as one partial -- smooth_t_kernel with the window read from a table
__global__ void __launch_bounds__(VV_WG)
stream_smooth_t_kernel(const double* __restrict__ ring, const int64_t hw, const int K, const int32_t* __restrict__ win, const int kt,
                       const double* __restrict__ Bsum, const uint16_t* __restrict__ bcnt, double* __restrict__ out,
                       double* __restrict__ partial) {
  __shared__ double wmax[VV_WG / 64];
  const int64_t pix = (int64_t)blockIdx.x * VV_WG + threadIdx.x;
  double best = SM_BG;
  if (pix < hw) {
    const StreamWin sw = sm_window(win, kt, K);
    double s = 0.0;
    int c = 0;
    for (int j = 1; j <= sw.count; ++j) {      // ascending frame order; the slot is wave-uniform
      const int64_t o = (int64_t)sm_slot(win, j, K) * hw + pix;
      s += Bsum[o];
      c += bcnt[o];
    }
    const bool p = ring[(int64_t)sw.cur * hw + pix] != SM_BG;      // a painted pixel counts itself: c >= 1
    best = p ? s / (double)c : SM_BG;
    out[pix] = best;
  }
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_down(best, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < VV_WG / 64; ++k) best = fmax(best, wmax[k]);
    partial[blockIdx.x] = best;
  }
}

__global__ void __launch_bounds__(VV_WG)
smooth_t_kernel(const double* __restrict__ masks, const int32_t* __restrict__ vid, const int F, const int64_t hw, const int f0,
                const int nblk, const int rt, const double* __restrict__ Bsum, const uint16_t* __restrict__ bcnt,
                double* __restrict__ out, double* __restrict__ partial) {
  __shared__ double wmax[VV_WG / 64];
  const int blk = blockIdx.x % nblk;
  const int fo = blockIdx.x / nblk;            // frame of the output
  const int f = f0 + fo;                       // ... and of the buffer
  const int64_t pix = (int64_t)blk * VV_WG + threadIdx.x;
  double best = SM_BG;
  if (pix < hw) {
    const int v = vid[f];
    double s = 0.0;
    int c = 0;
    const int g0 = f - rt < 0 ? 0 : f - rt, g1 = f + rt >= F ? F - 1 : f + rt;
    for (int g = g0; g <= g1; ++g) {           // ascending dt; g and vid[g] are wave-uniform
      if (vid[g] != v) continue;
      s += Bsum[(int64_t)g * hw + pix];
      c += bcnt[(int64_t)g * hw + pix];
    }
    const bool p = masks[(int64_t)f * hw + pix] != SM_BG;      // a painted pixel counts itself: c >= 1
    best = p ? s / (double)c : SM_BG;
    out[(int64_t)fo * hw + pix] = best;
  }
  if (!partial) return;
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_down(best, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < VV_WG / 64; ++k) best = fmax(best, wmax[k]);
    partial[blockIdx.x] = best;
  }
}

__global__ void __launch_bounds__(VV_WG)
smooth_fmax_kernel(const double* __restrict__ partial, const int nblk, double* __restrict__ fmax_out) {
  __shared__ double wmax[VV_WG / 64];
  const double* p = partial + (int64_t)blockIdx.x * nblk;
  double best = SM_BG;                         // a frame of no pixels keeps the background
  for (int i = threadIdx.x; i < nblk; i += VV_WG) best = fmax(best, p[i]);
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_down(best, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < VV_WG / 64; ++k) best = fmax(best, wmax[k]);
    fmax_out[blockIdx.x] = best;
  }
}

bool sm_sizes_ok(int32_t F, int32_t h, int32_t w, int32_t kt, int32_t ks) {
  if (F < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX) return false;
  return kt >= 1 && kt <= VV_SMOOTH_MAX && kt % 2 == 1 && ks >= 1 && ks <= VV_SMOOTH_MAX && ks % 2 == 1;
}

}  // namespace

// work: B double [F][h*w] | b uint16 [F][h*w] (padded to 8 bytes) | partial maxima double [F][ceil(h*w / 256)]
extern "C" int64_t vv_smooth_masks_work(int32_t F, int32_t h, int32_t w, int32_t kt, int32_t ks) {
  if (!sm_sizes_ok(F, h, w, kt, ks)) return -1;
  const int64_t hw = (int64_t)h * w, n = (int64_t)F * hw;
  return n * 8 + sm_align8(n * 2) + (int64_t)F * ((hw + VV_WG - 1) / VV_WG) * 8;
}

extern "C" int vv_smooth_masks(const double* masks, const int32_t* vid, int32_t F, int32_t h, int32_t w, int32_t f0, int32_t f1,
                               int32_t kt, int32_t ks, double* out, double* fmax_out, void* work, vv_stream stream) {
  static_assert(sm_lds_bytes(SM_RMAX) <= 64 * 1024, "the widest tile with its halo must fit a workgroup's LDS");
  if (!sm_sizes_ok(F, h, w, kt, ks) || f0 < 0 || f0 > f1 || f1 > F) return VV_ERR_BAD_ARG;
  if (F == 0 || f0 == f1) return VV_OK;
  const int64_t hw = (int64_t)h * w;
  const int nf = f1 - f0;
  const int nblk = (int)((hw + VV_WG - 1) / VV_WG);
  if (hw == 0) {                               // frames of no pixels: nothing to filter, the maxima are the background
    if (fmax_out) {
      VV_LAUNCH(smooth_fmax_kernel, dim3((unsigned)nf), dim3(VV_WG), 0, (hipStream_t)stream, (const double*)nullptr, 0, fmax_out);
      VV_CHECK_LAUNCH();
    }
    return VV_OK;
  }
  if (!masks || !vid || !out || !work || ((uintptr_t)work & 7)) return VV_ERR_BAD_ARG;
  const int rt = kt / 2, rs = ks / 2;
  const int fa = f0 - rt < 0 ? 0 : f0 - rt, fb = f1 + rt > F ? F : f1 + rt;      // the frames the T pass reads
  const int tiles_x = (w + SM_T - 1) / SM_T, tiles = tiles_x * ((h + SM_T - 1) / SM_T);
  if ((int64_t)tiles * (fb - fa) > INT32_MAX || (int64_t)nblk * nf > INT32_MAX) return VV_ERR_UNSUPPORTED;
  const int64_t n = (int64_t)F * hw;
  double* Bsum = static_cast<double*>(work);
  uint16_t* bcnt = reinterpret_cast<uint16_t*>(Bsum + n);
  double* partial = fmax_out ? reinterpret_cast<double*>(reinterpret_cast<char*>(bcnt) + sm_align8(n * 2)) : nullptr;
  VV_LAUNCH(smooth_xy_kernel, dim3((unsigned)(tiles * (fb - fa))), dim3(VV_WG), (size_t)sm_lds_bytes(rs), (hipStream_t)stream, masks,
            (int)h, (int)w, fa, tiles_x, tiles, rs, Bsum, bcnt);
  VV_CHECK_LAUNCH();
  VV_LAUNCH(smooth_t_kernel, dim3((unsigned)(nblk * nf)), dim3(VV_WG), 0, (hipStream_t)stream, masks, vid, (int)F, hw, (int)f0, nblk,
            rt, (const double*)Bsum, (const uint16_t*)bcnt, out, partial);
  VV_CHECK_LAUNCH();
  if (fmax_out) {
    VV_LAUNCH(smooth_fmax_kernel, dim3((unsigned)nf), dim3(VV_WG), 0, (hipStream_t)stream, (const double*)partial, nblk, fmax_out);
    VV_CHECK_LAUNCH();
  }
  return VV_OK;
}

extern "C" int64_t vv_stream_smooth_partials(int32_t h, int32_t w) {
  if (h < 0 || w < 0 || (int64_t)h * w > INT32_MAX) return -1;
  return ((int64_t)h * w + VV_WG - 1) / VV_WG;
}

extern "C" int vv_stream_smooth(const double* ring, int32_t K, int32_t h, int32_t w, const int32_t* win, int32_t kt, int32_t ks,
                                double* Bsum, uint16_t* bcnt, double* out, double* partial, vv_stream stream) {
  if (K < 1 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX || (int64_t)K * h * w > INT64_MAX / 8) return VV_ERR_BAD_ARG;
  if (kt < 1 || kt > VV_SMOOTH_MAX || ks < 1 || ks > VV_SMOOTH_MAX || ks % 2 == 0) return VV_ERR_BAD_ARG;
  const int64_t hw = (int64_t)h * w;
  if (hw == 0) return VV_OK;                   // frames of no pixels: no partial either, the caller's maximum is the background
  if (!ring || !win || !Bsum || !bcnt || !out || !partial) return VV_ERR_BAD_ARG;
  const int rs = ks / 2;
  const int tiles_x = (w + SM_T - 1) / SM_T, tiles = tiles_x * ((h + SM_T - 1) / SM_T);
  const int nblk = (int)((hw + VV_WG - 1) / VV_WG);
  VV_LAUNCH(stream_smooth_xy_kernel, dim3((unsigned)tiles), dim3(VV_WG), (size_t)sm_lds_bytes(rs), (hipStream_t)stream, ring, (int)h,
            (int)w, (int)K, win, (int)kt, tiles_x, rs, Bsum, bcnt);
  VV_CHECK_LAUNCH();
  VV_LAUNCH(stream_smooth_t_kernel, dim3((unsigned)nblk), dim3(VV_WG), 0, (hipStream_t)stream, ring, hw, (int)K, win, (int)kt,
            (const double*)Bsum, (const uint16_t*)bcnt, out, partial);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
