// Region- and track-based detection criteria (RBDC / TBDC) on the device: the exact integer geometry behind them.
//   per-pixel ground truth -> 8-connected regions, numbered in raster order of their first pixel (vv_label_regions)
//   regions x scored boxes -> region areas, best matching score per region, matched / false-positive state per box (vv_region_match)
//   regions of consecutive frames that share a pixel position -> link bits (vv_region_links)
// Everything is integer counting plus a max over doubles, so the results do not depend on the order anything runs in.  The
// curves themselves are a host matter of a few thousand numbers (vec_vad_amd/scoring.py: link_tracks, region_curves).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

constexpr int REGION_MAX = VV_REGION_MAX;    // regions per frame the match and link tables hold
constexpr int LABEL_TILE = 256;              // pixels per workgroup of the union-find passes
constexpr int RANK_WG = 1024;                // threads of the per-frame ranking workgroup
constexpr int LINK_PER_THREAD = 8;           // pixels per thread of the link pass: one LDS table per 2048 pixels

// ---- labelling: union-find on pixel indices of one frame -------------------------------------------------------------------
// L[p] is the parent of pixel p (an index into the same frame, -1 for background) with the invariant L[p] <= p, which every
// write keeps (atomicMin only lowers, flatten writes a root that lies below).  So a walk up the tree strictly descends and
// ends at a root (L[r] == r) after at most p steps, whatever other threads do meanwhile; nothing here waits for another
// workgroup.  The root of a finished component is its smallest index = its first pixel in raster order.
__device__ __forceinline__ int uf_load(const int32_t* L, int i) { return __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int32_t* L, int a) {
  for (int p = uf_load(L, a); p != a; p = uf_load(L, a)) a = p;      // p < a: strictly descending
  return a;
}

// Joins the trees of a and b.  Per round, with a > b the two roots found: atomicMin(L[a], b) either hooks the root a under b
// (it returned a: done) or finds that a got a parent `old` < a meanwhile, and the round is repeated with (old, b): max(a, b)
// strictly decreases from round to round, so there are at most max(a, b) rounds.
__device__ __forceinline__ void uf_union(int32_t* L, int a, int b) {
  while (true) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(LABEL_TILE) label_init_kernel(const uint8_t* __restrict__ gt, int32_t* __restrict__ labels, int f0,
                                                                int hw) {
  const int p = blockIdx.x * LABEL_TILE + threadIdx.x;
  if (p >= hw) return;
  const int64_t base = (int64_t)(f0 + blockIdx.y) * hw;
  labels[base + p] = gt[base + p] ? p : -1;
}

// every foreground pixel joins its W, NW, N and NE neighbours (the other four directions are those pixels' own joins)
__global__ void __launch_bounds__(LABEL_TILE) label_merge_kernel(int32_t* __restrict__ labels, int f0, int h, int w) {
  const int hw = h * w;
  const int p = blockIdx.x * LABEL_TILE + threadIdx.x;
  if (p >= hw) return;
  int32_t* L = labels + (int64_t)(f0 + blockIdx.y) * hw;
  if (uf_load(L, p) < 0) return;
  const int y = p / w, x = p - y * w;
  if (x > 0 && uf_load(L, p - 1) >= 0) uf_union(L, p, p - 1);
  if (y > 0) {
    const int q = p - w;
    if (uf_load(L, q) >= 0) uf_union(L, p, q);
    if (x > 0 && uf_load(L, q - 1) >= 0) uf_union(L, p, q - 1);
    if (x + 1 < w && uf_load(L, q + 1) >= 0) uf_union(L, p, q + 1);
  }
}

// L[p] = root of p.  The trees no longer change shape here except by this very shortening, which keeps L[p] <= p and the roots.
__global__ void __launch_bounds__(LABEL_TILE) label_flatten_kernel(int32_t* __restrict__ labels, int f0, int hw) {
  const int p = blockIdx.x * LABEL_TILE + threadIdx.x;
  if (p >= hw) return;
  int32_t* L = labels + (int64_t)(f0 + blockIdx.y) * hw;
  if (uf_load(L, p) < 0) return;
  const int r = uf_find(L, p);
  __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per frame turns root indices into the canonical numbers: roots are ranked in raster order with a block scan over
// tiles of RANK_WG pixels and marked -(rank + 1) (<= -2; background is -1), then every other foreground pixel (still >= 0: the
// index of its root, which is not rewritten in that phase) takes its root's rank, then roots and background take their final
// values.  The phases are separated by workgroup barriers; no other workgroup touches the frame.
__global__ void __launch_bounds__(RANK_WG) label_rank_kernel(int32_t* labels, int32_t* n_regions, int hw) {
  __shared__ int wsum[RANK_WG / 64];
  __shared__ int carry;
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int32_t* L = labels + (int64_t)f * hw;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < hw; base += RANK_WG) {      // hw <= INT32_MAX - RANK_WG: base does not wrap
    const int p = base + tid;
    const bool root = p < hw && L[p] == p;
    const unsigned long long m = __ballot(root);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(m);
    __syncthreads();
    int off = carry, tot = 0;
    for (int k = 0; k < RANK_WG / 64; ++k) {
      const int s = wsum[k];
      off += k < wave ? s : 0;
      tot += s;
    }
    if (root) L[p] = -(off + before + 1) - 1;           // rank = off + before + 1
    __syncthreads();                                    // every thread has read carry and wsum
    if (tid == 0) carry += tot;
  }
  __syncthreads();
  if (tid == 0) n_regions[f] = carry;
  for (int p = tid; p < hw; p += RANK_WG) {
    const int r = L[p];
    if (r >= 0) L[p] = -L[r] - 1;                       // L[r] <= -2 stays as it is until the next barrier
  }
  __syncthreads();
  for (int p = tid; p < hw; p += RANK_WG) {
    const int v = L[p];
    if (v < 0) L[p] = -v - 1;                           // background -1 -> 0, root -(rank + 1) -> rank
  }
}

// ---- match: one workgroup per frame ---------------------------------------------------------------------------------------------
// area[r] from an LDS histogram of the frame's labels; per box (a loop over the CSR range: any number of boxes) the threads stride
// over its rectangle and count the pixels of every region inside it in a second LDS histogram; thread r < 64 owns region r + 1:
// the integer IoU test in int64 and the max into the region's score.  Integer adds and fmax: independent of the order.
__global__ void __launch_bounds__(256) region_match_kernel(const int32_t* __restrict__ labels, const double* __restrict__ scores,
                                                           const int32_t* __restrict__ frame_off, const int4* __restrict__ rects,
                                                           int pct, double big, int h, int w, int32_t* __restrict__ region_area,
                                                           double* __restrict__ region_score, uint8_t* __restrict__ box_state) {
  __shared__ int area[REGION_MAX + 1];
  __shared__ int inter[REGION_MAX + 1];
  __shared__ int hit;
  const int f = blockIdx.x, tid = threadIdx.x;
  const int hw = h * w;
  const int32_t* L = labels + (int64_t)f * hw;
  if (tid <= REGION_MAX) area[tid] = 0;
  __syncthreads();
  for (int p = tid; p < hw; p += 256) {
    const int l = L[p];
    if (l > 0 && l <= REGION_MAX) atomicAdd(&area[l], 1);
  }
  __syncthreads();
  double best = -big;                                   // of region tid + 1, in threads 0..63
  const int my_area = tid < REGION_MAX ? area[tid + 1] : 0;
  const int m0 = frame_off[f], m1 = frame_off[f + 1];
  for (int m = m0; m < m1; ++m) {
    const int4 r = rects[m];                            // y0, y1, x0, x1; clamped here only to protect memory (box_rects clips)
    const int y0 = max(r.x, 0), y1 = min(r.y, h), x0 = max(r.z, 0), x1 = min(r.w, w);
    if (y1 <= y0 || x1 <= x0) {                         // uniform over the workgroup
      if (tid == 0) box_state[m] = 0;
      continue;
    }
    if (tid <= REGION_MAX) inter[tid] = 0;
    if (tid == 0) hit = 0;
    __syncthreads();
    const int rw = x1 - x0;
    const int n = (y1 - y0) * rw;                       // <= h * w
    for (int i = tid; i < n; i += 256) {
      const int dy = i / rw;
      const int l = L[(y0 + dy) * w + x0 + (i - dy * rw)];
      if (l > 0 && l <= REGION_MAX) atomicAdd(&inter[l], 1);
    }
    __syncthreads();
    if (tid < REGION_MAX) {
      const long long in = inter[tid + 1];
      if (in > 0 && 100ll * in >= (long long)pct * ((long long)n + my_area - in)) {
        best = fmax(best, scores[m]);
        hit = 1;                                        // every writer writes 1
      }
    }
    __syncthreads();
    if (tid == 0) box_state[m] = hit ? 1 : 2;
    __syncthreads();                                    // hit and inter are read before the next box clears them
  }
  if (tid < REGION_MAX) {
    region_area[(int64_t)f * REGION_MAX + tid] = my_area;
    region_score[(int64_t)f * REGION_MAX + tid] = best;
  }
}

// ---- links: bit q-1 of links[f][r-1] when region r of frame f and region q of the frame before share a pixel position ----------
// A workgroup takes 2048 pixel positions of one frame pair, ORs into a 64 x 64-bit LDS table and sends the non-zero rows on with one
// 64-bit global atomicOr each (vector memory instructions).  OR is idempotent and commutative: independent of the order.
__global__ void __launch_bounds__(256) region_links_kernel(const int32_t* __restrict__ prev_labels, const int32_t* __restrict__ labels,
                                                           const uint8_t* __restrict__ same_video, int f0, int hw,
                                                           unsigned long long* __restrict__ links) {
  __shared__ unsigned long long tab[REGION_MAX];
  const int f = f0 + blockIdx.y, tid = threadIdx.x;
  if (!same_video[f]) return;                           // uniform over the workgroup
  const int32_t* cur = labels + (int64_t)f * hw;
  const int32_t* prv = f > 0 ? cur - hw : prev_labels;
  if (!prv) return;
  if (tid < REGION_MAX) tab[tid] = 0ull;
  __syncthreads();
  const int64_t start = (int64_t)blockIdx.x * (256 * LINK_PER_THREAD);
#pragma unroll
  for (int j = 0; j < LINK_PER_THREAD; ++j) {
    const int64_t p = start + j * 256 + tid;
    if (p >= hw) break;
    const int l = cur[p];
    if (l <= 0 || l > REGION_MAX) continue;
    const int q = prv[p];
    if (q <= 0 || q > REGION_MAX) continue;
    atomicOr(&tab[l - 1], 1ull << (q - 1));
  }
  __syncthreads();
  if (tid < REGION_MAX && tab[tid]) atomicOr(links + (int64_t)f * REGION_MAX + tid, tab[tid]);
}

}  // namespace

extern "C" int vv_label_regions(const uint8_t* gt, int32_t* labels, int32_t* n_regions, int32_t n_frames, int32_t h, int32_t w,
                                vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX) return VV_ERR_BAD_ARG;
  if (n_frames == 0) return VV_OK;
  if (!n_regions || ((!gt || !labels) && (int64_t)h * w > 0)) return VV_ERR_BAD_ARG;
  const int64_t hw64 = (int64_t)h * w;
  if (hw64 > INT32_MAX - RANK_WG) return VV_ERR_UNSUPPORTED;      // the tile loops count in int32
  const int hw = (int)hw64;
  if (hw > 0) {
    const int tiles = (hw + LABEL_TILE - 1) / LABEL_TILE;
    for (int f0 = 0; f0 < n_frames; f0 += 65535) {                  // gridDim.y
      const dim3 grid(tiles, min(65535, n_frames - f0));
      VV_LAUNCH(label_init_kernel, grid, dim3(LABEL_TILE), 0, (hipStream_t)stream, gt, labels, f0, hw);
      VV_CHECK_LAUNCH();
      VV_LAUNCH(label_merge_kernel, grid, dim3(LABEL_TILE), 0, (hipStream_t)stream, labels, f0, h, w);
      VV_CHECK_LAUNCH();
      VV_LAUNCH(label_flatten_kernel, grid, dim3(LABEL_TILE), 0, (hipStream_t)stream, labels, f0, hw);
      VV_CHECK_LAUNCH();
    }
  }
  VV_LAUNCH(label_rank_kernel, dim3(n_frames), dim3(RANK_WG), 0, (hipStream_t)stream, labels, n_regions, hw);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_region_match(const int32_t* labels, const double* scores, const int32_t* frame_off, const int32_t* rects,
                               int32_t iou_pct, double big, int32_t n_frames, int32_t h, int32_t w, int32_t n_boxes,
                               int32_t* region_area, double* region_score, uint8_t* box_state, vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || n_boxes < 0 || iou_pct < 1 || iou_pct > 100 || (int64_t)h * w > INT32_MAX)
    return VV_ERR_BAD_ARG;
  if (n_frames == 0) return VV_OK;
  if (!frame_off || !region_area || !region_score || (!labels && (int64_t)h * w > 0) || ((!scores || !rects || !box_state) && n_boxes > 0))
    return VV_ERR_BAD_ARG;
  if ((int64_t)h * w > INT32_MAX - 256) return VV_ERR_UNSUPPORTED;
  VV_LAUNCH(region_match_kernel, dim3(n_frames), dim3(256), 0, (hipStream_t)stream, labels, scores, frame_off,
            reinterpret_cast<const int4*>(rects), iou_pct, big, h, w, region_area, region_score, box_state);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_region_links(const int32_t* prev_labels, const int32_t* labels, const uint8_t* same_video, int32_t n_frames,
                               int32_t h, int32_t w, uint64_t* links, vv_stream stream) {
  if (n_frames < 0 || h < 0 || w < 0 || (int64_t)h * w > INT32_MAX) return VV_ERR_BAD_ARG;
  if (n_frames == 0) return VV_OK;
  if (!links || !same_video || (!labels && (int64_t)h * w > 0)) return VV_ERR_BAD_ARG;
  {
    const hipError_t e = hipMemsetAsync(links, 0, (size_t)n_frames * REGION_MAX * sizeof(uint64_t), (hipStream_t)stream);
    if (e != hipSuccess) return VV_HIP_STATUS(e);
  }
  const int hw = h * w;
  if (hw == 0) return VV_OK;
  const int per = 256 * LINK_PER_THREAD;
  const int tiles = (int)(((int64_t)hw + per - 1) / per);
  for (int f0 = 0; f0 < n_frames; f0 += 65535) {                    // gridDim.y
    VV_LAUNCH(region_links_kernel, dim3(tiles, min(65535, n_frames - f0)), dim3(256), 0, (hipStream_t)stream, prev_labels, labels,
              same_video, f0, hw, reinterpret_cast<unsigned long long*>(links));
    VV_CHECK_LAUNCH();
  }
  return VV_OK;
}
