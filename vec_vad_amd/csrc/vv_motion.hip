// Motion-based foreground localisation (reference fore_det/obj_det_with_motion.py:144-223 get_mt_bboxes), two stages:
//   vv_motion_mask : Gaussian blur of the frames of N windows, |a-b| + |b-c| (uint8 wrap), threshold, erase of the appearance
//                    boxes, any-channel -> one 0/255 mask per window.  One launch; a workgroup owns a 16x64 pixel tile and walks the
//                    N windows with three blurred tiles cached in LDS, so a frame shared by neighbouring windows is blurred once per
//                    tile and the blurred planes never exist in HBM.
//   vv_mask_boxes  : cv2.findContours(RETR_EXTERNAL) + boundingRect + the reference's filter, as connected-component labelling:
//                    foreground 8-connected, background 4-connected, min-rooted union-find (tile-local in LDS, tile borders merged
//                    with atomicMin), bounding rectangles by atomicMin / atomicMax, compaction by ranking the surviving labels.
// Everything is integer arithmetic and every cross-thread result is a min, a max or an or: outputs do not depend on scheduling.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

constexpr int TILE_H = 16, TILE_W = 64;      // pixels per workgroup tile: 256 threads x 4 consecutive pixels of a row
constexpr int AP_CAP = 64;                   // appearance boxes of one window kept in LDS per tile (more: read from HBM)
constexpr int CHUNK = 1024;                  // pixels per workgroup in the compaction passes

__device__ __forceinline__ int reflect101(const int i, const int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// ------------------------------------------------------------------------------------------------------------------------
// stage 1
template <int C, int R>
struct MotionLds {
  static constexpr int TWC = TILE_W * C;                                 // bytes of a tile row
  static constexpr int ROWS = TILE_H + 2 * R;
  static constexpr int RS = (((TILE_W + 2 * R) * C + 3 + 3) / 4) * 4;    // raw row stride: halo + up to 3 bytes of misalignment
  uint32_t raw[ROWS * RS / 4];
  uint16_t hs[ROWS * TWC];                                               // horizontal pass, un-normalised
  uint32_t slot[3][TILE_H * TWC / 4];                                    // blurred tiles of three frames
  int ap[AP_CAP][4];
  int nap;
};

// blurred tile of frame f -> L.slot[s].  cv2's fixed kernels for sigma = 0, BORDER_REFLECT_101, one rounding after both passes.
template <int C, int R>
__device__ void blur_tile(MotionLds<C, R>& L, const uint8_t* __restrict__ frames, const int64_t total, const int f, const int H,
                          const int W, const int x0, const int y0, const int s, const int tid) {
  using M = MotionLds<C, R>;
  constexpr int TWC = M::TWC, RS = M::RS, DW = RS / 4;
  const int WC = W * C;
  const int xa = max(0, x0 - R), xb = min(W, x0 + TILE_W + R);
  const int ya = max(0, y0 - R), yb = min(H, y0 + TILE_H + R);
  const int nrows = yb - ya, rowbytes = (xb - xa) * C;
  const int64_t fbase = (int64_t)f * H * WC + xa * C;
  // in-image bytes of the halo tile, as aligned dwords (a row starts up to 3 bytes into its first dword)
  for (int it = tid; it < nrows * DW; it += VV_WG) {
    const int rr = it / DW, d = it % DW, y = ya + rr;
    const int64_t gb = fbase + (int64_t)y * WC;
    const int sh = (int)(gb & 3);
    if (4 * d < sh + rowbytes) {
      const int64_t ga = gb - sh + 4 * d;
      uint32_t v = 0;
      if (ga + 4 <= total) {
        v = *reinterpret_cast<const uint32_t*>(frames + ga);
      } else {
        for (int b = 0; b < 4; ++b)
          if (ga + b < total) v |= (uint32_t)frames[ga + b] << (8 * b);
      }
      L.raw[(y - (y0 - R)) * DW + d] = v;
    }
  }
  __syncthreads();
  constexpr int w0 = 1, w1 = R == 1 ? 2 : 4, w2 = 6;
  const uint8_t* rawb = reinterpret_cast<const uint8_t*>(L.raw);
  for (int it = tid; it < nrows * TWC; it += VV_WG) {
    const int rr = it / TWC, j = it % TWC, y = ya + rr, c = j % C, x = x0 + j / C;
    if (x < W) {
      const int sh = (int)((fbase + (int64_t)y * WC) & 3);
      const uint8_t* row = rawb + (y - (y0 - R)) * RS + sh + c;
      int S;
      if constexpr (R == 1) {
        S = w0 * (row[(reflect101(x - 1, W) - xa) * C] + row[(reflect101(x + 1, W) - xa) * C]) + w1 * row[(x - xa) * C];
      } else {
        S = w0 * (row[(reflect101(x - 2, W) - xa) * C] + row[(reflect101(x + 2, W) - xa) * C]) +
            w1 * (row[(reflect101(x - 1, W) - xa) * C] + row[(reflect101(x + 1, W) - xa) * C]) + w2 * row[(x - xa) * C];
      }
      L.hs[(y - (y0 - R)) * TWC + j] = (uint16_t)S;
    }
  }
  __syncthreads();
  uint8_t* out = reinterpret_cast<uint8_t*>(L.slot[s]);
  for (int it = tid; it < TILE_H * TWC; it += VV_WG) {
    const int yl = it / TWC, j = it % TWC, y = y0 + yl, x = x0 + j / C;
    int v = 0;
    if (y < H && x < W) {
      const uint16_t* col = L.hs + j - (y0 - R) * TWC;
      if constexpr (R == 1) {
        v = (w0 * (col[reflect101(y - 1, H) * TWC] + col[reflect101(y + 1, H) * TWC]) + w1 * col[y * TWC] + 8) >> 4;
      } else {
        v = (w0 * (col[reflect101(y - 2, H) * TWC] + col[reflect101(y + 2, H) * TWC]) +
             w1 * (col[reflect101(y - 1, H) * TWC] + col[reflect101(y + 1, H) * TWC]) + w2 * col[y * TWC] + 128) >> 8;
      }
    }
    out[it] = (uint8_t)v;
  }
  __syncthreads();
}

template <int C, int R>
__global__ void __launch_bounds__(VV_WG) motion_mask_kernel(const uint8_t* __restrict__ frames, const int F, const int H, const int W,
                                                            const int32_t* __restrict__ win, const int N, const int thr,
                                                            const int32_t* __restrict__ ap, const int M, const int extend,
                                                            uint8_t* __restrict__ mask) {
  using ML = MotionLds<C, R>;
  __shared__ ML L;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
  const int64_t total = (int64_t)F * H * W * C;
  const int yl = tid / (TILE_W / 4), xg = tid % (TILE_W / 4);
  const int y = y0 + yl, x = x0 + 4 * xg;
  int tag[3] = {-1, -1, -1};                         // frame held by each slot: the same in every thread
  for (int n = 0; n < N; ++n) {
    __syncthreads();                                 // the previous window's reads of slots and box list are done
    int f[3], s[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) f[j] = min(max(win[3 * n + j], 0), F - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      int sj = tag[0] == f[j] ? 0 : (tag[1] == f[j] ? 1 : (tag[2] == f[j] ? 2 : -1));
      if (sj < 0) {                                  // block-uniform: evict a slot this window does not read
        auto needed = [&](const int t) { return t == f[0] || t == f[1] || t == f[2]; };
        sj = !needed(tag[0]) ? 0 : (!needed(tag[1]) ? 1 : 2);
        blur_tile<C, R>(L, frames, total, f[j], H, W, x0, y0, sj, tid);
        if (sj == 0) tag[0] = f[j]; else if (sj == 1) tag[1] = f[j]; else tag[2] = f[j];
      }
      s[j] = sj;
    }
    // erase rectangles of this window that touch the tile
    if (tid == 0) L.nap = 0;
    __syncthreads();
    for (int m = tid; m < M; m += VV_WG) {
      if (ap[5 * m] != n) continue;
      const int bx1 = max(0, ap[5 * m + 1] - extend), by1 = max(0, ap[5 * m + 2] - extend);
      const int bx2 = min(ap[5 * m + 3] + extend, W), by2 = min(ap[5 * m + 4] + extend, H);
      if (bx1 > bx2 || by1 > by2 || bx2 < x0 || bx1 >= x0 + TILE_W || by2 < y0 || by1 >= y0 + TILE_H) continue;
      const int k = atomicAdd(&L.nap, 1);
      if (k < AP_CAP) { L.ap[k][0] = bx1; L.ap[k][1] = by1; L.ap[k][2] = bx2; L.ap[k][3] = by2; }
    }
    __syncthreads();
    const int nap = L.nap;
    if (y < H && x < W) {
      uint32_t a[C], b[C], c[C];
      const int o = (yl * ML::TWC + xg * 4 * C) / 4;
#pragma unroll
      for (int k = 0; k < C; ++k) { a[k] = L.slot[s[0]][o + k]; b[k] = L.slot[s[1]][o + k]; c[k] = L.slot[s[2]][o + k]; }
      uint32_t outw = 0;
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        bool set = false;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const int i = px * C + ch, sh = (i & 3) * 8;
          const int va = (a[i >> 2] >> sh) & 255, vb = (b[i >> 2] >> sh) & 255, vc = (c[i >> 2] >> sh) & 255;
          const int d = (abs(va - vb) + abs(vb - vc)) & 255;            // numpy adds two uint8 arrays: modulo 256
          set |= d > thr;
        }
        const int xx = x + px;
        if (set) {
          if (nap <= AP_CAP) {
            for (int k = 0; k < nap; ++k)
              if (xx >= L.ap[k][0] && xx <= L.ap[k][2] && y >= L.ap[k][1] && y <= L.ap[k][3]) set = false;
          } else {
            for (int m = 0; m < M; ++m)
              if (ap[5 * m] == n && xx >= max(0, ap[5 * m + 1] - extend) && xx <= min(ap[5 * m + 3] + extend, W) &&
                  y >= max(0, ap[5 * m + 2] - extend) && y <= min(ap[5 * m + 4] + extend, H))
                set = false;
          }
        }
        if (set) outw |= 0xFFu << (8 * px);
      }
      uint8_t* dst = mask + ((int64_t)n * H + y) * W + x;
      if ((W & 3) == 0) {
        *reinterpret_cast<uint32_t*>(dst) = outw;
      } else {
        for (int px = 0; px < 4; ++px)
          if (x + px < W) dst[px] = (uint8_t)(outw >> (8 * px));
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// stage 2: min-rooted union-find.  A parent is always a smaller index of the same set, so a stale read is still an ancestor.
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int* L, int i) {
  int p;
  while ((p = uf_load(L + i)) != i) i = p;
  return i;
}

__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a);
    b = uf_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(L + a, b);            // hang the larger root under the smaller one
    if (old == a) return;
    a = old;                                        // someone re-parented a first: its old parent still has to meet b
  }
}

struct Px4 {
  int v[4];
};

// the 4 mask bytes of a thread (x .. x+3 of row y of window n); out of the image: -1
__device__ __forceinline__ Px4 load_px4(const uint8_t* __restrict__ m, const int H, const int W, const int y, const int x) {
  Px4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) r.v[k] = -1;
  if (y < H && x < W) {
    const uint8_t* p = m + (int64_t)y * W + x;
    if ((W & 3) == 0) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
      for (int k = 0; k < 4; ++k) r.v[k] = ((w >> (8 * k)) & 255) != 0;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) r.v[k] = p[k] != 0;
    }
  }
  return r;
}

// labels [N][HW+1] (entry HW: the virtual background ring round the frame), stats [N][HW][4] = min x, max x, max y, external
__global__ void __launch_bounds__(VV_WG) ccl_local_kernel(const uint8_t* __restrict__ mask, const int H, const int W,
                                                          int* __restrict__ labels, int4* __restrict__ stats) {
  __shared__ int8_t cls[TILE_H * TILE_W];
  __shared__ int lab[TILE_H * TILE_W];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int HW = H * W;
  const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
  const int yl = tid / (TILE_W / 4), xl0 = (tid % (TILE_W / 4)) * 4;
  const int y = y0 + yl, x = x0 + xl0;
  const Px4 v = load_px4(mask + (int64_t)n * HW, H, W, y, x);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cls[yl * TILE_W + xl0 + k] = (int8_t)v.v[k];
    lab[yl * TILE_W + xl0 + k] = yl * TILE_W + xl0 + k;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = v.v[k], xl = xl0 + k, i = yl * TILE_W + xl;
    if (c < 0) continue;
    if (xl > 0 && cls[i - 1] == c) uf_union(lab, i, i - 1);
    if (yl > 0) {
      if (cls[i - TILE_W] == c) uf_union(lab, i, i - TILE_W);
      if (c == 1) {                                 // foreground is 8-connected
        if (xl > 0 && cls[i - TILE_W - 1] == 1) uf_union(lab, i, i - TILE_W - 1);
        if (xl < TILE_W - 1 && cls[i - TILE_W + 1] == 1) uf_union(lab, i, i - TILE_W + 1);
      }
    }
  }
  __syncthreads();
  int* Ln = labels + (int64_t)n * (HW + 1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (v.v[k] < 0) continue;
    const int r = uf_find(lab, yl * TILE_W + xl0 + k);         // tile raster order = frame raster order: the minimum carries over
    const int p = y * W + x + k;
    Ln[p] = (y0 + r / TILE_W) * W + x0 + r % TILE_W;
    stats[(int64_t)n * HW + p] = make_int4(W, -1, -1, 0);
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) Ln[HW] = HW;
}

// unions across tile borders, and of every background pixel on the frame edge with the virtual ring
__global__ void __launch_bounds__(VV_WG) ccl_border_kernel(const uint8_t* __restrict__ mask, const int H, const int W,
                                                           int* __restrict__ labels) {
  const int HW = H * W, n = blockIdx.y;
  const int p = blockIdx.x * VV_WG + threadIdx.x;
  if (p >= HW) return;
  const int y = p / W, x = p % W;
  const bool top = y % TILE_H == 0 && y > 0, left = x % TILE_W == 0 && x > 0;
  const bool right = x % TILE_W == TILE_W - 1 && x < W - 1 && y > 0;
  const bool edge = x == 0 || y == 0 || x == W - 1 || y == H - 1;
  if (!(top || left || right || edge)) return;
  const uint8_t* m = mask + (int64_t)n * HW;
  int* L = labels + (int64_t)n * (HW + 1);
  if (m[p]) {
    if (top) {
      if (m[p - W]) uf_union(L, p, p - W);
      if (x > 0 && m[p - W - 1]) uf_union(L, p, p - W - 1);
      if (x < W - 1 && m[p - W + 1]) uf_union(L, p, p - W + 1);
    }
    if (left) {
      if (m[p - 1]) uf_union(L, p, p - 1);
      if (y > 0 && !top && m[p - W - 1]) uf_union(L, p, p - W - 1);
    }
    if (right && !top && m[p - W + 1]) uf_union(L, p, p - W + 1);
  } else {
    if (top && !m[p - W]) uf_union(L, p, p - W);
    if (left && !m[p - 1]) uf_union(L, p, p - 1);
    if (edge) uf_union(L, HW, p);
  }
}

// bounding rectangle and externality of every foreground component, accumulated at its root
__global__ void __launch_bounds__(VV_WG) ccl_stats_kernel(const uint8_t* __restrict__ mask, const int H, const int W,
                                                          const int* __restrict__ labels, int* __restrict__ stats) {
  const int HW = H * W, n = blockIdx.y;
  const int p = blockIdx.x * VV_WG + threadIdx.x;
  if (p >= HW) return;
  const uint8_t* m = mask + (int64_t)n * HW;
  if (!m[p]) return;
  const int* L = labels + (int64_t)n * (HW + 1);
  const int y = p / W, x = p % W;
  const int r = uf_find(L, p);
  int* S = stats + ((int64_t)n * HW + r) * 4;
  // the fields only ever move one way, so a read that already covers this pixel makes the atomic unnecessary
  if (x < uf_load(S + 0)) atomicMin(S + 0, x);
  if (x > uf_load(S + 1)) atomicMax(S + 1, x);
  if (y > uf_load(S + 2)) atomicMax(S + 2, y);
  if (uf_load(S + 3) == 0) {
    bool ext = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    if (!ext) {                                     // 4-adjacent to the background region that reaches the frame edge
      const int ring = uf_find(L, HW);
      ext = (!m[p - 1] && uf_find(L, p - 1) == ring) || (!m[p + 1] && uf_find(L, p + 1) == ring) ||
            (!m[p - W] && uf_find(L, p - W) == ring) || (!m[p + W] && uf_find(L, p + W) == ring);
    }
    if (ext) atomicMax(S + 3, 1);
  }
}

// is pixel p the root of an external foreground component that passes the reference's size filter; its box if so
__device__ __forceinline__ bool survivor(const uint8_t* __restrict__ m, const int* __restrict__ L, const int4* __restrict__ S,
                                         const int p, const int H, const int W, const int area_thr, const int extend, int4& box) {
  if (L[p] != p || !m[p]) return false;
  const int4 s = S[p];
  if (!s.w) return false;
  const int bx = s.x, by = p / W, w = s.y - s.x + 1, h = s.z - by + 1;
  if (!((int64_t)(w + 1) * (h + 1) > area_thr && w < 10 * h && h < 10 * w)) return false;
  box = make_int4(max(0, bx - extend), max(0, by - extend), min(bx + w + extend, W), min(by + h + extend, H));
  return true;
}

__global__ void __launch_bounds__(VV_WG) ccl_count_kernel(const uint8_t* __restrict__ mask, const int H, const int W,
                                                          const int* __restrict__ labels, const int4* __restrict__ stats,
                                                          const int area_thr, const int extend, int* __restrict__ cnt) {
  __shared__ int sh[VV_WG];
  const int HW = H * W, n = blockIdx.y, tid = threadIdx.x;
  const uint8_t* m = mask + (int64_t)n * HW;
  const int* L = labels + (int64_t)n * (HW + 1);
  const int4* S = stats + (int64_t)n * HW;
  int c = 0;
  int4 box;
  for (int k = 0; k < 4; ++k) {
    const int p = blockIdx.x * CHUNK + 4 * tid + k;
    if (p < HW && survivor(m, L, S, p, H, W, area_thr, extend, box)) ++c;
  }
  sh[tid] = c;
  __syncthreads();
  for (int d = VV_WG / 2; d > 0; d >>= 1) {
    if (tid < d) sh[tid] += sh[tid + d];
    __syncthreads();
  }
  if (tid == 0) cnt[n * gridDim.x + blockIdx.x] = sh[0];
}

// position of a surviving box = number of surviving labels above it: descending label order, independent of scheduling
__global__ void __launch_bounds__(VV_WG) ccl_emit_kernel(const uint8_t* __restrict__ mask, const int H, const int W,
                                                         const int* __restrict__ labels, const int4* __restrict__ stats,
                                                         const int area_thr, const int extend, const int* __restrict__ cnt,
                                                         const int cap, int* __restrict__ count, int4* __restrict__ boxes) {
  __shared__ int sh[VV_WG];
  __shared__ int base_sh;
  const int HW = H * W, n = blockIdx.y, tid = threadIdx.x, nchunk = gridDim.x;
  const uint8_t* m = mask + (int64_t)n * HW;
  const int* L = labels + (int64_t)n * (HW + 1);
  const int4* S = stats + (int64_t)n * HW;
  int above = 0;                                    // survivors in the chunks after this one
  for (int k = blockIdx.x + 1 + tid; k < nchunk; k += VV_WG) above += cnt[n * nchunk + k];
  sh[tid] = above;
  __syncthreads();
  for (int d = VV_WG / 2; d > 0; d >>= 1) {
    if (tid < d) sh[tid] += sh[tid + d];
    __syncthreads();
  }
  if (tid == 0) base_sh = sh[0];
  __syncthreads();
  const int base = base_sh;
  int4 box[4];
  bool ok[4];
  int c = 0;
  for (int k = 0; k < 4; ++k) {
    const int p = blockIdx.x * CHUNK + 4 * tid + k;
    ok[k] = p < HW && survivor(m, L, S, p, H, W, area_thr, extend, box[k]);
    c += ok[k];
  }
  // inclusive suffix sum over threads: sh[t] = survivors of threads t .. 255
  sh[tid] = c;
  __syncthreads();
  for (int d = 1; d < VV_WG; d <<= 1) {
    const int add = tid + d < VV_WG ? sh[tid + d] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  int pos = base + sh[tid] - c;                     // survivors of the threads after this one
  for (int k = 3; k >= 0; --k) {
    if (ok[k]) {
      if (pos < cap) boxes[(int64_t)n * cap + pos] = box[k];
      ++pos;
    }
  }
  if (blockIdx.x == 0 && tid == 0) count[n] = base + sh[0];
}

inline int64_t align16(const int64_t v) { return (v + 15) & ~(int64_t)15; }

}  // namespace

extern "C" int vv_motion_mask(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* win, int32_t N,
                              int32_t ksize, int32_t binary_thr, const int32_t* ap, int32_t M, int32_t extend, uint8_t* mask,
                              vv_stream stream) {
  if (!frames || !win || !mask || F <= 0 || N < 0 || M < 0 || (M > 0 && !ap) || extend < 0) return VV_ERR_BAD_ARG;
  if ((C != 1 && C != 3) || (ksize != 3 && ksize != 5)) return VV_ERR_UNSUPPORTED;
  if (H <= ksize / 2 || W <= ksize / 2 || (int64_t)H * W > 0x3fffffff) return VV_ERR_BAD_ARG;       // one reflection must suffice
  if (((uintptr_t)frames & 3) || ((uintptr_t)mask & 3)) return VV_ERR_BAD_ARG;
  if (N == 0) return VV_OK;
  const dim3 grid((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H);
  if (grid.y > 65535) return VV_ERR_BAD_ARG;
#define VV_MM(CC, RR)                                                                                                            \
  VV_LAUNCH((motion_mask_kernel<CC, RR>), grid, dim3(VV_WG), 0, (hipStream_t)stream, frames, F, H, W, win, N, binary_thr, ap, M, \
            extend, mask)
  if (C == 1 && ksize == 3) VV_MM(1, 1);
  else if (C == 1) VV_MM(1, 2);
  else if (ksize == 3) VV_MM(3, 1);
  else VV_MM(3, 2);
#undef VV_MM
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int64_t vv_mask_boxes_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  const int64_t HW = (int64_t)H * W, nchunk = (HW + CHUNK - 1) / CHUNK;
  return align16(4 * (int64_t)N * (HW + 1)) + 16 * (int64_t)N * HW + align16(4 * (int64_t)N * nchunk);
}

extern "C" int vv_mask_boxes(const uint8_t* mask, int32_t N, int32_t H, int32_t W, int32_t area_thr, int32_t extend, int32_t cap,
                             void* workspace, int64_t workspace_bytes, int32_t* count, int32_t* boxes, vv_stream stream) {
  if (!mask || !count || !boxes || N < 0 || H <= 0 || W <= 0 || cap <= 0 || extend < 0) return VV_ERR_BAD_ARG;
  if ((int64_t)H * W > 0x3fffffff || N > 65535) return VV_ERR_BAD_ARG;
  if (N == 0) return VV_OK;
  if (!workspace || workspace_bytes < vv_mask_boxes_workspace_bytes(N, H, W)) return VV_ERR_BAD_ARG;
  if (((uintptr_t)mask & 3) || ((uintptr_t)workspace & 15) || ((uintptr_t)boxes & 15)) return VV_ERR_BAD_ARG;
  const int HW = H * W, nchunk = (HW + CHUNK - 1) / CHUNK;
  if ((int64_t)N * nchunk > 0x7fffffff) return VV_ERR_BAD_ARG;
  char* ws = (char*)workspace;
  int* labels = (int*)ws;
  int4* stats = (int4*)(ws + align16(4 * (int64_t)N * (HW + 1)));
  int* cnt = (int*)((char*)stats + 16 * (int64_t)N * HW);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 tiles((W + TILE_W - 1) / TILE_W, (H + TILE_H - 1) / TILE_H, N);
  if (tiles.y > 65535) return VV_ERR_BAD_ARG;
  const dim3 pix((HW + VV_WG - 1) / VV_WG, N), chunks(nchunk, N);
  VV_LAUNCH(ccl_local_kernel, tiles, dim3(VV_WG), 0, st, mask, H, W, labels, stats);
  VV_CHECK_LAUNCH();
  VV_LAUNCH(ccl_border_kernel, pix, dim3(VV_WG), 0, st, mask, H, W, labels);
  VV_CHECK_LAUNCH();
  VV_LAUNCH(ccl_stats_kernel, pix, dim3(VV_WG), 0, st, mask, H, W, (const int*)labels, (int*)stats);
  VV_CHECK_LAUNCH();
  VV_LAUNCH(ccl_count_kernel, chunks, dim3(VV_WG), 0, st, mask, H, W, (const int*)labels, (const int4*)stats, area_thr, extend, cnt);
  VV_CHECK_LAUNCH();
  VV_LAUNCH(ccl_emit_kernel, chunks, dim3(VV_WG), 0, st, mask, H, W, (const int*)labels, (const int4*)stats, area_thr, extend,
            (const int*)cnt, cap, count, (int4*)boxes);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
