// Pictures a person can look at ([mi355x] render): the two entry points of include/vecvad_hip.h, vv_flow_color and vv_render_overlay.
//   flow_rad_kernel: one workgroup per FC_TILE pixels of one image takes the maximum of sqrt(u*u + v*v) (float32, product and sum
//     rounded separately; unknown and NaN pixels count as (0,0)) and leaves it as one partial per workgroup.  A maximum does not round,
//     so the order it is taken in does not show: bit-identical run to run, no atomics.  The partials of an image are its own.
//   flow_color_kernel: every workgroup first takes the maximum of its image's partials (a few dozen floats at 240x360), then colours
//     its pixels: Middlebury wheel in constant memory, float32 arithmetic, three bytes per pixel.
//   overlay_kernel: vv_paint_masks' layout -- a thread owns OV_PIX consecutive pixels of the frame taken as a flat h*w array and walks
//     the frame's boxes, staged in LDS OV_PASS at a time (every lane reads the same box: broadcast) -- with the colour table in LDS.
//     Per pixel 8 bytes of mask, 1 or 3 of frame and 1 of ground truth come in and 3 bytes go out; the 12 bytes of a thread leave as
//     three dwords when the frame's first byte is dword aligned.  Integer arithmetic and single IEEE double operations only: exact.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

// ---- Middlebury colour wheel, from the published description (Baker et al., "A Database and Evaluation Methodology for Optical
// Flow", IJCV 2011, and the flow-code it ships): six segments RY 15, YG 6, GC 4, CB 11, BM 13, MR 6; inside a segment of n entries
// one channel ramps as floor(255 * i / n), up or down, and the other two stay at 0 or 255 -------------------------------------------
constexpr int FC_NCOLS = 55;
__constant__ uint8_t fc_wheel[FC_NCOLS][3] = {
    // RY: red -> yellow, green up
    {255, 0, 0}, {255, 17, 0}, {255, 34, 0}, {255, 51, 0}, {255, 68, 0}, {255, 85, 0}, {255, 102, 0}, {255, 119, 0}, {255, 136, 0},
    {255, 153, 0}, {255, 170, 0}, {255, 187, 0}, {255, 204, 0}, {255, 221, 0}, {255, 238, 0},
    // YG: yellow -> green, red down
    {255, 255, 0}, {213, 255, 0}, {170, 255, 0}, {128, 255, 0}, {85, 255, 0}, {43, 255, 0},
    // GC: green -> cyan, blue up
    {0, 255, 0}, {0, 255, 63}, {0, 255, 127}, {0, 255, 191},
    // CB: cyan -> blue, green down
    {0, 255, 255}, {0, 232, 255}, {0, 209, 255}, {0, 186, 255}, {0, 163, 255}, {0, 140, 255}, {0, 116, 255}, {0, 93, 255},
    {0, 70, 255}, {0, 47, 255}, {0, 24, 255},
    // BM: blue -> magenta, red up
    {0, 0, 255}, {19, 0, 255}, {39, 0, 255}, {58, 0, 255}, {78, 0, 255}, {98, 0, 255}, {117, 0, 255}, {137, 0, 255}, {156, 0, 255},
    {176, 0, 255}, {196, 0, 255}, {215, 0, 255}, {235, 0, 255},
    // MR: magenta -> red, blue down
    {255, 0, 255}, {255, 0, 213}, {255, 0, 170}, {255, 0, 128}, {255, 0, 85}, {255, 0, 43}};

constexpr int FC_PIX = 16;                     // pixels per thread of the maximum pass
constexpr int FC_TILE = FC_PIX * VV_WG;        // 4096 pixels per partial
constexpr float FC_UNKNOWN = 1e7f;             // |u| or |v| above it: an unknown pixel
constexpr float FC_EPS = 2.220446049250313e-16f;      // 2^-52, what the float64 original adds to the radius
constexpr float FC_PI = 3.14159265358979323846f;

// (u, v) of a pixel as the colouring sees it: unknown and NaN pixels are (0, 0), and `known` says which they were
__device__ __forceinline__ bool fc_known(float& u, float& v) {
  const bool known = fabsf(u) <= FC_UNKNOWN && fabsf(v) <= FC_UNKNOWN;      // false for a NaN as well
  if (!known) u = v = 0.0f;
  return known;
}

__device__ __forceinline__ float fc_block_max(float best, float* wmax) {
  for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_down(best, o));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = best;
  __syncthreads();
  best = wmax[0];
  for (int k = 1; k < VV_WG / 64; ++k) best = fmaxf(best, wmax[k]);
  return best;                                 // the same value in every thread
}

__global__ void __launch_bounds__(VV_WG)
flow_rad_kernel(const float2* __restrict__ flow, const int hw, const int nblk, float* __restrict__ partial) {
  __shared__ float wmax[VV_WG / 64];
  const int img = blockIdx.y, blk = blockIdx.x;
  const float2* fl = flow + (int64_t)img * hw;
  float best = -1.0f;                          // max(-1, ...)
  const int p0 = blk * FC_TILE + threadIdx.x;
#pragma unroll 4
  for (int k = 0; k < FC_PIX; ++k) {
    const int p = p0 + k * VV_WG;
    if (p < hw) {
      float2 uv = fl[p];
      fc_known(uv.x, uv.y);
      best = fmaxf(best, __fsqrt_rn(__fadd_rn(__fmul_rn(uv.x, uv.x), __fmul_rn(uv.y, uv.y))));
    }
  }
  best = fc_block_max(best, wmax);
  if (threadIdx.x == 0) partial[(int64_t)img * nblk + blk] = best;
}

__global__ void __launch_bounds__(VV_WG)
flow_color_kernel(const float2* __restrict__ flow, const int hw, const int nblk, const int cblk, const float maxrad,
                  const float* __restrict__ partial, uint8_t* __restrict__ out) {
  __shared__ float wmax[VV_WG / 64];
  const int img = blockIdx.x / cblk, blk = blockIdx.x - img * cblk;
  float R = maxrad;
  if (!(maxrad > 0.0f)) {                      // per-image mode: the maximum of this image's partials
    float best = -1.0f;
    for (int i = threadIdx.x; i < nblk; i += VV_WG) best = fmaxf(best, partial[(int64_t)img * nblk + i]);
    R = fc_block_max(best, wmax);
  }
  const int p = blk * VV_WG + threadIdx.x;
  if (p >= hw) return;
  float2 uv = flow[(int64_t)img * hw + p];
  const bool known = fc_known(uv.x, uv.y);
  uint8_t* o = out + ((int64_t)img * hw + p) * 3;
  if (!known) {
    o[0] = o[1] = o[2] = 0;
    return;
  }
  const float den = R + FC_EPS;
  const float u = uv.x / den, v = uv.y / den;
  const float rad = __fsqrt_rn(u * u + v * v);
  const float a = atan2f(-v, -u) / FC_PI;      // the sign of a zero v picks the end of the wheel: atan2(-/+0, -u) = -/+pi for u > 0
  const float fk = (a + 1.0f) / 2.0f * (float)(FC_NCOLS - 1) + 1.0f;
  int k0 = (int)floorf(fk);
  k0 = k0 < 1 ? 1 : (k0 > FC_NCOLS ? FC_NCOLS : k0);      // 1..55 already; the clamp only protects the table
  const int k1 = k0 == FC_NCOLS ? 1 : k0 + 1;
  const float f = fk - (float)k0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float col = (1.0f - f) * ((float)fc_wheel[k0 - 1][c] / 255.0f) + f * ((float)fc_wheel[k1 - 1][c] / 255.0f);
    col = rad <= 1.0f ? 1.0f - rad * (1.0f - col) : col * 0.75f;
    const int level = (int)floorf(255.0f * col);
    o[c] = (uint8_t)(level < 0 ? 0 : (level > 255 ? 255 : level));
  }
}

// ---- overlay ------------------------------------------------------------------------------------------------------------------------
constexpr int OV_PASS = 256;                   // boxes per LDS pass = threads of the workgroup
constexpr int OV_PIX = 4;                      // consecutive pixels per thread: 12 output bytes
constexpr int OV_TILE = OV_PIX * VV_WG;        // pixels per workgroup
constexpr double OV_BG = VV_RENDER_UNPAINTED;

// the level of a value: 0 at or below lo, 255 at or above hi, floor((v - lo) / (hi - lo) * 255) between, every operation rounded once
__device__ __forceinline__ int ov_level(double v, double lo, double hi) {
  if (v <= lo) return 0;
  if (v >= hi) return 255;
  const int q = (int)floor(__dmul_rn(__ddiv_rn(__dsub_rn(v, lo), __dsub_rn(hi, lo)), 255.0));
  return q < 0 ? 0 : (q > 255 ? 255 : q);      // 0..255 already (a NaN lands on 0); the clamp only protects the table
}

__global__ void __launch_bounds__(VV_WG)
overlay_kernel(const uint8_t* __restrict__ frames, const int c, const int bgr, const double* __restrict__ mask,
               const uint8_t* __restrict__ gt, const int4* __restrict__ rects, const double* __restrict__ scores,
               const int32_t* __restrict__ frame_off, const uint8_t* __restrict__ lut, const double lo, const double hi,
               const int alpha, const int f0, const int h, const int w, uint8_t* __restrict__ out) {
  __shared__ int4 srect[OV_PASS];
  __shared__ double ssc[OV_PASS];
  __shared__ uint8_t slut[256 * 3];
  for (int i = threadIdx.x; i < 256 * 3; i += VV_WG) slut[i] = lut[i];
  const int f = f0 + blockIdx.y;
  const int hw = h * w;
  const int m0 = frame_off ? frame_off[f] : 0, m1 = frame_off ? frame_off[f + 1] : 0;
  const int p0 = blockIdx.x * OV_TILE + OV_PIX * (int)threadIdx.x;
  int y[OV_PIX], x[OV_PIX];
  bool edge[OV_PIX];
  double best[OV_PIX];
#pragma unroll
  for (int k = 0; k < OV_PIX; ++k) {
    const int p = p0 + k;
    y[k] = p < hw ? p / w : -1;                // a pixel past the frame lies in no box
    x[k] = p < hw ? p - y[k] * w : -1;
    edge[k] = false;
    best[k] = 0.0;
  }
  for (int base = m0; base < m1; base += OV_PASS) {
    const int cnt = min(OV_PASS, m1 - base);
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
      srect[threadIdx.x] = rects[base + threadIdx.x];
      ssc[threadIdx.x] = scores[base + threadIdx.x];
    }
    __syncthreads();
    for (int b = 0; b < cnt; ++b) {
      const int4 r = srect[b];                 // y0, y1, x0, x1
      if (r.y <= r.x || r.w <= r.z) continue;  // an empty rectangle has no outline (wave-uniform)
      const double s = ssc[b];
#pragma unroll
      for (int k = 0; k < OV_PIX; ++k) {
        const bool in = y[k] >= r.x && y[k] < r.y && x[k] >= r.z && x[k] < r.w;
        const bool on = in && (y[k] == r.x || y[k] == r.y - 1 || x[k] == r.z || x[k] == r.w - 1);
        if (on) {
          best[k] = edge[k] ? fmax(best[k], s) : s;
          edge[k] = true;
        }
      }
    }
  }
  __syncthreads();                             // the colour table (and, without boxes, nothing else) is in LDS
  const int64_t fbase = (int64_t)f * hw;
  uint8_t px[OV_PIX * 3];
#pragma unroll
  for (int k = 0; k < OV_PIX; ++k) {
    const int p = p0 + k;
    int r = 0, g = 0, b = 0;
    if (p < hw) {
      const int64_t i = fbase + p;
      if (c == 1) {
        r = g = b = frames[i];
      } else {
        const uint8_t* s3 = frames + i * 3;
        r = s3[bgr ? 2 : 0]; g = s3[1]; b = s3[bgr ? 0 : 2];
      }
      const double mv = mask[i];
      if (mv != OV_BG) {
        const uint8_t* t = slut + 3 * ov_level(mv, lo, hi);
        r = (r * (256 - alpha) + t[0] * alpha + 128) >> 8;
        g = (g * (256 - alpha) + t[1] * alpha + 128) >> 8;
        b = (b * (256 - alpha) + t[2] * alpha + 128) >> 8;
      }
      if (edge[k]) {
        const uint8_t* t = slut + 3 * ov_level(best[k], lo, hi);
        r = t[0]; g = t[1]; b = t[2];
      }
      if (gt && gt[i]) {                       // a ground-truth pixel with a 4-neighbour that is zero or outside the frame
        const int yy = y[k], xx = x[k];
        const bool border = yy == 0 || yy == h - 1 || xx == 0 || xx == w - 1;
        if (border || !gt[i - w] || !gt[i + w] || !gt[i - 1] || !gt[i + 1]) r = g = b = 255;
      }
    }
    px[3 * k] = (uint8_t)r; px[3 * k + 1] = (uint8_t)g; px[3 * k + 2] = (uint8_t)b;
  }
  uint8_t* o = out + (fbase + p0) * 3;
  if (p0 + OV_PIX <= hw && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
  } else {
#pragma unroll
    for (int k = 0; k < OV_PIX; ++k) {
      if (p0 + k < hw) {
        o[3 * k] = px[3 * k]; o[3 * k + 1] = px[3 * k + 1]; o[3 * k + 2] = px[3 * k + 2];
      }
    }
  }
}

bool fc_sizes_ok(int32_t n, int32_t h, int32_t w) { return n >= 0 && h >= 0 && w >= 0 && (int64_t)h * w <= INT32_MAX - FC_TILE; }

}  // namespace

// work: the partial maxima, float [n][ceil(h*w / 4096)]
extern "C" int64_t vv_flow_color_work(int32_t n, int32_t h, int32_t w) {
  if (!fc_sizes_ok(n, h, w)) return -1;
  const int64_t hw = (int64_t)h * w;
  return (int64_t)n * ((hw + FC_TILE - 1) / FC_TILE) * 4;
}

extern "C" int vv_flow_color(const float* flow, int32_t n, int32_t h, int32_t w, float maxrad, uint8_t* out, void* work,
                             vv_stream stream) {
  if (!fc_sizes_ok(n, h, w) || maxrad != maxrad) return VV_ERR_BAD_ARG;
  if (n == 0 || h == 0 || w == 0) return VV_OK;
  const bool per_image = !(maxrad > 0.0f);
  if (!flow || !out || (per_image && !work) || ((uintptr_t)flow & 7) || ((uintptr_t)work & 3)) return VV_ERR_BAD_ARG;
  const int hw = h * w;
  const int nblk = (hw + FC_TILE - 1) / FC_TILE, cblk = (hw + VV_WG - 1) / VV_WG;
  if ((int64_t)cblk * n > INT32_MAX) return VV_ERR_UNSUPPORTED;
  if (per_image) {
    for (int i0 = 0; i0 < n; i0 += 65535) {    // gridDim.y
      VV_LAUNCH(flow_rad_kernel, dim3((unsigned)nblk, (unsigned)min(65535, n - i0)), dim3(VV_WG), 0, (hipStream_t)stream,
                reinterpret_cast<const float2*>(flow) + (int64_t)i0 * hw, hw, nblk, static_cast<float*>(work) + (int64_t)i0 * nblk);
      VV_CHECK_LAUNCH();
    }
  }
  VV_LAUNCH(flow_color_kernel, dim3((unsigned)(cblk * n)), dim3(VV_WG), 0, (hipStream_t)stream, reinterpret_cast<const float2*>(flow),
            hw, nblk, cblk, maxrad, static_cast<const float*>(work), out);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_render_overlay(const uint8_t* frames, int32_t c, int32_t bgr, const double* mask, const uint8_t* gt,
                                 const int32_t* rects, const double* scores, const int32_t* frame_off, int32_t n_boxes,
                                 const uint8_t* lut, double lo, double hi, int32_t alpha, int32_t n, int32_t h, int32_t w, uint8_t* out,
                                 vv_stream stream) {
  if (n < 0 || h < 0 || w < 0 || n_boxes < 0 || (int64_t)h * w > INT32_MAX - OV_TILE) return VV_ERR_BAD_ARG;
  if ((c != 1 && c != 3) || alpha < 0 || alpha > 256 || !(hi > lo)) return VV_ERR_BAD_ARG;
  if (n == 0 || h == 0 || w == 0) return VV_OK;
  if (!frames || !mask || !lut || !out || (n_boxes > 0 && (!rects || !scores || !frame_off)) || ((uintptr_t)rects & 15))
    return VV_ERR_BAD_ARG;
  const int tiles = (h * w + OV_TILE - 1) / OV_TILE;
  for (int f0 = 0; f0 < n; f0 += 65535) {      // gridDim.y
    VV_LAUNCH(overlay_kernel, dim3(tiles, min(65535, n - f0)), dim3(VV_WG), 0, (hipStream_t)stream, frames, (int)c, (int)bgr, mask, gt,
              reinterpret_cast<const int4*>(rects), scores, n_boxes > 0 ? frame_off : (const int32_t*)nullptr, lut, lo, hi, (int)alpha,
              f0, (int)h, (int)w, out);
    VV_CHECK_LAUNCH();
  }
  return VV_OK;
}
