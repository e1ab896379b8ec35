// Cube extraction: crop + cv2.resize(INTER_LINEAR) of n boxes out of T decoded frames in one launch
// (reference vad_datasets.py:70-93 get_foreground; calc_optical_flow.py:46-59,82 whole-frame resizes); vv_cube_cut / vv_cube_energy
// do the same for the boxes of many consecutive frames at once, every box with its own frame window (test.py's direct path).
// HBM-bound gather: every output element reads <= 4 source elements that neighbouring lanes share through L2/TCP.
// The uint8 path is bit-exact fixed point; the float path rounds every product and sum to fp32 (no FMA contraction: the pragma
// of vv_resize.h, where the arithmetic lives) like the C++ it replaces.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

#include "vv_resize.h"      // Tap / resize_pixel / crop_ok / box_energy, shared with vv_stream.hip; switches FMA contraction off

namespace {

using namespace vv_resize;

template <typename T>
__global__ void __launch_bounds__(256) crop_resize_kernel(const T* __restrict__ frames, int nT, int H, int W, int C,
                                                          const int32_t* __restrict__ crops, int n, int oh, int ow,
                                                          T* __restrict__ out) {
  int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)n * nT * oh * ow;
  if (gid >= total) return;
  int dx = (int)(gid % ow);
  int dy = (int)((gid / ow) % oh);
  int t = (int)((gid / ((int64_t)ow * oh)) % nT);
  int i = (int)(gid / ((int64_t)ow * oh * nT));
  int x_min = crops[4 * i + 0], y_min = crops[4 * i + 1];
  int cw = crops[4 * i + 2] - x_min, ch = crops[4 * i + 3] - y_min;
  const T* src = frames + (((int64_t)t * H + y_min) * W + x_min) * C;
  T* dst = out + gid * C;
  resize_pixel(src, (int64_t)W * C, C, cw, ch, oh, ow, dy, dx, [dst](int c, T v) { dst[c] = v; });
}

// vv_cube_cut: one thread per output pixel of (box i, context frame t); every box brings its own frame window and store slot.
template <typename T>
__global__ void __launch_bounds__(256) cube_cut_kernel(const T* __restrict__ frames, int F, int H, int W, int C,
                                                       const int32_t* __restrict__ crops, const int32_t* __restrict__ win,
                                                       const int32_t* __restrict__ slot, int n, int nT, int P, int64_t slots,
                                                       T* __restrict__ out) {
  int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t total = (int64_t)n * nT * P * P;
  if (gid >= total) return;
  int dx = (int)(gid % P);
  int dy = (int)((gid / P) % P);
  int t = (int)((gid / ((int64_t)P * P)) % nT);
  int i = (int)(gid / ((int64_t)P * P * nT));
  int64_t s = slot[i];
  if (s < 0 || s >= slots) return;
  int x_min = crops[4 * i + 0], y_min = crops[4 * i + 1], x_max = crops[4 * i + 2], y_max = crops[4 * i + 3];
  if (!crop_ok(x_min, y_min, x_max, y_max, H, W)) return;
  int f = min(max(win[(int64_t)i * nT + t], 0), F - 1);
  const T* src = frames + (((int64_t)f * H + y_min) * W + x_min) * C;
  T* dst = out + (((s * nT + t) * P + dy) * P + dx) * C;
  resize_pixel(src, (int64_t)W * C, C, x_max - x_min, y_max - y_min, P, P, dy, dx, [dst](int c, T v) { dst[c] = v; });
}

// vv_cube_energy: one workgroup per box.  Thread j sums the squares of pixels j, j + 256, ... of the [Tf][P][P] patch in that order
// (channels in order inside a pixel), the 256 partial sums meet in a fixed LDS tree: the same bits on every run.
__global__ void __launch_bounds__(256) cube_energy_kernel(const float* __restrict__ frames, int F, int H, int W, int C,
                                                          const int32_t* __restrict__ crops, const int32_t* __restrict__ win,
                                                          int n, int nT, int P, double thr, double* __restrict__ energy,
                                                          uint8_t* __restrict__ keep) {
  __shared__ double part[256];
  int i = blockIdx.x;
  double e = box_energy(frames, F, H, W, C, crops[4 * i + 0], crops[4 * i + 1], crops[4 * i + 2], crops[4 * i + 3],
                        win + (int64_t)i * nT, nT, P, part, nullptr);
  if (threadIdx.x == 0) {
    energy[i] = e;
    keep[i] = e > thr ? 1 : 0;
  }
}

// vv_flow_pairs_prep: one thread per output pixel (x fastest) of frame k of pair n; the C = 1 | 3 channel values of that pixel, the
// uint8 arithmetic of vv_crop_resize on the whole frame, go as floats into the 3 planes of FlowNet2's [N][3][2][oh][ow] input (a
// grey frame's one plane three times).  Writes are coalesced along x inside a plane.
__global__ void __launch_bounds__(256) flow_pairs_prep_kernel(const uint8_t* __restrict__ frames, int F, int H, int W, int C,
                                                              const int32_t* __restrict__ pairs, int N, int oh, int ow,
                                                              float* __restrict__ out) {
  int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t plane = (int64_t)oh * ow;
  if (gid >= (int64_t)N * 2 * plane) return;
  int dx = (int)(gid % ow);
  int dy = (int)((gid / ow) % oh);
  int k = (int)((gid / plane) % 2);
  int n = (int)(gid / (2 * plane));
  int f = min(max(pairs[2 * n + k], 0), F - 1);
  const uint8_t* src = frames + (int64_t)f * H * W * C;
  float* dst = out + ((int64_t)n * 6 + k) * plane + (int64_t)dy * ow + dx;        // plane (n, c, k) = (n * 3 + c) * 2 + k
  int64_t cstep = 2 * plane;
  if (C == 1) {
    resize_pixel(src, (int64_t)W, 1, W, H, oh, ow, dy, dx, [dst, cstep](int, uint8_t v) {
      float x = (float)v;
      dst[0] = x;
      dst[cstep] = x;
      dst[2 * cstep] = x;
    });
  } else {
    resize_pixel(src, (int64_t)W * 3, 3, W, H, oh, ow, dy, dx, [dst, cstep](int c, uint8_t v) { dst[c * cstep] = (float)v; });
  }
}

// vv_flow_resize_back: one thread per output pixel (x fastest) of pair n; each of the two planes of FlowNet2's planar [N][2][fh][fw]
// output goes through the float path with C = 1 (the per-channel arithmetic of vv_crop_resize on the interleaved field), and the
// two values leave as one 8-byte store into the [H][W][2] field of row rows[n].
__global__ void __launch_bounds__(256) flow_resize_back_kernel(const float* __restrict__ flow, int N, int fh, int fw,
                                                               const int32_t* __restrict__ rows, int H, int W,
                                                               float* __restrict__ out, int64_t out_rows) {
  int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t field = (int64_t)H * W;
  if (gid >= (int64_t)N * field) return;
  int dx = (int)(gid % W);
  int dy = (int)((gid / W) % H);
  int n = (int)(gid / field);
  int64_t r = rows[n];
  if (r < 0 || r >= out_rows) return;
  int64_t plane = (int64_t)fh * fw;
  const float* src = flow + (int64_t)n * 2 * plane;
  float2 v;
  resize_pixel(src, (int64_t)fw, 1, fw, fh, H, W, dy, dx, [&v](int, float x) { v.x = x; });
  resize_pixel(src + plane, (int64_t)fw, 1, fw, fh, H, W, dy, dx, [&v](int, float x) { v.y = x; });
  *reinterpret_cast<float2*>(out + ((r * H + dy) * W + dx) * 2) = v;
}

}  // namespace

extern "C" int vv_crop_resize(const void* frames, int32_t is_f32, int32_t T, int32_t H, int32_t W, int32_t C,
                              const int32_t* crops, int32_t n, int32_t oh, int32_t ow, void* out, vv_stream stream) {
  if (!frames || !crops || !out || T <= 0 || H <= 0 || W <= 0 || C <= 0 || n < 0 || oh <= 0 || ow <= 0)
    return VV_ERR_BAD_ARG;
  if (n == 0) return VV_OK;
  int64_t total = (int64_t)n * T * oh * ow;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return VV_ERR_BAD_ARG;
  if (is_f32) {
    VV_LAUNCH(crop_resize_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
              (const float*)frames, T, H, W, C, crops, n, oh, ow, (float*)out);
  } else {
    VV_LAUNCH(crop_resize_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
              (const uint8_t*)frames, T, H, W, C, crops, n, oh, ow, (uint8_t*)out);
  }
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_cube_cut(const void* frames, int32_t is_f32, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* crops,
                           const int32_t* win, const int32_t* slot, int32_t n, int32_t T, int32_t P, void* out, int64_t out_slots,
                           vv_stream stream) {
  if (F <= 0 || H <= 0 || W <= 0 || C <= 0 || n < 0 || T <= 0 || P <= 0 || out_slots < 0) return VV_ERR_BAD_ARG;
  if (n == 0) return VV_OK;
  if (!frames || !crops || !win || !slot || !out) return VV_ERR_BAD_ARG;
  int64_t total = (int64_t)n * T * P * P;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return VV_ERR_BAD_ARG;
  if (is_f32) {
    VV_LAUNCH(cube_cut_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)frames, F, H, W, C,
              crops, win, slot, n, T, P, out_slots, (float*)out);
  } else {
    VV_LAUNCH(cube_cut_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)frames, F, H, W,
              C, crops, win, slot, n, T, P, out_slots, (uint8_t*)out);
  }
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_cube_energy(const float* frames, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* crops,
                              const int32_t* win, int32_t n, int32_t T, int32_t P, double thr, double* energy, uint8_t* keep,
                              vv_stream stream) {
  if (F <= 0 || H <= 0 || W <= 0 || C <= 0 || n < 0 || T <= 0 || P <= 0 || P > 1024) return VV_ERR_BAD_ARG;
  if ((int64_t)T * P * P > 0x7fffffff) return VV_ERR_BAD_ARG;      // the kernel indexes a box's patch with an int
  if (n == 0) return VV_OK;
  if (!frames || !crops || !win || !energy || !keep) return VV_ERR_BAD_ARG;
  VV_LAUNCH(cube_energy_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, frames, F, H, W, C, crops, win, n, T, P, thr,
            energy, keep);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_flow_pairs_prep(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* pairs, int32_t N,
                                  int32_t oh, int32_t ow, float* out, vv_stream stream) {
  if (F <= 0 || H <= 0 || W <= 0 || (C != 1 && C != 3) || N < 0 || oh <= 0 || ow <= 0) return VV_ERR_BAD_ARG;
  if (N == 0) return VV_OK;
  if (!frames || !pairs || !out) return VV_ERR_BAD_ARG;
  int64_t total = (int64_t)N * 2 * oh * ow;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return VV_ERR_BAD_ARG;
  VV_LAUNCH(flow_pairs_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames, F, H, W, C, pairs, N, oh, ow,
            out);
  VV_CHECK_LAUNCH();
  return VV_OK;
}

extern "C" int vv_flow_resize_back(const float* flow, int32_t N, int32_t fh, int32_t fw, const int32_t* rows, int32_t H, int32_t W,
                                   float* out, int64_t out_rows, vv_stream stream) {
  if (N < 0 || fh <= 0 || fw <= 0 || H <= 0 || W <= 0 || out_rows < 0) return VV_ERR_BAD_ARG;
  if (N == 0) return VV_OK;
  if (!flow || !rows || !out || ((uintptr_t)out & 7)) return VV_ERR_BAD_ARG;          // the kernel stores float2
  int64_t total = (int64_t)N * H * W;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return VV_ERR_BAD_ARG;
  VV_LAUNCH(flow_resize_back_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, flow, N, fh, fw, rows, H, W, out,
            out_rows);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
