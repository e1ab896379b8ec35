// cv2.resize (INTER_LINEAR) of a crop, one output pixel at a time, and the motion energy of a box built on it: THE one place this
// arithmetic lives.  vv_extract.hip (vv_crop_resize, vv_cube_cut, vv_cube_energy, the two flow resizes) and vv_stream.hip (vv_stream_cut)
// include it, so a cube cut per frame on the stream and a cube cut per chunk on the batch route agree to the bit.
// The uint8 path is bit-exact fixed point; the float path rounds every product and sum to fp32 like the C++ it replaces.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Every product and sum below must be rounded separately, like the host arithmetic it replaces: forbid FMA contraction from here to
// the end of the translation unit.  (ROCm's __fmul_rn/__fadd_rn are plain operators defined in a header, i.e. BEFORE this pragma, and
// do get fused after inlining -- hence ordinary operators here.)
#pragma clang fp contract(off)

namespace vv_resize {

struct Tap {
  int s0, s1;
  float w0, w1;
};

// one axis of cv::resize's linear table: d -> (s0, s1, 1-f, f)
__device__ inline Tap axis_tap(int d, int dst, int src, bool horizontal) {
  double scale = 1.0 / ((double)dst / (double)src);
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f = f - (float)s;
  Tap t;
  if (horizontal) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= src - 1) { f = 0.f; s = src - 1; }
    t.s0 = s;
    t.s1 = min(s + 1, src - 1);
  } else {
    t.s0 = min(max(s, 0), src - 1);
    t.s1 = min(max(s + 1, 0), src - 1);
  }
  t.w0 = 1.f - f;
  t.w1 = f;
  return t;
}

__device__ inline int fixed11(float w) {
  int v = __float2int_rn(w * 2048.f);
  return min(max(v, -32768), 32767);
}

// One output pixel (all C channels) of cv::resize(crop, (ow, oh)): src = the crop's top-left element inside its frame, rs = the
// frame's row stride in elements.  emit(c, v) receives each channel value -- a store (vv_crop_resize, vv_cube_cut) or a sum
// (vv_cube_energy) -- so every caller shares one arithmetic.
template <typename T, typename Emit>
__device__ inline void resize_pixel(const T* __restrict__ src, int64_t rs, int C, int cw, int ch, int oh, int ow, int dy, int dx,
                                    Emit emit) {
  if (cw == ow && ch == oh) {                       // same size: plain copy
    for (int c = 0; c < C; ++c) emit(c, src[dy * rs + (int64_t)dx * C + c]);
    return;
  }
  if (cw == 2 * ow && ch == 2 * oh) {               // exact 2x decimation -> INTER_AREA
    const T* p = src + (2 * dy) * rs + (int64_t)(2 * dx) * C;
    for (int c = 0; c < C; ++c) {
      if constexpr (sizeof(T) == 1) {
        emit(c, (T)(((int)p[c] + (int)p[C + c] + (int)p[rs + c] + (int)p[rs + C + c] + 2) >> 2));
      } else {
        emit(c, (((p[c] + p[C + c]) + p[rs + c]) + p[rs + C + c]) * 0.25f);
      }
    }
    return;
  }
  Tap tx = axis_tap(dx, ow, cw, true), ty = axis_tap(dy, oh, ch, false);
  const T* r0 = src + ty.s0 * rs;
  const T* r1 = src + ty.s1 * rs;
  int64_t o0 = (int64_t)tx.s0 * C, o1 = (int64_t)tx.s1 * C;
  if constexpr (sizeof(T) == 1) {
    int a0 = fixed11(tx.w0), a1 = fixed11(tx.w1), b0 = fixed11(ty.w0), b1 = fixed11(ty.w1);
    for (int c = 0; c < C; ++c) {
      int h0 = (int)r0[o0 + c] * a0 + (int)r0[o1 + c] * a1;
      int h1 = (int)r1[o0 + c] * a0 + (int)r1[o1 + c] * a1;
      int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
      emit(c, (T)min(max(v, 0), 255));
    }
  } else {
    for (int c = 0; c < C; ++c) {
      float h0 = r0[o0 + c] * tx.w0 + r0[o1 + c] * tx.w1;
      float h1 = r1[o0 + c] * tx.w0 + r1[o1 + c] * tx.w1;
      emit(c, h0 * ty.w0 + h1 * ty.w1);
    }
  }
}

// a crop that does not lie inside the frame reads nothing.  The Python wrappers refuse such a table before they launch
// (extract.check_tables); this guard, the slot guards and the window clamps of the kernels only keep a caller of the bare C ABI with a
// wrong table from touching memory outside its buffers.
__device__ inline bool crop_ok(int x0, int y0, int x1, int y1, int H, int W) {
  return 0 <= x0 && x0 < x1 && x1 <= W && 0 <= y0 && y0 < y1 && y1 <= H;
}

// The motion energy of one box, formed by a workgroup of 256 threads: thread j sums the squares of pixels j, j + 256, ... of the
// [nT][P][P] patch in that order (channels in order inside a pixel), each value widened to float64 before it is squared, the 256
// partial sums meet in a fixed LDS tree (part: 256 doubles) and the total is divided by nT: the same bits on every run, and the same
// bits in every kernel that calls this.  win: the nT frames of the box's window as indices into frames [F][H][W][C] (clamped).  cube
// (or null): the resized patch is also stored there as [nT][P][P][C], the values the sum was formed from.  Every thread of the
// workgroup must call it with the same arguments and gets the result; a crop that fails crop_ok reads nothing and gives 0.
__device__ inline double box_energy(const float* __restrict__ frames, int F, int H, int W, int C, int x_min, int y_min, int x_max,
                                    int y_max, const int32_t* __restrict__ win, int nT, int P, double* part, float* __restrict__ cube) {
  double acc = 0.0;
  if (crop_ok(x_min, y_min, x_max, y_max, H, W)) {       // the same for every thread of the workgroup
    int per = nT * P * P;                                // fits: the entry points refuse T * P * P > INT32_MAX
    for (int j = threadIdx.x; j < per; j += 256) {
      int dx = j % P, dy = (j / P) % P, t = j / (P * P);
      int f = min(max(win[t], 0), F - 1);
      const float* src = frames + (((int64_t)f * H + y_min) * W + x_min) * C;
      float* dst = cube ? cube + (int64_t)j * C : nullptr;
      resize_pixel(src, (int64_t)W * C, C, x_max - x_min, y_max - y_min, P, P, dy, dx, [&acc, dst](int c, float v) {
        if (dst) dst[c] = v;
        double d = (double)v;
        acc = acc + d * d;
      });
    }
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + s];
    __syncthreads();
  }
  return part[0] / (double)nT;
}

}  // namespace vv_resize
