// Per-pixel reconstruction error of the UNet bank: what vv_outconv_fwd sums into one float per cube, kept per pixel.
//   e_raw[b][p] = sum over the raw UNets g (tgt_src[g] == 0), sum over c < oc[g] of (out4[g][b*HW+p][c] - tgt0[b*HW+p][tgt_coff[g]+c])^2
//   e_of        = the same over the flow UNets (tgt_src[g] == 1) and tgt1
// from the stored reconstruction out4 [G][B*HW][4] of the eval-mode forward (vv_outconv_params.out4 != NULL) and its two targets.
// One streaming pass: a thread owns one pixel, reads the G 16-byte out4 rows of that pixel (coalesced: consecutive lanes, consecutive
// rows) and the 3 / 2 target floats of every UNet, writes two floats.  G*B*HW*16 bytes of out4 + the targets in, 8*B*HW bytes out;
// no LDS, no atomics, nothing for the matrix cores.  Groups in ascending g, channels in ascending c, fp32 like the score itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vecvad_hip.h"
#include "vv_common.h"

namespace {

__global__ void __launch_bounds__(VV_WG)
error_maps_kernel(const int G, const int64_t MB, const float* __restrict__ out4, const int32_t* __restrict__ oc,
                  const int32_t* __restrict__ tgt_src, const int32_t* __restrict__ tgt_coff, const float* __restrict__ tgt0,
                  const int tcs0, const float* __restrict__ tgt1, const int tcs1, float* __restrict__ e_raw,
                  float* __restrict__ e_of) {
  const int64_t pix = (int64_t)blockIdx.x * VV_WG + threadIdx.x;
  if (pix >= MB) return;
  float er = 0.f, eo = 0.f;
  for (int g = 0; g < G; ++g) {                // g, oc, tgt_src, tgt_coff are wave-uniform: scalar loads, no divergence
    const int src = tgt_src[g];
    if (src != 0 && !e_of) continue;           // flow UNets of a caller that keeps no flow map
    const int n = oc[g];
    const float4 o = *reinterpret_cast<const float4*>(out4 + ((int64_t)g * MB + pix) * 4);
    const float* q = (src == 0 ? tgt0 + pix * tcs0 : tgt1 + pix * tcs1) + tgt_coff[g];
    const float ov[4] = {o.x, o.y, o.z, o.w};
    float acc = src == 0 ? er : eo;
    for (int c = 0; c < 4; ++c)
      if (c < n) {
        const float d = ov[c] - q[c];
        acc = fmaf(d, d, acc);
      }
    if (src == 0) er = acc; else eo = acc;
  }
  e_raw[pix] = er;
  if (e_of) e_of[pix] = eo;
}

}  // namespace

extern "C" int vv_error_maps(int32_t G, int32_t B, int32_t HW, const float* out4, const int32_t* oc, const int32_t* tgt_src,
                             const int32_t* tgt_coff, const float* tgt0, int32_t tgt0_cstride, const float* tgt1,
                             int32_t tgt1_cstride, float* e_raw, float* e_of, vv_stream stream) {
  if (G < 0 || B < 0 || HW < 0 || tgt0_cstride < 0 || tgt1_cstride < 0) return VV_ERR_BAD_ARG;
  const int64_t MB = (int64_t)B * HW;
  if (MB == 0) return VV_OK;
  if (!e_raw || (G > 0 && (!out4 || !oc || !tgt_src || !tgt_coff || !tgt0)) || (e_of && G > 0 && !tgt1)) return VV_ERR_BAD_ARG;
  const int64_t blocks = (MB + VV_WG - 1) / VV_WG;
  if (blocks > INT32_MAX) return VV_ERR_BAD_ARG;
  VV_LAUNCH(error_maps_kernel, dim3((unsigned)blocks), dim3(VV_WG), 0, (hipStream_t)stream, (int)G, MB, out4, oc, tgt_src, tgt_coff,
            tgt0, (int)tgt0_cstride, tgt1, (int)tgt1_cstride, e_raw, e_of);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
