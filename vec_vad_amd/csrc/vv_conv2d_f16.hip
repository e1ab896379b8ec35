// FlowNet2 fp16 mode (FlowNet2(fp16=True)): the direct NHWC convolution of vv_conv2d.hip on fp16 activations and fp16 weight
// panels, v_mfma_f32_32x32x16_f16 (v_mfma_f32_16x16x32_f16 for layers of at most 16 output channels), fp32 accumulation.
//
//   conv   : nn.Conv2d(k in {1,3,5,7}, stride in {1,2}, padding=(k-1)//2) [+ LeakyReLU(0.1)]   components/misc.py:8-28,42-44
//   deconv : nn.ConvTranspose2d(k4, s2, p1) [+ LeakyReLU(0.1)] as 4 output-parity phases of 2x2 taps   components/misc.py:31-39
//   row-K  : the few-channel first layers (3-channel 7x7 s2, 6-channel 3x3): K walks the (kx, c) run under one filter row
//
// Semantics are those of the module after .half() (FlowNet2_src/main.py:123-125, "fp16 storage fp32 math"): products of fp16
// operands summed in fp32, the fp32 bias (holding fp16-rounded values) added in fp32, the sum rounded to fp16, LeakyReLU applied to
// the rounded value and rounded again (vv_act_out).  Split-K writes fp32 partials; vv_conv2d_splitk_finish_f16 rounds once.
//
// One workgroup = 8 x TW output pixels (tile space: input pixels for the transposed conv) x 32 / 64 output channels; four waves of
// 2 (TW = 32) or 1 (TW = 16, the H/64 level) 32-pixel M blocks.  The input halo tile [HH][HW][CK + 8] halves goes global ->
// registers -> LDS one K chunk ahead of the MFMAs (the +8 halves shift consecutive pixels by 16 B across the banks); A fragments
// (lane l: pixel l & 31, K 8 (l >> 5) .. +7) are one ds_read_b128, B fragments one 16-byte global load from the packed panel
// [tap][CinP / 8][CoutP][8] halves (lane l: output channel l & 31, K group l >> 5), 512 contiguous bytes per wave and K step.
// Channel strides of the fp16 buffers are multiples of 8 halves (16 B); channels past ceil8(Cin) are never read.
#include "vv_common.h"

namespace {

typedef _Float16 v8hf __attribute__((ext_vector_type(8)));

template <int R, int STRIDE, int DECONV, int NR, int CK, int CP = 0, int N16 = 0, int TW = 32>
__global__ void __launch_bounds__(VV_WG, 2)
conv2d_f16_kernel(const vv_conv2d_params p, const int tilesX, const int tilesY, const int NN, const int total, const int nper) {
  constexpr int TH = 8;
  static_assert(TW == 32 || (TW == 16 && !N16 && !CP), "tile width");
  constexpr int HH = DECONV ? TH + 2 : (TH - 1) * STRIDE + R;
  constexpr int HW = DECONV ? TW + 2 : (TW - 1) * STRIDE + R;
  constexpr int SP = DECONV ? 1 : STRIDE;
  constexpr int S = CP ? CP : CK + 8;                  // halves per staged pixel
  constexpr int NG = (CP ? CP : CK) / 8;               // 16-byte groups per staged pixel
  constexpr int NTAP = DECONV ? 4 : (CP ? R : R * R);
  constexpr int MR = TW / 16, TN = NR * 32;
  constexpr int KST = N16 ? 32 : 16;                   // K per MFMA
  constexpr int KG = CK / KST;
  constexpr int NSL = HH * HW * NG;
  constexpr int NIT = (NSL + VV_WG - 1) / VV_WG;
  constexpr int EXTRA = CP ? 8 : 0;                    // row-K: the K padding of the tile's last pixel reads past the tile
  static_assert(!CP || (!DECONV && CP == 8 && CK % 16 == 0 && CK >= R * CP && CK < R * CP + 16), "row-K geometry");
  static_assert(CK % KST == 0 && (!N16 || NR == 1), "K chunk / 16-wide N");
  __shared__ __attribute__((aligned(16))) vv_h lds[HH * HW * S + EXTRA];
  if constexpr (EXTRA != 0) {
    if (threadIdx.x < EXTRA) lds[HH * HW * S + threadIdx.x] = (vv_h)0.f;
  }
  int w = vv_xcd_remap(blockIdx.x, nper);
  if (w >= total) return;
  const int KS = p.pad0 > 1 ? p.pad0 : 1;
  const int ks = w % KS; w /= KS;
  const int tx = w % tilesX; w /= tilesX;
  const int ty = w % tilesY; w /= tilesY;
  const int nn = w % NN; w /= NN;
  constexpr int NPH = DECONV ? 4 : 1;
  const int ph = w % NPH;
  const int img = w / NPH;
  const int py = ph >> 1, px = ph & 1;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const int q16 = lane >> 4, l15 = lane & 15;
  const int H = p.H, W = p.W;
  const int ty0 = ty * TH, tx0 = tx * TW;
  constexpr int pad = (R - 1) / 2;
  const int oy0 = DECONV ? ty0 - 1 : ty0 * STRIDE - pad;
  const int ox0 = DECONV ? tx0 - 1 : tx0 * STRIDE - pad;

  const vv_h* __restrict__ src = reinterpret_cast<const vv_h*>(p.src.ptr);
  const int cs = p.src.cstride, scoff = p.src.coff;
  const int C8 = (p.Cin + 7) & ~7;                     // channels read per pixel (pad channels up to ceil8 are finite; their panel rows are 0)
  const int CoutP = p.CoutP, KQ = p.CinP >> 3;
  const int co0 = nn * TN;
  const vv_h* __restrict__ wg = reinterpret_cast<const vv_h*>(p.w);

  // tap t: halo-tile offset (halves) of its input pixel and its panel tap index
  int aoff[NTAP], wtap[NTAP];
#pragma unroll
  for (int t = 0; t < NTAP; ++t) {
    if constexpr (DECONV) {
      // oy = 2*iy - 1 + ky: even rows use ky=1 (iy=r) and ky=3 (iy=r-1); odd rows ky=2 (iy=r) and ky=0 (iy=r+1)
      const int ty_ = t >> 1, tx_ = t & 1;
      const int dy = py ? (ty_ ? 1 : 0) : (ty_ ? -1 : 0), ky = py ? (ty_ ? 0 : 2) : (ty_ ? 3 : 1);
      const int dx = px ? (tx_ ? 1 : 0) : (tx_ ? -1 : 0), kx = px ? (tx_ ? 0 : 2) : (tx_ ? 3 : 1);
      aoff[t] = ((1 + dy) * HW + (1 + dx)) * S;
      wtap[t] = ky * 4 + kx;
    } else if constexpr (CP != 0) {
      aoff[t] = t * HW * S;
      wtap[t] = t;
    } else {
      aoff[t] = ((t / R) * HW + (t % R)) * S;
      wtap[t] = t;
    }
  }
  int abase[N16 ? 4 : MR];
  if constexpr (N16 != 0) {
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
      const int pp = wave * 64 + mb * 16 + l15;
      abase[mb] = (((pp / TW) * SP) * HW + (pp % TW) * SP) * S + 8 * q16;
    }
  } else {
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const int pp = wave * (32 * MR) + m * 32 + l31;
      abase[m] = (((pp / TW) * SP) * HW + (pp % TW) * SP) * S + 8 * half;
    }
  }
  v16f acc[MR][NR];
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int n = 0; n < NR; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.f;
  v4f acc16[4];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) acc16[mb] = v4f{0.f, 0.f, 0.f, 0.f};

  uint4 stg[NIT];
  auto issue = [&](const int c0) {
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int it = tid + k * VV_WG;
      const int g = it % NG, hp = it / NG;
      const int y = oy0 + hp / HW, x = ox0 + hp % HW;
      const int ch = CP ? 8 * g : c0 + 8 * g;
      const bool ok = (NSL % VV_WG == 0 || it < NSL) && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W && (CP || ch < C8);
      stg[k] = ok ? *reinterpret_cast<const uint4*>(src + ((int64_t)(img * H + y) * W + x) * cs + scoff + ch) : make_uint4(0, 0, 0, 0);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
      const int it = tid + k * VV_WG;
      if (NSL % VV_WG == 0 || it < NSL) *reinterpret_cast<uint4*>(lds + (it / NG) * S + 8 * (it % NG)) = stg[k];
    }
  };

  const int nchunk = p.CinP / CK;
  const int cbeg = (nchunk * ks / KS) * CK, cend = (nchunk * (ks + 1) / KS) * CK;
  if (cbeg < cend) issue(cbeg);
  for (int c0 = cbeg; c0 < cend; c0 += CK) {
    if (c0 != cbeg) __syncthreads();                  // every wave finished reading the previous chunk
    commit();
    __syncthreads();
    if (c0 + CK < cend) issue(c0 + CK);
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
#pragma unroll
      for (int kg = 0; kg < KG; ++kg) {
        if constexpr (N16 != 0) {
          const v8hf b = *reinterpret_cast<const v8hf*>(
              wg + ((int64_t)(wtap[t] * KQ + (c0 >> 3) + kg * 4 + q16) * CoutP + co0 + l15) * 8);
#pragma unroll
          for (int mb = 0; mb < 4; ++mb) {
            const v8hf a = *reinterpret_cast<const v8hf*>(lds + abase[mb] + aoff[t] + kg * 32);
            acc16[mb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc16[mb], 0, 0, 0);
          }
        } else {
          v8hf a[MR], b[NR];
#pragma unroll
          for (int n = 0; n < NR; ++n)
            b[n] = *reinterpret_cast<const v8hf*>(
                wg + ((int64_t)(wtap[t] * KQ + (c0 >> 3) + kg * 2 + half) * CoutP + co0 + n * 32 + l31) * 8);
#pragma unroll
          for (int m = 0; m < MR; ++m) a[m] = *reinterpret_cast<const v8hf*>(lds + abase[m] + aoff[t] + kg * 16);
#pragma unroll
          for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int n = 0; n < NR; ++n) acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[m], b[n], acc[m][n], 0, 0, 0);
        }
      }
    }
  }

  // ---- epilogue: fp32 partials (split-K) or bias + round + LeakyReLU + round into the (possibly shared concat) fp16 buffer
  const int OH = DECONV ? 2 * H : (H + 2 * pad - R) / STRIDE + 1;
  const int OW = DECONV ? 2 * W : (W + 2 * pad - R) / STRIDE + 1;
  const int LH = DECONV ? H : OH, LW = DECONV ? W : OW;
  const bool split = KS > 1;
  float* __restrict__ wsp = reinterpret_cast<float*>(p.out.ptr) + (int64_t)ks * p.B * OH * OW * CoutP;
  vv_h* __restrict__ outg = reinterpret_cast<vv_h*>(p.out.ptr) + p.out.coff;
  const int ocs = p.out.cstride;
  const float slope = p.slope;
  if constexpr (N16 != 0) {
    // D of the 16x16 tile: lane (channel l15, row quarter q) holds pixels mb*16 + 4q + i
    const int co = co0 + l15;
    const bool cok = split || co < p.Cout;
    const float b = (!split && p.bias && cok) ? p.bias[co] : 0.f;
#pragma unroll
    for (int mb = 0; mb < 4; ++mb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int pp = wave * 64 + mb * 16 + q16 * 4 + i;
        const int r = ty0 + pp / TW, c = tx0 + pp % TW;
        if (r < LH && c < LW && cok) {
          const int oy = DECONV ? 2 * r + py : r, ox = DECONV ? 2 * c + px : c;
          const int64_t pix = (int64_t)(img * OH + oy) * OW + ox;
          if (split) wsp[pix * CoutP + co] = acc16[mb][i];
          else outg[pix * ocs + co] = vv_act_out<vv_h>(acc16[mb][i] + b, slope);
        }
      }
    return;
  }
  float bias[NR];
  bool cok[NR];
#pragma unroll
  for (int n = 0; n < NR; ++n) {
    const int co = co0 + n * 32 + l31;
    cok[n] = split || co < p.Cout;
    bias[n] = (!split && p.bias && cok[n]) ? p.bias[co] : 0.f;
  }
#pragma unroll
  for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = (i & 3) + 8 * (i >> 2) + 4 * half;
      const int pp = wave * (32 * MR) + m * 32 + row;
      const int r = ty0 + pp / TW, c = tx0 + pp % TW;
      if (r < LH && c < LW) {
        const int oy = DECONV ? 2 * r + py : r, ox = DECONV ? 2 * c + px : c;
        const int64_t pix = (int64_t)(img * OH + oy) * OW + ox;
#pragma unroll
        for (int n = 0; n < NR; ++n) {
          const int co = co0 + n * 32 + l31;
          if (split) wsp[pix * CoutP + co] = acc[m][n][i];
          else if (cok[n]) outg[pix * ocs + co] = vv_act_out<vv_h>(acc[m][n][i] + bias[n], slope);
        }
      }
    }
}

// fp32 nn.Conv2d / nn.ConvTranspose2d weight -> fp16 panel [tap][KP/8][NP][8] (zero K / N padding); the one rounding of .half()
__global__ void __launch_bounds__(VV_WG)
pack_conv2d_f16_kernel(const float* __restrict__ w, vv_h* __restrict__ packed, const int taps, const int K, const int KP,
                       const int N, const int NP, const int transposed) {
  const int64_t total = (int64_t)taps * KP * NP;
  const int KQ = KP >> 3;
  for (int64_t d = (int64_t)blockIdx.x * VV_WG + threadIdx.x; d < total; d += (int64_t)gridDim.x * VV_WG) {
    const int j = (int)(d & 7);
    int64_t t = d >> 3;
    const int n = (int)(t % NP); t /= NP;
    const int kq = (int)(t % KQ);
    const int tap = (int)(t / KQ);
    const int k = kq * 8 + j;
    float v = 0.f;
    if (k < K && n < N)
      v = transposed ? w[((int64_t)k * N + n) * taps + tap]       // ConvTranspose2d weight [Cin=k][Cout=n][ky][kx]
                     : w[((int64_t)n * K + k) * taps + tap];      // Conv2d weight [Cout=n][Cin=k][ky][kx]
    packed[d] = (vv_h)v;
  }
}

template <int R, int STRIDE, int DECONV, int CK, int CP = 0>
int launch_f16(const vv_conv2d_params* p, hipStream_t st) {
  constexpr int pad = (R - 1) / 2;
  const int LH = DECONV ? p->H : (p->H + 2 * pad - R) / STRIDE + 1;
  const int LW = DECONV ? p->W : (p->W + 2 * pad - R) / STRIDE + 1;
  const bool narrow = LW <= 16 && !CP;          // the H/64 level: 8 x 16 tiles
  const int tilesY = (LH + 7) / 8, tilesX = narrow ? 1 : (LW + 31) / 32;
  const bool wide = p->CoutP % 64 == 0 && p->Cout > 32;
  const int NN = p->CoutP / (wide ? 64 : 32);
  constexpr bool CAN16 = !CP && CK % 32 == 0;
  const int total = p->B * (DECONV ? 4 : 1) * NN * tilesY * tilesX * (p->pad0 > 1 ? p->pad0 : 1);
  const int nper = (total + 7) / 8;
  const dim3 grid(nper * 8), blk(VV_WG);
  if (narrow) {
    if constexpr (CP == 0) {
      if (wide) VV_LAUNCH((conv2d_f16_kernel<R, STRIDE, DECONV, 2, CK, 0, 0, 16>), grid, blk, 0, st, *p, tilesX, tilesY, NN, total, nper);
      else VV_LAUNCH((conv2d_f16_kernel<R, STRIDE, DECONV, 1, CK, 0, 0, 16>), grid, blk, 0, st, *p, tilesX, tilesY, NN, total, nper);
    }
  } else if (wide) {
    VV_LAUNCH((conv2d_f16_kernel<R, STRIDE, DECONV, 2, CK, CP>), grid, blk, 0, st, *p, tilesX, tilesY, NN, total, nper);
  } else if (CAN16 && p->Cout <= 16) {
    if constexpr (CAN16)
      VV_LAUNCH((conv2d_f16_kernel<R, STRIDE, DECONV, 1, CK, 0, 1>), grid, blk, 0, st, *p, tilesX, tilesY, NN, total, nper);
  } else {
    VV_LAUNCH((conv2d_f16_kernel<R, STRIDE, DECONV, 1, CK, CP>), grid, blk, 0, st, *p, tilesX, tilesY, NN, total, nper);
  }
  VV_CHECK_LAUNCH();
  return VV_OK;
}

}  // namespace

extern "C" int vv_conv2d_f16(const vv_conv2d_params* p, vv_stream stream) {
  if (!p || !p->src.ptr || !p->w || !p->out.ptr) return VV_ERR_BAD_ARG;
  if (p->CoutP % 32 || p->src.cstride % 8 || p->src.coff % 8 || p->Cin > p->CinP) return VV_ERR_BAD_ARG;
  // the loader (issue) addresses src + (int64_t)pixel * cstride with 64-bit pointers, so no byte limit applies here; the limit on
  // elements (2^32 bytes of halves) is kept
  if ((int64_t)p->B * p->H * p->W * p->src.cstride >= (1ll << 31)) return VV_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (p->kind == 2) {
    // row-K: pixels exactly 8 halves apart, Cin = CinP = the flattened (kx, c) run padded to 16; no split-K
    if (p->src.coff != 0 || p->pad0 > 1 || p->Cin != p->CinP || p->src.cstride != 8) return VV_ERR_BAD_ARG;
    if (p->R == 7 && p->stride == 2 && p->CinP == 64) return launch_f16<7, 2, 0, 64, 8>(p, st);
    if (p->R == 3 && p->stride == 1 && p->CinP == 32) return launch_f16<3, 1, 0, 32, 8>(p, st);
    return VV_ERR_UNSUPPORTED;
  }
  if (p->CinP % 32 || (p->src.coff + ((p->Cin + 7) & ~7)) > p->src.cstride) return VV_ERR_BAD_ARG;
  if (p->kind == 1) {
    if (p->R != 4 || p->stride != 2) return VV_ERR_BAD_ARG;
    return launch_f16<4, 2, 1, 32>(p, st);
  }
  if (p->kind != 0) return VV_ERR_BAD_ARG;
  switch (p->R * 10 + p->stride) {
    case 11: return launch_f16<1, 1, 0, 32>(p, st);
    case 31: return launch_f16<3, 1, 0, 32>(p, st);
    case 32: return launch_f16<3, 2, 0, 16>(p, st);
    case 52: return launch_f16<5, 2, 0, 16>(p, st);
    case 72: return launch_f16<7, 2, 0, 16>(p, st);
  }
  return VV_ERR_UNSUPPORTED;
}

extern "C" int vv_pack_conv2d_f16(const float* w, uint16_t* packed, int32_t taps, int32_t K, int32_t KP, int32_t N, int32_t NP,
                                  int32_t transposed, vv_stream stream) {
  if (!w || !packed || KP % 16 || NP % 32) return VV_ERR_BAD_ARG;
  const int64_t total = (int64_t)taps * KP * NP;
  int64_t nb = (total + VV_WG - 1) / VV_WG;
  if (nb > 16384) nb = 16384;
  VV_LAUNCH(pack_conv2d_f16_kernel, dim3((unsigned)nb), dim3(VV_WG), 0, (hipStream_t)stream, w, reinterpret_cast<vv_h*>(packed),
            taps, K, KP, N, NP, transposed);
  VV_CHECK_LAUNCH();
  return VV_OK;
}
