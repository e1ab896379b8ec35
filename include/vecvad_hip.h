/* vecvad_hip.h -- C ABI of libvecvad_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the VEC_VAD
 * spatio-temporal-cube completion path (UNet bank forward / backward / Adam) and the FlowNet2 native ops.
 *
 * Conventions (the only C-ABI precedent in the reference is the cffi seam of the three
 * FlowNet2 ops, FlowNet2_src/models/components/ops/correlation/src/correlation_cuda.h:1-8,
 * correlation_cuda_kernel.h:5-39, resample2d/src/Resample2d_cuda.c:8-11, channelnorm/src/ChannelNorm_cuda.c:8-11):
 *   - every entry point returns 0 on success and a non-zero vv_status otherwise; nothing aborts or prints;
 *   - the caller owns every buffer (inputs, outputs, scratch); raw device pointers + explicit sizes, no torch types;
 *   - launches are asynchronous on the hipStream_t passed in (pass PyTorch's current stream); no host sync;
 *   - no global mutable state: re-entrant, safe with one process per GPU and with several streams;
 *   - all tensors are fp32; activations are NHWC ("pixel-major, channel-minor"), grouped tensors are [G][...]
 *     with an explicit element stride between the G independent UNets of a bank.
 *
 * Which reference code each entry point replaces is stated next to it (paths relative to the reference root).
 */
#ifndef VECVAD_HIP_H
#define VECVAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vv_stream; /* hipStream_t */

/* Every entry point returns an int: 0 on success, otherwise (status & 0xff) is one of the codes below and, for VV_ERR_LAUNCH,
 * (status >> 8) is the hipError_t the runtime reported -- the whole error travels in the return value, the library keeps no
 * last-error variable or any other mutable state between calls.  vv_status_string() renders a returned value as text. */
enum vv_status {
  VV_OK = 0,
  VV_ERR_BAD_ARG = 1,      /* unsupported shape / null pointer */
  VV_ERR_LAUNCH = 2,       /* hipGetLastError() != hipSuccess after the launch; the hipError_t sits in bits 8.. of the return */
  VV_ERR_UNSUPPORTED = 3
};

/* ---- how a convolution reads its input ("transform on load"; replaces separate BN/ReLU/pool/cat kernels) ---- */
enum vv_in_mode {
  VV_IN_PLAIN = 0, /* x                                                       */
  VV_IN_ACT = 1,   /* relu(a[c]*x + b[c])      nn.BatchNorm2d + nn.ReLU  model/unet.py:11-12,14-15 */
  VV_IN_POOL = 2,  /* 2x2 max of relu(a*x+b)   + nn.MaxPool2d(2)         model/unet.py:38          */
  VV_IN_CAT = 3,   /* [relu(a*x0+b) , x1]      torch.cat([x2, x1], 1)    model/unet.py:59          */
  VV_IN_CUBE = 4,  /* channel gather through chmap (frame erasure)       model/unet.py:178-183     */
  VV_IN_BNBWD = 5  /* BatchNorm + ReLU backward on load: src0 = dA, src1 = z (the layer's pre-BN conv output, plain),
                      a = the layer's vv_bn_bwd_sums table (group stride ab_gstride):  gk (dA [a z + b > 0] - c1 - xhat c2),
                      xhat = (z - mean) invstd -- bit-identical to the dy vv_bn_bwd_apply stores.  Per-tile vv_conv_wino only. */
};

enum vv_conv_kind {
  VV_CONV3 = 0,     /* 3x3, stride 1, pad 1 (forward, or data-gradient with flipped packed weights)     */
  VV_CONVT_FWD = 1, /* ConvTranspose2d(k3,s2,p1,op1) forward as 4 output-parity phases  model/unet.py:54 */
  VV_CONVT_DGRAD = 2 /* its data gradient = 3x3 stride-2 gather over the 2Hx2W gradient                 */
};

/* Source/destination tensor view: NHWC, channel slice [coff, coff+C) of pixels with `cstride` floats each. */
typedef struct vv_view {
  float* ptr;        /* group 0 base */
  int64_t gstride;   /* floats between groups (0: shared by all groups) */
  int32_t cstride;   /* floats per pixel */
  int32_t coff;      /* first channel of the slice */
} vv_view;

/* MFMA implicit-GEMM convolution (v_mfma_f32_32x32x2_f32, exact fp32).
 * Replaces nn.Conv2d(k3,p1) / nn.ConvTranspose2d(k3,s2,p1,op1) forward and their autograd data-gradients
 * (cuDNN in the reference: model/unet.py:10,13,54) with BatchNorm/ReLU/MaxPool/cat of the producer fused into
 * the load, bias + per-channel sum / sum-of-squares partials (BatchNorm batch statistics) fused into the store. */
/* vv_conv_params.pad0 flag: round both operands to bf16 (nearest even) on their way into LDS and contract on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- torch.autocast(bfloat16) semantics for the convolution; tensors in
 * HBM, bias, BatchNorm statistics and master weights stay fp32 (BASELINE config 4, "mixed bf16").  `w` must then be a bf16
 * panel (vv_pack_weights with mode | VV_PACK_BF16; CinP % 16 == 0). */
#define VV_CONV_BF16 1
/* with VV_CONV_BF16 and in_mode = VV_IN_PLAIN: src0 holds bf16 elements (same [B,H,W,C] indexing, gstride still in floats) --
 * the data gradient reading a dy that vv_bn_bwd_apply stored as bf16 (VV_BNBWD_DZ_BF16): same values as rounding on load, half
 * the bytes */
#define VV_CONV_SRC_BF16 2
/* with VV_CONV_BF16, VV_CONV3 / VV_CONVT_DGRAD: `out` is stored as bf16 (nearest even; same element indexing, gstride in
 * floats) and `stats` sums the stored values -- activation gradients in bf16, torch.autocast's dtype for them; read back by
 * vv_bn_bwd_* (VV_BNBWD_DA_BF16), by the transposed conv's data / weight gradient (VV_CONV_SRC_BF16 / VV_WGRAD_DY_BF16).
 * The tile is stored as 16-byte items of 8 channels: out.coff and out.cstride (and out1.coff) must be multiples of 8 elements and
 * the tensor base 16-byte aligned, else VV_ERR_BAD_ARG.  (VV_CONVT_FWD with VV_CONV_ALLSRC_BF16 stores single elements: no such rule.) */
#define VV_CONV_OUT_BF16 8
/* with VV_CONV_BF16 (any kind; modes PLAIN / ACT / CAT): EVERY source tensor of the launch holds bf16 elements -- pre-BN conv
 * outputs written with VV_CONV_OUT_BF16 (then also allowed on forward and VV_CONVT_FWD launches: torch.autocast's output dtype),
 * pooled / frame-erased inputs written by vv_pool_act / vv_cube_erase with their bf16 switch.  coff / cstride / csplit stay in
 * elements, gstride in floats. */
#define VV_CONV_ALLSRC_BF16 16
/* VV_CONV3 launches of vv_conv_mfma / vv_conv_wino: out = max(conv + bias, 0).  The eval-mode path (test.py:255-257,312-345): with
 * running-statistics BatchNorm the affine map is a constant of the model, so vv_fold_bn folds it into the filter and the bias once per
 * loaded model, the producing convolution applies the ReLU, and every consumer reads its input as VV_IN_PLAIN. */
#define VV_CONV_RELU 32
/* A/B switch: an all-bf16 3x3 launch (VV_CONV_BF16 | VV_CONV_OUT_BF16 | VV_CONV_ALLSRC_BF16 or VV_CONV_SRC_BF16) normally runs the
 * GEMM-shaped kernel of round 4 (vv_conv_bf16.hip, 256-pixel tiles on every level); with this flag it stays on the round-3
 * kernel (128-pixel tiles on the 16x16 / 8x8 / 4x4 levels).  vv_conv_ntiles2 follows the same flags. */
#define VV_CONV_NO_GEMM16 64
/* A/B switch: vv_conv_wino runs the 32x32-level launches with at most 32 input channels on the persistent LDS-DMA ring kernel of
 * round 5 (bit-identical results); with this flag they stay on the per-tile kernel. */
#define VV_CONV_NO_RING 128
/* A/B switches of vv_conv_mfma's fp32 VV_CONVT_FWD / VV_CONVT_DGRAD launches on the 128-pixel tiles (forward: 8x8 / 4x4 input; data
 * gradient: 16x16 / 8x8 / 4x4 output).  With Cout % 64 == 0 such a launch runs 64-wide N tiles (each staged input tile serves 64 output
 * channels) when it still has a workgroup for every slot of the chip, else 32-wide ones; results, `stats` and bn_partial rows are
 * bit-identical either way.  VV_CONV_CONVT_NARROW forces the 32-wide tiles, VV_CONV_CONVT_WIDE the 64-wide ones wherever they exist
 * (Cout % 64 != 0, VV_IN_POOL / VV_IN_CUBE sources, other levels and the bf16 kernels ignore it); NARROW wins over WIDE.  Environment,
 * read once, for launches without these bits: VV_CONVT_WIDE=0 keeps every launch 32-wide, VV_CONVT_WIDE=2 runs every launch that has a
 * wide form 64-wide whatever its workgroup count. */
#define VV_CONV_CONVT_NARROW 256
#define VV_CONV_CONVT_WIDE 512
typedef struct vv_conv_params {
  int32_t kind;      /* vv_conv_kind */
  int32_t in_mode;   /* vv_in_mode */
  int32_t G, B;      /* groups (UNets), cubes */
  int32_t H, W;      /* CONV3: image size; CONVT_FWD: INPUT size (output is 2H x 2W); CONVT_DGRAD: OUTPUT size
                        (= the transposed conv's input size; the gradient read is 2H x 2W) */
  int32_t Cin;       /* GEMM-K channels actually present */
  int32_t CinP;      /* Cin rounded up to the packing granule (multiple of 16; 8 for CONVT_DGRAD) */
  int32_t Cout;      /* GEMM-N channels (multiple of 32) */
  vv_view src0;      /* primary input */
  const float* a;    /* per-channel scale of src0's BatchNorm (VV_IN_ACT/POOL/CAT), [G][Cact] */
  const float* b;    /* per-channel shift */
  int64_t ab_gstride;
  vv_view src1;      /* VV_IN_CAT: second input (plain) */
  int32_t csplit;    /* VV_IN_CAT: channels [0,csplit) come from src0 */
  int32_t pad0;      /* flags: VV_CONV_BF16 (vv_conv_mfma only) */
  const int32_t* chmap; /* VV_IN_CUBE: [G][CinP] source channel or -1 (zero) */
  const float* w;    /* packed weights [9][CinP/8][2][Cout][4]  (see vv_pack_weights) */
  int64_t w_gstride;
  const float* bias; /* [G][Cout] or NULL */
  int64_t bias_gstride;
  vv_view out;       /* output */
  float* stats;      /* NULL or [G][ntiles][2][Cout] partial sums (sum, sum of squares) over valid pixels; ntiles = vv_conv_ntiles2 of
                        the launch's kind / pad0.  VV_CONVT_FWD keeps no column sums: such a launch with stats != NULL returns
                        VV_ERR_UNSUPPORTED (fp32 and bf16) */
  /* vv_conv_wino only, data-gradient launches: the first reduction pass of the BatchNorm backward that consumes this output
   * (vv_bn_bwd_reduce) done in the epilogue.  out = dA of the producing layer's activation relu(a z + b); with z that layer's
   * conv output [G][B*H*W][Cout] (pixel stride Cout) the kernel also leaves  sum dz, sum dz * xhat  per pixel tile, dz = dA [a z + b > 0],
   * xhat = (z - mean) invstd, in bn_partial [G][ntiles][2][Cout] -- the layout vv_bn_bwd_apply reads with VV_BNBWD_PARTIALS_PER_TILE.
   * a / b / mean / invstd: [G][Cout] each, group stride bn_gstride.  bn_partial == NULL: off.
   * vv_conv_mfma takes the same fields for all-bf16 3x3 launches with Cout % 64 != 0 on the 32x32 level (z then holds bf16
   * elements; rows per vv_conv_ntiles(B,H,W), read with VV_BNBWD_PARTIALS_PER_CTILE); other launches with bn_partial set are refused. */
  const float* bn_z; int64_t bn_z_gstride;
  const float* bn_a; const float* bn_b; const float* bn_mean; const float* bn_invstd; int64_t bn_gstride;
  float* bn_partial;
  /* vv_conv_mfma, bf16-output 3x3 launches (VV_CONV_BF16 | VV_CONV_OUT_BF16) only: optional second output view.  Output channels
   * [osplit, Cout) go to out1 (as its channels [0, Cout - osplit)), channels [0, osplit) to out: the data gradient of a concat
   * layer leaves as two dense tensors, one per consumer (skip half -> BatchNorm backward, upsampled half -> transposed-conv
   * backward) -- with 32 bf16 channels per half an interleaved pixel row gives each consumer 64 useful bytes of every 128 fetched.
   * osplit a multiple of 32; out1.cstride == out.cstride; out1.gstride == out.gstride.  out1.ptr == NULL: off. */
  vv_view out1;
  int32_t osplit;
  int32_t pad1;
} vv_conv_params;

int vv_conv_mfma(const vv_conv_params* p, vv_stream stream);
/* number of pixel tiles the kernel uses for this (B,H,W): rows of the `stats` partial array */
int vv_conv_ntiles(int32_t B, int32_t H, int32_t W);
/* the same for a launch with these `kind` / pad0 `flags`: the bf16 3x3 kernels use 128-pixel tiles on the 8x8 / 4x4 levels; the fp32
 * VV_CONVT_DGRAD kernel uses them on the 16x16 / 8x8 / 4x4 levels, where this returns vv_convt_dgrad_ntiles(B, H, W, 0) */
int vv_conv_ntiles2(int32_t B, int32_t H, int32_t W, int32_t kind, int32_t flags);
/* pixel tiles of a VV_CONVT_DGRAD launch of vv_conv_mfma (H x W = its output = the transposed conv's INPUT resolution; flags: the
 * launch's pad0, only VV_CONV_BF16 matters) = the rows of bn_partial such a launch leaves; -1 for an unsupported size */
int vv_convt_dgrad_ntiles(int32_t B, int32_t H, int32_t W, int32_t flags);

/* Weight-gradient (autograd of nn.Conv2d / nn.ConvTranspose2d wrt weight; cuDNN in the reference).
 * dW[tap][ci][co] = sum_pixels act[pixel+tap][ci] * dy[pixel][co]  (CONV3)
 * dW[tap][ci][co] = sum_pixels act[pixel][ci] * dy[2*pixel-1+tap][co] (CONVT)
 * Deterministic split-K: each workgroup-wave writes its own partial slab, vv_wgrad_reduce sums them in fixed order. */
typedef struct vv_wgrad_params {
  int32_t kind;      /* VV_CONV3 or VV_CONVT_FWD (meaning: weight gradient of the transposed conv) */
  int32_t in_mode;   /* how the layer input (act) is read, as in the forward */
  int32_t G, B, H, W; /* H,W: resolution of `act` pixels the GEMM-K runs over (CONVT: the transposed conv's input) */
  int32_t Cin, CinP, Cout;
  int32_t ksplit;    /* pixel-tile split factor */
  vv_view src0; const float* a; const float* b; int64_t ab_gstride;
  vv_view src1; int32_t csplit;
  int32_t pad0;      /* flags: bit 8 (256) = Winograd F(2x2,3x3) form for VV_CONV3 (dU = sum_tiles V^T dM, dg = G^T dU G; same
                        tiles, k-split and slabs, 2.25x fewer MFMA cycles, a few ulp from the direct form; W == H in {32,16,8,4};
                        three workgroups per CU: pick ksplit for 768 workgroup slots); low bits: bring-up */
  const int32_t* chmap;
  vv_view dy;        /* gradient wrt the conv output (CONV3: HxW; CONVT: 2Hx2W) */
  float* partial;    /* [G][nslab][9][32][32] with nslab = (CinP/32... see vv_wgrad_nslab) */
  int64_t partial_gstride;
  /* dy_bn != NULL: `dy` holds dA (the gradient wrt relu(bn(z))) and the operand is formed on load as VV_IN_BNBWD does, from dA, z
   * (dy_z: [B,H,W,Cout] plain) and the vv_bn_bwd_sums table dy_bn (group stride dy_bn_gstride).  VV_CONV3 with the Winograd flag
   * (pad0 bit 8) only. */
  vv_view dy_z;
  const float* dy_bn; int64_t dy_bn_gstride;
} vv_wgrad_params;

int vv_wgrad_mfma(const vv_wgrad_params* p, vv_stream stream);
int vv_wgrad_ntiles(int32_t kind, int32_t B, int32_t H, int32_t W);
/* slabs written per (ci-tile, co-tile): ksplit (the 4 waves of a workgroup are summed in LDS first) */

/* Weight gradient of the 3x3 convolution with bf16 operands / fp32 accumulation (mixed precision, BASELINE config 4;
 * torch.autocast(bfloat16) semantics of the autograd weight gradient of nn.Conv2d, model/unet.py:10,13): act (after the
 * deferred BatchNorm+ReLU) and dy are rounded to bf16 on their way into LDS, products accumulate in fp32 on
 * v_mfma_f32_32x32x16_bf16.  Same parameter block as vv_wgrad_mfma (pad0: VV_WGRAD_DY_BF16 only); kind = VV_CONV3 with H = W in {32, 16, 8, 4}, or
 * VV_CONVT_FWD (weight gradient of nn.ConvTranspose2d(k3,s2,p1,op1), model/unet.py:54) with H = W in {16, 8, 4}.
 * One workgroup covers up to 64 ci x 64 co and every ksplit-th pixel tile:  slabs per (ci-tile, co-tile) = ksplit * kw.
 * vv_wgrad_bf16_plan returns 0 when the geometry is not handled (use vv_wgrad_mfma), else 1 and
 *   *ntiles  = pixel tiles (the upper bound of ksplit),
 *   *nblocks = workgroups per group and k-split part,
 *   *kw      = slabs per workgroup and (ci-tile, co-tile) (1 today): pass ksplit * kw to vv_wgrad_reduce. */
#define VV_WGRAD_X_BF16 2    /* vv_wgrad_bf16, pad0: the layer input (src0 / src1) holds bf16 elements; needs VV_WGRAD_DY_BF16 too */
#define VV_WGRAD_DY_BF16 1   /* vv_wgrad_bf16, pad0: dy holds bf16 elements (written by vv_bn_bwd_apply with VV_BNBWD_DZ_BF16) */
int vv_wgrad_bf16(const vv_wgrad_params* p, vv_stream stream);
int vv_wgrad_bf16_plan(int32_t kind, int32_t B, int32_t H, int32_t W, int32_t CinP, int32_t Cout, int32_t* ntiles, int32_t* nblocks,
                       int32_t* kw);

/* Sum the slabs and scatter into PyTorch parameter layout:
 * CONV3 : grad[co][ci][ky][kx]   (nn.Conv2d.weight  [Cout,Cin,3,3])
 * CONVT : grad[ci][co][ky][kx]   (nn.ConvTranspose2d.weight [Cin,Cout,3,3]) */
int vv_wgrad_reduce(int32_t kind, int32_t G, int32_t Cin, int32_t CinP, int32_t Cout, int32_t nslab_per_tile,
                    const float* partial, int64_t partial_gstride, float* grad, int64_t grad_gstride,
                    vv_stream stream);
/* The same for several layers in ONE launch (e.g. every weight gradient of a data-parallel gradient bucket).  Device table, sorted by
 * block_start; entry e owns blocks [block_start, block_start + ceil(CinP/32)*(Cout/32)*36) of the launch; total_blocks = their sum.
 * Slabs of entry e start at partial + g*partial_gstride + part_off; its gradient at grads + grad_off + g*grad_gstride (floats). */
typedef struct vv_reduce_entry {
  int32_t kind, Cin, Cout, NCO, nslab, block_start;
  int64_t part_off, grad_off, grad_gstride;
} vv_reduce_entry;
int vv_wgrad_reduce_grouped(const vv_reduce_entry* table_dev, int32_t nentries, int32_t total_blocks, int32_t G, const float* partial,
                            int64_t partial_gstride, float* grads, vv_stream stream);

/* ---- weight packing: PyTorch OIHW -> MFMA B-operand panels ----
 * mode 0: conv forward      Wp[t=ky*3+kx][k=ci][n=co] = W[co][ci][ky][kx]
 * mode 1: conv data-grad    Wp[t=(2-ky)*3+(2-kx)][k=co][n=ci] = W[co][ci][ky][kx]
 * mode 2: convT forward     Wp[t=ky*3+kx][k=ci][n=co] = Wt[ci][co][ky][kx]
 * mode 3: convT data-grad   Wp[t=ky*3+kx][k=co][n=ci] = Wt[ci][co][ky][kx]
 * packed element (t,k,n) lives at (((t*KP/8 + k/8)*2 + (k%8)/4)*N + n)*4 + k%4 ; rows k >= K are zero.
 * mode | 4 (VV_PACK_BF16): the same panel as bf16 for VV_CONV_BF16 launches (KP % 16 == 0):
 * element (t,k,n) is the bf16 at index (((t*KP/16 + k/16)*2 + (k%16)/8)*N + n)*8 + k%8 from the same dst_off. */
#define VV_PACK_BF16 4
typedef struct vv_pack_entry {
  int64_t src_off;   /* floats from the group's parameter base */
  int64_t dst_off;   /* floats from the group's packed base */
  int32_t mode, K, KP, N;
} vv_pack_entry;
int vv_pack_weights(const vv_pack_entry* table_dev, int32_t nentries, int32_t G, const float* params,
                    int64_t params_gstride, float* packed, int64_t packed_gstride, int32_t max_elems,
                    vv_stream stream);

/* ---- Winograd F(2x2,3x3) form of the same 3x3 / stride 1 / pad 1 convolution (forward and data-gradient) ----
 * vv_conv_wino takes the vv_conv_params of a VV_CONV3 launch with `w` = panels from vv_pack_wino
 * ([16 = xi*4+nu][CinP/8][2][Cout][4], U = G g G^T; mode 0 forward, mode 1 data-gradient i.e. flipped + transposed filter);
 * 2.25x fewer MFMA cycles than vv_conv_mfma, fp32 throughout (results differ from the direct form by a few ulp).
 * in_mode PLAIN / ACT / CAT; CinP % 8 == 0; `stats` has vv_wino_ntiles(B, H) rows per UNet. */
int vv_conv_wino(const vv_conv_params* p, vv_stream stream);
int vv_wino_ntiles(int32_t B, int32_t H);
int vv_pack_wino(const vv_pack_entry* table_dev, int32_t nentries, int32_t G, const float* params, int64_t params_gstride,
                 float* packed, int64_t packed_gstride, int32_t max_kn, vv_stream stream);

/* ---- Winograd F(4x4,3x3) form of the same convolution (round 5; forward and data-gradient) ----
 * 2.25 matrix-core multiply-adds per output pixel and channel pair (F(2x2,3x3): 4, direct: 9), fp32 throughout; the larger transform
 * constants leave the result a few 1e-6 of the tensor's maximum from the direct form (F(2x2): a few 1e-7).
 * vv_conv_wino44 takes the vv_conv_params of a VV_CONV3 launch (same fields and contract as vv_conv_wino, incl. `stats`, the fused
 * BatchNorm-backward sums `bn_partial` and VV_CONV_RELU) with `w` = panels from vv_pack_wino44:
 * [36 = xi*6+nu][CinP/8][2][2][Cout][2], element (t, k, n) at ((((t*CinP/8 + k/8)*2 + (k%4)/2)*2 + (k%8)/4)*Cout + n)*2 + k%2,
 * U = G g G^T (6x6); mode 0 forward, mode 1 data-gradient (flipped + transposed filter).  36*KP*N floats per entry.
 * in_mode PLAIN / ACT / CAT; CinP % 8 == 0; H = W in {32, 16, 8, 4}; `stats` / `bn_partial` have vv_wino44_ntiles(B, H) rows per UNet
 * (a row = 32 tiles of 4x4 pixels). */
int vv_conv_wino44(const vv_conv_params* p, vv_stream stream);
int vv_wino44_ntiles(int32_t B, int32_t H);
int vv_pack_wino44(const vv_pack_entry* table_dev, int32_t nentries, int32_t G, const float* params, int64_t params_gstride,
                   float* packed, int64_t packed_gstride, int32_t max_kn, vv_stream stream);

/* ---- BatchNorm (nn.BatchNorm2d(eps=1e-5, momentum=0.1), model/unet.py:11,14) ----
 * train != 0: batch statistics from the conv's partial sums; writes scale/shift a,b for the consumer's load,
 *             mean / invstd for the backward pass, and updates running_mean / running_var (unbiased) in place.
 * train == 0: a,b from the running statistics. */
int vv_bn_finalize(int32_t G, int32_t C, int32_t ntiles, int64_t count, int32_t train, float momentum, float eps,
                   const float* stats, int64_t stats_gstride, const float* gamma, const float* beta,
                   int64_t param_gstride, float* running_mean, float* running_var, int64_t buf_gstride,
                   float* a, float* b, float* mean, float* invstd, int64_t ab_gstride, vv_stream stream);

/* BatchNorm + ReLU (+ MaxPool, + skip fan-in) backward, phase 1:
 * dz = (dA0 [+ route(dPool)]) * [a*y+b > 0]; writes per-block partial sums of dz and dz*xhat (not dz). */
/* vv_bnbwd_params.flags: vv_bn_bwd_apply writes dy as bf16 (nearest even; [B,H,W,C] with 2-byte elements at the same base,
 * dz_gstride still in floats) for consumers that round it to bf16 anyway (vv_conv_mfma + VV_CONV_SRC_BF16, vv_wgrad_bf16 +
 * VV_WGRAD_DY_BF16) */
#define VV_BNBWD_DZ_BF16 1
#define VV_BNBWD_PARTIALS_PER_CUBE 2   /* vv_bn_bwd_apply: `partial` holds [G][B][2][C] written by vv_outconv_bwd */
#define VV_BNBWD_Y_BF16 8              /* y holds bf16 elements (VV_CONV_OUT_BF16 on the forward launch) */
#define VV_BNBWD_DA_BF16 4             /* dA (and dpool) hold bf16 elements (VV_CONV_OUT_BF16 / vv_outconv_bwd dA_bf16) */
#define VV_BNBWD_PARTIALS_PER_TILE 16  /* vv_bn_bwd_apply: `partial` holds [G][vv_wino_ntiles(B,H)][2][C] written by the data-gradient
                                          launch that produced dA (vv_conv_params.bn_partial): no vv_bn_bwd_reduce pass for that layer */
#define VV_BNBWD_PARTIALS_PER_CTILE 32 /* the same for a data-gradient launch of vv_conv_mfma (all-bf16 tensors): [G][vv_conv_ntiles(B,H,W)][2][C] */
#define VV_BNBWD_PARTIALS_PER_TTILE 128  /* ... of the transposed conv's data gradient (vv_conv_mfma, VV_CONVT_DGRAD, fp32 kernel):
                                           [G][vv_convt_dgrad_ntiles(B,H,W,0)][2][C] */
#define VV_BNBWD_PARTIALS_PER_TILE44 64 /* the same for a data-gradient launch of vv_conv_wino44: [G][vv_wino44_ntiles(B,H)][2][C] */
typedef struct vv_bnbwd_params {
  int32_t G, B, H, W, C;
  int32_t flags;
  const float* y; int64_t y_gstride;             /* pre-BN conv output [B,H,W,C] */
  const float* a; const float* b; const float* mean; const float* invstd; int64_t ab_gstride;
  vv_view dA;                                    /* gradient wrt the post-ReLU activation (same resolution) */
  const float* dpool; int64_t dpool_gstride;     /* NULL or gradient wrt maxpool2(act) [B,H/2,W/2,C] */
  float* dz; int64_t dz_gstride;                 /* out [B,H,W,C] */
  float* partial;                                /* [G][nblk][2][C] */
} vv_bnbwd_params;
int vv_bn_bwd_reduce(const vv_bnbwd_params* p, vv_stream stream);
int vv_bn_bwd_nblk(int32_t B, int32_t H, int32_t W, int32_t C);
/* phase 2: sums the partials (fixed order, fp64), writes dgamma/dbeta, then re-reads dA and y and writes
 * dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)) into p->dz (dz itself is never materialised). */
int vv_bn_bwd_apply(const vv_bnbwd_params* p, const float* gamma, int64_t param_gstride, float* dgamma, float* dbeta,
                    int64_t grad_gstride, float* scratch /* [G][2][C] */, vv_stream stream);
/* phase 2 without the apply pass: sums the partials exactly as vv_bn_bwd_apply does, writes dgamma/dbeta and the per-channel table
 * [G][VV_BNBWD_TAB_ROWS][C] (group stride table_gstride floats) that consumers reading dA and z with VV_IN_BNBWD (data gradient) or
 * vv_wgrad_params.dy_bn (weight gradient) form dy from.  p->dz is not used; fp32 tensors only, no dpool. */
#define VV_BNBWD_TAB_ROWS 7   /* rows: a, b, mean, invstd, gk = gamma * invstd, c1 = mean(dz), c2 = mean(dz * xhat) */
int vv_bn_bwd_sums(const vv_bnbwd_params* p, const float* gamma, int64_t param_gstride, float* dgamma, float* dbeta,
                   int64_t grad_gstride, float* table, int64_t table_gstride, vv_stream stream);

/* ---- output 1x1 conv + squared error (model/unet.py:63-70 ; train.py:385-392,421-426 ; test.py:330-335) ----
 * out[p][co] = bias[co] + sum_c relu(a*y+b)[p][c] * W[co][c];  score[g][cube] = sum (out - target)^2;
 * optional dout[p][co] = gscale[g] * (out - target)  (gradient of lambda * MSELoss(mean)). */
typedef struct vv_outconv_params {
  int32_t G, B, HW, C;           /* HW pixels per cube (1024), C = features_root */
  const float* y; int64_t y_gstride; const float* a; const float* b; int64_t ab_gstride;
  const float* w; const float* bias; int64_t param_gstride;   /* W [oc][C], bias [oc] inside the parameter block */
  const int32_t* oc;             /* [G] output channels (3 raw / 2 flow) */
  const float* tgt0; int32_t tgt0_cstride; int32_t pad0;   /* cube NHWC [B,HW,15]; pad0 bit 0: y holds bf16 elements */
  const float* tgt1; int32_t tgt1_cstride; int32_t pad1;   /* flow NHWC [B,HW,2*T_of] */
  const int32_t* tgt_src;        /* [G] 0: tgt0, 1: tgt1 */
  const int32_t* tgt_coff;       /* [G] first target channel */
  float* out4;                   /* NULL (fused train / scoring steps: nobody reads it) or [G][B*HW][4] reconstruction (channels >= oc are 0) */
  float* score;                  /* [G][B] */
  const float* gscale;           /* NULL or [G] */
  float* dout4;                  /* NULL or [G][B*HW][4] */
} vv_outconv_params;
int vv_outconv_fwd(const vv_outconv_params* p, vv_stream stream);

/* backward of the 1x1 conv: dA[p][c] = sum_co dout[p][co] W[co][c]; dW[co][c] = sum_p dout[p][co] act[p][c];
 * db[co] = sum_p dout[p][co].  partial: [G][nblk][4*C + 4]; reduced by vv_outconv_bwd_reduce.  C = features_root: 32 or 64. */
/* bnpart != NULL: also writes the BatchNorm-backward partial sums of the layer in front of the output conv, [G][B][2][C]
 * (per cube: sum of g = dA * [act > 0], sum of g * xhat; mean / invstd: [G][ab_gstride] like a, b) -- vv_bn_bwd_apply with
 * VV_BNBWD_PARTIALS_PER_CUBE then needs no vv_bn_bwd_reduce pass for that layer. */
int vv_outconv_bwd(int32_t G, int32_t B, int32_t HW, int32_t C, const float* dout4, const float* y,
                   int64_t y_gstride, const float* a, const float* b, int64_t ab_gstride, const float* w,
                   int64_t param_gstride, float* dA, int64_t dA_gstride, float* partial, const float* mean,
                   const float* invstd, float* bnpart, int32_t flags /* bit 0: store dA as bf16 (VV_BNBWD_DA_BF16 consumer); bit 1: y holds bf16 elements */,
                   vv_stream stream);
int vv_outconv_bwd_nblk(int32_t B, int32_t HW);
/* vv_outconv_fwd followed by vv_outconv_bwd with dout = gscale * (out - target), in ONE pass over y (the fused train step: the
 * reference's loss.backward() right behind the forward, train.py:385-402): same score / dA / partial / bnpart bits as the two
 * calls, y read once, d(out) never stored (p->dout4 may be NULL; p->gscale must be given).  flags: bit 0 = dA stored as bf16,
 * bit 1 = y holds bf16 elements (must equal bit 0 of p->pad0). */
int vv_outconv_fwdbwd(const vv_outconv_params* p, float* dA, int64_t dA_gstride, float* partial, const float* mean,
                      const float* invstd, float* bnpart, int32_t flags, vv_stream stream);
int vv_outconv_bwd_reduce(int32_t G, int32_t C, int32_t nblk, const float* partial, const int32_t* oc,
                          float* dW, float* db, int64_t grad_gstride, vv_stream stream);

/* bias gradient of the transposed conv: db[co] = sum_pixels dy[p][co] (two-stage, deterministic) */
int vv_bias_grad(int32_t G, int64_t M, int32_t C, const float* dy, int64_t dy_gstride, int32_t cstride,
                 int32_t coff, float* scratch, float* db, int64_t grad_gstride, vv_stream stream);
/* The same bias gradient without a pass over the tensor: when dy is the output of a vv_conv_mfma / vv_conv_wino launch that was
 * given a `stats` array ([G][ntiles][2][C]: per-tile column sums in slot 0), db[g][j] = sum_tiles stats[g][tile][0][coff + j]
 * (fixed order, fp64).  Used for the transposed conv's bias: its output gradient is a channel slice of the concat layer's data
 * gradient (autograd of nn.ConvTranspose2d bias, model/unet.py:54). */
int vv_bias_from_partials(int32_t G, int32_t C, int32_t ntiles, int32_t coff, int32_t n, const float* partial,
                          int64_t partial_gstride, float* db, int64_t grad_gstride, vv_stream stream);

/* ---- fused Adam over one flat buffer (torch.optim.Adam(eps=1e-7), train.py:376,400-402) ---- */
int vv_adam(int64_t n, float* param, const float* grad, float* m, float* v, float lr, float beta1, float beta2,
            float eps, float bias_corr1, float bias_corr2_sqrt, float grad_scale, vv_stream stream);

/* Graph-replayable form of the same optimiser step (a captured train step must not carry host-computed bias corrections):
 *  vv_adam_tick     : t_dev[0] += 1; sc_dev[0] = lr / (1 - beta1^t), sc_dev[1] = sqrt(1 - beta2^t)   (one thread; beta as doubles)
 *  vv_adam_bucketed : Adam over param / m / v [G][U] reading sc_dev, with the gradient buffer in BUCKET-MAJOR layout -- bucket k =
 *                     columns [bounds[k], bounds[k+1]) of every UNet, contiguous as [G][width_k] at float offset G*bounds[k], so
 *                     that each data-parallel all-reduce (train.py:375) runs in place on one contiguous range.  bounds: HOST array
 *                     of nb+1 multiples of 4, bounds[0] = 0, bounds[nb] = U, nb <= 8. */
int vv_adam_tick(int64_t* t_dev, float lr, double beta1, double beta2, float* sc_dev, vv_stream stream);
/* counters[0..n) += inc on the device: BatchNorm2d's num_batches_tracked of a train-mode forward (model/unet.py:11,14 through
 * torch.nn.BatchNorm2d) -- a first-party launch, so that a captured train step holds no framework kernel */
int vv_counter_add(int64_t* counters, int32_t n, int64_t inc, vv_stream stream);
int vv_adam_bucketed(int32_t G, int64_t U, int32_t nb, const int64_t* bounds, float* param, const float* grad, float* m,
                     float* v, const float* sc_dev, float beta1, float beta2, float eps, float grad_scale, vv_stream stream);

/* ---- cube adapter (vad_datasets.py:130-168: [T,H,W,C] -> [H,W,T*C], uint8 -> float/255) ----
 * raw  uint8 [N][T][HW][3]  -> x   fp32 NHWC [B][HW][3T]   for the cubes idx[0..B)
 * flow fp32  [N][Tf][HW][2] -> xof fp32 NHWC [B][HW][2Tf]                                      */
int vv_cube_gather(int32_t B, int32_t T, int32_t Tf, int32_t HW, const int64_t* idx, const uint8_t* raw,
                   const float* flow, float* x, float* xof, vv_stream stream);

/* Small materialised inputs that keep the MFMA kernels on their fast (plain, pipelined) load path:
 *  vv_pool_act  : out[g][b,y,x,c] = max_{2x2} relu(a*y+b)    nn.MaxPool2d(2) of the activated tensor (model/unet.py:38);
 *                 1/4 of the source tensor, written once in the forward and reused by the weight-gradient.
 *  vv_cube_erase: out[g][pixel][k] = cube[pixel][chmap[g][k]] (or 0): the frame-erased input of UNet g, Cin padded to CP
 *                 (model/unet.py:178-183). */
int vv_pool_act(int32_t G, int32_t B, int32_t H2, int32_t W2, int32_t C, const float* y, int64_t y_gstride, const float* a,
                const float* b, int64_t ab_gstride, float* out, int64_t out_gstride, int32_t io_bf16 /* y and out hold bf16 */,
                vv_stream stream);
int vv_cube_erase(int32_t G, int64_t npix, int32_t Cc, int32_t CP, const float* cube, const int32_t* chmap, float* out,
                  int64_t out_gstride, int32_t out_bf16, vv_stream stream);

/* NCHW <-> NHWC for the module surface (forward(x, x_of) takes NCHW like the reference) */
int vv_nchw_to_nhwc(int32_t B, int32_t C, int32_t HW, const float* src, float* dst, vv_stream stream);
/* gathers channels [0,oc) of out4[g] into NCHW dst[b][choff + ...] ; dst has Ctot channels */
int vv_out4_to_nchw(int32_t B, int32_t HW, int32_t oc, const float* out4, float* dst, int32_t Ctot,
                    int32_t choff, vv_stream stream);
int vv_nchw_to_out4(int32_t B, int32_t HW, int32_t oc, const float* src, int32_t Ctot, int32_t choff,
                    float* out4, vv_stream stream);

/* ---- FlowNet2 native ops (forward only; FlowNet2 is inference-only in VEC_VAD, calc_optical_flow.py:56-57) ----
 * Same argument meaning as the reference's cffi functions, NCHW fp32 contiguous, stream = current stream.
 * Correlation_forward_cuda  (ops/correlation/src/correlation_cuda.c:11-93, correlation_cuda_kernel.cu:10-106):
 *   no rInput scratch is needed (bounds are predicated instead of materialising zero-padded NHWC copies).
 *   Served: kernel_size 1 with at most 24 displacements per axis and C * 128 + 256 * span bytes <= 160 KiB of LDS
 *   (span = 31 * stride1 + 2 * (max_displacement / stride2) * stride2 + 1, made odd), and any odd kernel_size > 1 by a plain
 *   kernel; the rest, an even kernel_size and corr_type_multiply != 1 return VV_ERR_UNSUPPORTED. */
int vv_correlation_fwd(const float* in1, const float* in2, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                       int32_t pad_size, int32_t kernel_size, int32_t max_displacement, int32_t stride1,
                       int32_t stride2, int32_t corr_type_multiply, vv_stream stream);
int vv_correlation_out_shape(int32_t C, int32_t H, int32_t W, int32_t pad_size, int32_t kernel_size,
                             int32_t max_displacement, int32_t stride1, int32_t stride2, int32_t* oC, int32_t* oH,
                             int32_t* oW);
/* The same op specialised to how FlowNetC uses it (FlowNetC.py:41-47,92-93,120: pad 20, kernel 1, max_displacement 20,
 * stride1 1, stride2 2, then LeakyReLU(0.1), then torch.cat with conv_redir): NHWC maps in (pixel stride `cstride` floats,
 * cstride >= C, cstride % 4 == 0, C % 16 == 0, 16-byte aligned; a pointer into the middle of a wider pixel is a slice), result * 1/C
 * through y = v > 0 ? v : slope*v written to channels [out_coff, out_coff+441) of an NHWC buffer with pixel stride out_cstride
 * (element stores: out_cstride and out_coff need no alignment).  W in {64, 128} (512- and 1024-wide inputs); other widths, C % 16 != 0
 * or a cstride that breaks the rules above return VV_ERR_UNSUPPORTED -> use vv_correlation_fwd. */
int vv_correlation_nhwc(const float* f1, const float* f2, int32_t cstride, int32_t B, int32_t C, int32_t H, int32_t W,
                        float* out, int32_t out_cstride, int32_t out_coff, float slope, vv_stream stream);
/* Resample2d_cuda_forward (ops/resample2d/src/Resample2d_cuda.c:8-11, Resample2d_kernel.cu:20-66) */
int vv_resample2d_fwd(const float* img, const float* flow, float* out, int32_t B, int32_t C, int32_t H, int32_t W,
                      int32_t fH, int32_t fW, int32_t kernel_size, vv_stream stream);
/* ChannelNorm_cuda_forward (ops/channelnorm/src/ChannelNorm_cuda.c:8-11, ChannelNorm_kernel.cu:19-51) */
int vv_channelnorm_fwd(const float* in, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t norm_deg,
                       vv_stream stream);

/* ---- FlowNet2 conv stack (forward only; FlowNet2_src/models/components/misc.py:8-44, FlowNet{C,S,SD,Fusion}.py) ----
 * Generic NHWC MFMA convolution: kind 0 = nn.Conv2d(k=R in {1,3,5,7}, stride in {1,2}, padding=(R-1)/2),
 * kind 1 = nn.ConvTranspose2d(k4, s2, p1); optional bias; y = v > 0 ? v : slope*v  (slope 0.1 = LeakyReLU, 1.0 = none).
 * src: NHWC with cstride % 4 == 0 and coff % 4 == 0 (pad channels must hold finite values); out: any channel slice of
 * the consumer's concat buffer.  Weights packed by vv_pack_conv2d: [taps][CinP/8][2][CoutP][4], zero padded.
 * kind 2 = the same nn.Conv2d in "row-K" form for the few-channel first layers (FlowNetC.py conv1: 7x7 s2 on 3 channels;
 * FlowNetSD.py conv0: 3x3 s1 on 6): src.cstride = 4 (R = 7, stride 2) or 8 (R = 3, stride 1), src.coff = 0; K runs over the
 * flattened (kx, c) run of one filter row, Cin = CinP = ceil8(R * cstride) (32 / 24), and the panel is packed with taps = R from a
 * weight tensor rearranged to [N][kx * cstride + c][ky] (zeros at the pad channels and beyond kx = R - 1).
 * Size limit: the source is loaded through 32-bit byte offsets, so B * H * W * src.cstride * 4 must stay below 2^31 bytes (2 GiB);
 * a larger source is refused with VV_ERR_UNSUPPORTED and nothing is launched.  vv_conv3x3_n2 and vv_conv2d_f16 address their source
 * with 64-bit pointers and refuse B * H * W * src_cstride >= 2^31 ELEMENTS (the pixel index is an int). */
typedef struct vv_conv2d_params {
  int32_t kind, R, stride;
  int32_t B, H, W;          /* input size */
  int32_t Cin, CinP, Cout, CoutP;
  vv_view src;
  const float* w;
  const float* bias;
  float slope;
  int32_t pad0;       /* ksplit: > 1 splits the input-channel loop over that many workgroups; `out` must then be a
                         workspace [ksplit][B*OH*OW][CoutP] (cstride = CoutP, coff = 0) finished by vv_conv2d_splitk_finish */
  vv_view out;
} vv_conv2d_params;
int vv_conv2d_mfma(const vv_conv2d_params* p, vv_stream stream);
/* The same conv(k = 3, stride 1, pad 1) [+ LeakyReLU(slope); slope 1 = none] in Winograd F(2x2, 3x3) form (fp32, a few ulp from the
 * direct form; 2.25x fewer MFMA cycles): FlowNet2's large stride-1 layers (components/misc.py:8-28 as used by FlowNetSD.py:9-103,
 * FlowNetFusion.py:9-64, FlowNetC.py / FlowNetS.py conv3_1 ... conv5_1).  `panel` = vv_pack_wino (mode 0, one entry, G = 1) of the
 * nn.Conv2d weight [Cout][Cin][3][3]: [16][CinP/8][2][Cout][4]; CinP % 8 == 0, Cout % 32 == 0, H % 2 == 0, W % 32 == 0.
 * src: NHWC, pixel stride src_cstride floats (multiple of 4), first channel src_coff; src_elems = floats in the source buffer
 * (reads of the K padding past it return zeros; pad channels inside it must be finite).  out: NHWC slice (out_cstride, out_coff). */
int vv_conv2d_wino(const float* src, int32_t src_cstride, int32_t src_coff, int64_t src_elems, const float* panel, const float* bias,
                   float slope, float* out, int32_t out_cstride, int32_t out_coff, int32_t B, int32_t H, int32_t W, int32_t CinP,
                   int32_t Cout, vv_stream stream);
int vv_conv2d_splitk_finish(const float* ws, int32_t ksplit, int64_t M, int32_t Cout, int32_t CoutP, const float* bias,
                            float slope, float* out, int32_t out_cstride, int32_t out_coff, vv_stream stream);
/* The two-channel flow heads, where a 32-wide MFMA tile would be 94 % padding:
 *  vv_conv3x3_n2  : predict_flow = nn.Conv2d(Cin, 2, 3, 1, 1) (components/misc.py:42-44).  wq = weights repacked as
 *                   [tap 9][C4P][out 2][4] (Cin zero-padded to 4*C4P, C4P*4 a multiple of 32), bias[2] or NULL.
 *  vv_deconv4x4_c2: upsampled_flow = nn.ConvTranspose2d(2, 2, 4, 2, 1) (FlowNetS.py:40-47 ...), w in PyTorch layout
 *                   [2][2][4][4].
 * NHWC in (pixel stride src_cstride, channels from 0), result through y = v > 0 ? v : slope*v into channels
 * [out_coff, out_coff+2) of an NHWC buffer with pixel stride out_cstride. */
int vv_conv3x3_n2(const float* src, int32_t src_cstride, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* wq,
                  int32_t C4P, const float* bias, float slope, float* out, int32_t out_cstride, int32_t out_coff,
                  vv_stream stream);
int vv_deconv4x4_c2(const float* src, int32_t src_cstride, int32_t B, int32_t H, int32_t W, const float* w,
                    const float* bias, float slope, float* out, int32_t out_cstride, int32_t out_coff, vv_stream stream);
/* w: Conv2d [N][K][R][R] (transposed = 0) or ConvTranspose2d [K][N][4][4] (transposed = 1); taps = R*R */
int vv_pack_conv2d(const float* w, float* packed, int32_t taps, int32_t K, int32_t KP, int32_t N, int32_t NP,
                   int32_t transposed, vv_stream stream);
/* nn.Upsample(scale_factor=4) on NCHW planes, times `scale` (flownet2.py:28,34,43-44,76,90,105,122).
 * bilinear: 0 = 'nearest', 1 = 'bilinear' with align_corners=False (torch >= 0.4), 2 = 'bilinear' with align_corners=True
 * (what 'bilinear' meant under the PyTorch 0.3 the reference's README pins for the flow extraction) */
int vv_upsample4(const float* src, float* dst, int32_t BC, int32_t H, int32_t W, int32_t bilinear, float scale,
                 vv_stream stream);

/* ---- eval mode: nn.BatchNorm2d with running statistics folded into the convolution in front of it (model/unet.py:9-16 under
 * net.eval(), test.py:255-257).  For every table entry and group g, with a[c] = gamma[c] / sqrt(running_var[c] + eps) (float64):
 *   folded[w_off + c*row + k] = a[c] * params[w_off + c*row + k]         (row = Cin*9 filter elements per output channel)
 *   folded[b_off + c]         = a[c] * (params[b_off + c] - running_mean[c]) + beta[c]
 * Offsets are in floats inside one group's block; params / folded have params_gstride / folded_gstride floats per group, bufs
 * (running statistics) bufs_gstride.  Entries the table does not name are left untouched (copy them first). */
typedef struct vv_fold_entry {
  int64_t w_off, b_off, g_off, beta_off; /* into the parameter block */
  int64_t rm_off, rv_off;                /* into the buffer block */
  int32_t cout, row;
} vv_fold_entry;
int vv_fold_bn(const vv_fold_entry* table_dev, int32_t nentries, int32_t G, const float* params, int64_t params_gstride,
               const float* bufs, int64_t bufs_gstride, float eps, float* folded, int64_t folded_gstride, vv_stream stream);

/* ---- FlowNet2 plumbing between the sub-networks (FlowNet2_src/models/flownet2.py:65-136), NHWC, no temporaries ----
 * vv_flownet_prep: inputs [B,3,2,H,W] fp32 (0..rgb_max) -> rgb_mean over (frame, H, W) per image and colour (:66-67),
 *   x = (inputs - rgb_mean) / rgb_max (:69), x6 [B,H,W,8] = cat(x1, x2) + 2 zero channels (:70-72), img0 / img1 [B,H,W,4] =
 *   the two frames + 1 zero channel (FlowNetC's siamese stem).  workspace: vv_flownet_prep_workspace_bytes(B) bytes, 16-byte
 *   aligned like every tensor here.  H * W must be even (the mean is summed with 16-byte loads per colour); an odd H * W returns
 *   VV_ERR_UNSUPPORTED.
 * vv_warp_pack12: flow = Upsample x4 (mode as vv_upsample4's `bilinear`) of flow2 [B,H/4,W/4,flow_cstride] (channels 0,1)
 *   times `scale` (:76,90); out12 [B,H,W,12] = cat(x6[0:6], Resample2d(img1, flow), flow / div_flow, ChannelNorm(x1 - warped))
 *   (:79-86, 93-100).
 * vv_fusion_pack11: s2 = nearest x4 of s2_flow2 * div_flow (:105), sd = nearest x4 of sd_flow2 / div_flow (:122);
 *   out12 [B,H,W,12] = cat(x1, sd, s2, |sd|, |s2|, |x1 - warp(img1, sd)|, |x1 - warp(img1, s2)|) + 1 zero channel (:132-136). */
int64_t vv_flownet_prep_workspace_bytes(int32_t B);
int vv_flownet_prep(const float* inputs, int32_t B, int32_t H, int32_t W, float rgb_max, void* workspace,
                    int64_t workspace_bytes, float* x6, float* img0, float* img1, vv_stream stream);
int vv_warp_pack12(const float* x6, const float* img1, const float* flow2, int32_t flow_cstride, int32_t B, int32_t H,
                   int32_t W, int32_t mode, float scale, float div_flow, float* out12, vv_stream stream);
int vv_fusion_pack11(const float* x6, const float* img1, const float* s2_flow2, int32_t s2_cstride, const float* sd_flow2,
                     int32_t sd_cstride, int32_t B, int32_t H, int32_t W, float div_flow, float* out12, vv_stream stream);

/* ---- cube extraction (vad_datasets.py:70-93 get_foreground, calc_optical_flow.py:46-59,82) ----
 * One launch crops n boxes out of T decoded frames and resizes each crop with cv2.resize's default INTER_LINEAR
 * arithmetic (uint8: 11-bit fixed point, bit-exact; float32: unfused fp32; exact 2x decimation -> 2x2 area mean;
 * equal size -> copy).
 *   frames [T][H][W][C] uint8 (is_f32 = 0) or float32 (is_f32 = 1)  -- the layout cv2.imread / np.load hand over
 *   crops  int32 [n][4] = x_min, y_min, x_max, y_max with 0 <= min < max <= W|H  (ceil + slice clipping done by the host)
 *   out    [n][T][oh][ow][C], same dtype  (= the [N,T,32,32,C] cube layout of the *_foreground_*.npy files)        */
int vv_crop_resize(const void* frames, int32_t is_f32, int32_t T, int32_t H, int32_t W, int32_t C, const int32_t* crops,
                   int32_t n, int32_t oh, int32_t ow, void* out, vv_stream stream);

/* ---- cubes of many frames per launch (test.py's direct path, foreground.extract_device): every box brings its own frame window ----
 * vv_cube_cut: the arithmetic of vv_crop_resize per output value (one shared device function), for N boxes of a chunk of F decoded
 *   frames that are each held once.
 *   frames [F][H][W][C] uint8 (is_f32 = 0) or float32 (is_f32 = 1)
 *   crops  int32 [N][4] as for vv_crop_resize
 *   win    int32 [N][T] = the frames of box i's temporal context as indices into the chunk, each in [0, F); repeats allowed
 *          (border modes repeat frames)
 *   slot   int32 [N] = the cube of the store that box i fills, < out_slots; boxes with slot < 0 are skipped; distinct boxes
 *          must name distinct slots, in any order
 *   The tables live in device memory, so the entry points cannot read them: the caller checks them (vec_vad_amd/extract.py
 *   check_tables raises on a bad one).  Against a table that breaks these rules the kernels only protect memory: such a crop or
 *   slot is skipped, such a window index is clamped, and the outputs for that box mean nothing.
 *   out    [out_slots][T][P][P][C], same dtype (the CubeStore / *_foreground_*.npy layout); untouched outside the named slots
 * vv_cube_energy: energy[i] = sum of squares of box i's resized float32 patch [T][P][P][C] (no patch is written), each value widened
 *   to float64 before squaring, divided by T (train.py:159-170: the mean over the context frames); keep[i] = energy[i] > thr.
 *   One workgroup per box, fixed summation order (strided per-thread sums, LDS tree), no atomics: bit-identical run to run.
 *   P <= 1024 and T * P * P <= INT32_MAX, else VV_ERR_BAD_ARG. */
int vv_cube_cut(const void* frames, int32_t is_f32, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* crops,
                const int32_t* win, const int32_t* slot, int32_t n, int32_t T, int32_t P, void* out, int64_t out_slots,
                vv_stream stream);
int vv_cube_energy(const float* frames, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* crops, const int32_t* win,
                   int32_t n, int32_t T, int32_t P, double thr, double* energy, uint8_t* keep, vv_stream stream);

/* ---- optical flow of a chunk of decoded frames (test.py's direct path with [mi355x] direct_flow; calc_optical_flow.chunk_flows) ----
 * The two whole-frame resizes of calc_optical_flow.py:46-59,82 around FlowNet2, each value that of vv_crop_resize (the same device
 * function), written in the layout the neighbour wants; one thread per output pixel, no framework op in between.
 * vv_flow_pairs_prep: FlowNet2's input for N frame pairs.
 *   frames uint8 [F][H][W][C], C = 1 | 3 (else VV_ERR_BAD_ARG)
 *   pairs  int32 [N][2] = (first, second) frame of pair n as indices into the chunk, each in [0, F); the caller checks them
 *          (vec_vad_amd/extract.py flow_pairs_prep raises), the kernel only clamps
 *   out    float32 [N][3][2][oh][ow]: out[n][c][k][y][x] = (float) resize_u8(frames[pairs[n][k]] -> oh x ow)[y][x][c]; with C = 1 the
 *          one plane is written three times
 * vv_flow_resize_back: FlowNet2's output back at frame size, vectors not rescaled.
 *   flow   float32 planar [N][2][fh][fw]
 *   rows   int32 [N] = the field of `out` that pair n fills; rows[n] < 0 skips pair n; a row >= out_rows is refused by the caller
 *          and skipped by the kernel; distinct pairs must name distinct rows
 *   out    float32 [out_rows][H][W][2], 8-byte aligned: out[rows[n]][y][x][c] = resize_f32(flow[n][c] -> H x W)[y][x]; untouched
 *          outside the named rows
 * N = 0 returns VV_OK and writes nothing (null tables allowed). */
int vv_flow_pairs_prep(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* pairs, int32_t N,
                       int32_t oh, int32_t ow, float* out, vv_stream stream);
int vv_flow_resize_back(const float* flow, int32_t N, int32_t fh, int32_t fw, const int32_t* rows, int32_t H, int32_t W,
                        float* out, int64_t out_rows, vv_stream stream);

/* ---- frame-by-frame scoring (vec_vad_amd/stream.py): one frame's boxes from a ring of recent frames to a frame score ----
 * Every table below lives in device memory and is read by the kernels, so the launch arguments stay the same from frame to frame.
 * vv_stream_cut: for the n[0] <= cap boxes of one frame (n[0] is clamped to [0, cap]) the raw cube and the flow cube of box b go into
 *   slot b of a fixed store in CubeStore layout, and keep[b] = the motion test of vv_cube_energy at `thr`.
 *   raw_ring  uint8 [R][H][W][C], flow_ring float32 [Rf][H][W][2]: the recent frames and their flow fields
 *   crops     int32 [cap][4] as for vv_crop_resize (rows >= n[0] are not read)
 *   raw_win   int32 [T], flow_win int32 [Tf]: the ring slots of the frame's two context windows (clamped to the rings; repeats allowed)
 *   raw_store uint8 [cap][T][P][P][C] = the bytes vv_cube_cut writes for the same frames, crop and window; flow_store float32
 *             [cap][Tf][P][P][2] likewise; keep uint8 [cap]; energy double [cap] or NULL = the value of vv_cube_energy (same device
 *             function: same float64 sum in the same order).  Slots >= n[0] of all four are not written.  A crop outside the frame
 *             (the caller checks) is dropped: keep 0, nothing cut.  P <= 1024, T * P * P and Tf * P * P <= INT32_MAX.
 * vv_stream_scores: raw / of float32 [cap] = the per-cube error sums of a scoring launch over the store (of == NULL drops the flow
 *   term), stats double [4] = (mu_r, sd_r, mu_o, sd_o) of the block's model or NULL for a block without one, mask uint8 [cap] = the
 *   boxes that belong to the block.  Box b counts iff b < n[0], keep[b] and mask[b]; then box_scores[b] = the score of vv_cube_scores
 *   (the same device function; +big without a model) and frame_score[0] = max(frame_score[0], box_scores[b]); a box below n[0] that
 *   does not count gets -big and its errors are not read, slots >= n[0] are not written: whatever they hold, NaN and Inf included, stays
 *   out of the maximum.  The caller starts frame_score[0] at -big; one workgroup, no atomics.
 * vv_stream_boxes: the tables of vv_stream_cut / vv_stream_scores for motion boxes that exist only on the device (StreamScorer with
 *   boxes = 'motion').  count int32 [1] and boxes int32 [mcap][4] = (x1, y1, x2, y2) as vv_mask_boxes leaves them for one window
 *   (count may exceed mcap; rows >= min(count, mcap) are not read); slots 0..n_ap-1 of the tables hold the host's appearance boxes
 *   and are not touched.  With m = min(count, mcap, cap - n_ap): n[0] = n_ap + m, dropped[0] = count - m, and for j < m in slot
 *   s = n_ap + j: boxes_out int32 [cap][4] = the box; crops int32 [cap][4] = max(x1,0), max(y1,0), min(x2,W), min(y2,H)
 *   (extract.boxes_to_crops on integers); masks uint8 [hb*wb][cap]: masks[hi*wb + wi][s] = 1 for every cell (hi, wi) of
 *   utils.calc_block_idx(x1, x2, y1, y2, h_step, w_step, block_mode) -- float64, int(((p + c) / 2.0) / step) per probe point, each
 *   operation rounded on its own -- that lies inside the hb x wb grid, provided rows [y1, y2) x columns [x1, x2) touch a pixel of a
 *   grid_h x grid_w mask under Python's slicing (scoring.box_paints); every other byte of columns n_ap..cap-1 of masks is set to 0.
 *   Slots >= n[0] of crops and boxes_out are not written.  One workgroup.  0 <= n_ap <= cap, cap >= 1, block_mode >= 1 (1: centre;
 *   2..8: + edge mid-points; >= 9: + corners), steps > 0, else VV_ERR_BAD_ARG without a launch. */
int vv_stream_cut(const uint8_t* raw_ring, int32_t R, const float* flow_ring, int32_t Rf, int32_t H, int32_t W, int32_t C,
                  const int32_t* n, const int32_t* crops, const int32_t* raw_win, const int32_t* flow_win, int32_t cap, int32_t T,
                  int32_t Tf, int32_t P, double thr, uint8_t* raw_store, float* flow_store, uint8_t* keep, double* energy,
                  vv_stream stream);
int vv_stream_scores(const float* raw, const float* of, const double* stats, double w_raw, double w_of, double big,
                     const uint8_t* keep, const int32_t* n, const uint8_t* mask, int32_t cap, double* box_scores, double* frame_score,
                     vv_stream stream);
int vv_stream_boxes(const int32_t* count, const int32_t* boxes, int32_t mcap, int32_t n_ap, int32_t cap, int32_t H, int32_t W,
                    int32_t grid_h, int32_t grid_w, int32_t hb, int32_t wb, double h_step, double w_step, int32_t block_mode,
                    int32_t* n, int32_t* dropped, int32_t* crops, uint8_t* masks, int32_t* boxes_out, vv_stream stream);

/* ---- several cameras in one scorer (vec_vad_amd/multistream.py): the two launches above over a camera dimension, ONE launch each for
 * `cams` cameras.  All tables live in device memory; the values are those of the single-camera entry points called per camera (the
 * same device functions).
 * vv_stream_cut_multi: one workgroup per (camera, slot).
 *   raw_ring  uint8 [cams*R][H][W][C], flow_ring float32 [cams*Rf][H][W][2]: camera k's frames and fields in slots k*R.. and k*Rf..
 *   n         int32 [cams], each clamped to [0, cap]; crops int32 [cams][cap][4] (rows >= n[k] of camera k are not read)
 *   raw_win   int32 [cams][T], flow_win int32 [cams][Tf]: ABSOLUTE ring slots, clamped into the whole rings
 *   Box b < n[k] of camera k goes to store slot k*cap + b: raw_store uint8 [cams*cap][T][P][P][C], flow_store float32
 *   [cams*cap][Tf][P][P][2], keep uint8 [cams*cap], energy double [cams*cap] or NULL.  Every other slot keeps what it holds.  A crop
 *   outside the frame is dropped: keep 0, nothing read.  VV_ERR_BAD_ARG as vv_stream_cut, and for cams <= 0, cams > 65535 or
 *   cams * R, cams * Rf, cams * cap > INT32_MAX.
 * vv_stream_scores_multi: one workgroup per camera; one block's share of `cams` frame scores.
 *   raw / of float32 [cams*cap], stats double [4] or NULL, keep and mask uint8 [cams*cap], n int32 [cams].  Box b of camera k counts
 *   iff b < n[k], keep[k*cap+b] and mask[k*cap+b]; then box_scores[k*box_stride + b] = the score of vv_stream_scores (+big without
 *   stats) and frame_score[k*frame_stride] is max-accumulated; a box below n[k] that does not count gets -big and its errors are not
 *   read; slots >= n[k] are neither read nor written, and a camera with n[k] = 0 leaves its cell as it was.  Strides in elements,
 *   box_stride >= cap and frame_stride >= 1 (the cameras' rows and cells must not overlap), cams >= 1, else VV_ERR_BAD_ARG. */
int vv_stream_cut_multi(const uint8_t* raw_ring, int32_t R, const float* flow_ring, int32_t Rf, int32_t H, int32_t W, int32_t C,
                        int32_t cams, const int32_t* n, const int32_t* crops, const int32_t* raw_win, const int32_t* flow_win,
                        int32_t cap, int32_t T, int32_t Tf, int32_t P, double thr, uint8_t* raw_store, float* flow_store,
                        uint8_t* keep, double* energy, vv_stream stream);
int vv_stream_scores_multi(const float* raw, const float* of, const double* stats, double w_raw, double w_of, double big,
                           const uint8_t* keep, const int32_t* n, const uint8_t* mask, int32_t cams, int32_t cap, double* box_scores,
                           int64_t box_stride, double* frame_score, int64_t frame_stride, vv_stream stream);

/* ---- training from pushed frames (vec_vad_amd/stream_train.py): the kept cubes of one vv_stream_cut round appended to ONE large
 * training store, behind the round's cut on the same stream, with no word to the host.
 * vv_stream_append: one workgroup per slot of the round.
 *   raw_slots uint8 [cap][raw_cube_bytes], flow_slots float32 [cap][flow_cube_bytes / 4], keep uint8 [cap], n int32 [1]: the stores,
 *             keep flags and box count of vv_stream_cut; n[0] is read on the device and clamped to [0, cap]
 *   masks     uint8 [cells][cap]: the round's block rows (the descriptor's, or those of vv_stream_boxes); NULL only with cells == 0
 *   boxes     int32 [cap][4] (the boxes_out of vv_stream_boxes) or NULL
 *   frame     the running frame index; slot0: the box index of slot 0 (round * cap)
 *   cursor_in, cursor_out int32 [1]: two DIFFERENT cells, which the host alternates per launch
 *   raw_store uint8 [capacity][raw_cube_bytes], flow_store float32 [capacity][flow_cube_bytes / 4], meta int32 [capacity][2],
 *             meta_boxes int32 [capacity][4], meta_cells uint8 [capacity][cells]
 *   The kept slots are the b < n[0] with keep[b] != 0, in ascending b; the j-th of them goes to store cube d = cursor_in[0] + j.  If
 *   0 <= d < capacity: its raw_cube_bytes and flow_cube_bytes are copied unchanged to cube d of the two stores, meta[d] = (frame,
 *   slot0 + b), meta_boxes[d] = boxes[b] (four zeros when boxes == NULL) and meta_cells[d][k] = masks[k * cap + b] for k < cells.  A
 *   cube with d >= capacity is not written anywhere.  cursor_out[0] = cursor_in[0] + (number of kept slots), NOT clamped, so that the
 *   host can say how many cubes would have been needed.  Nothing else is written, whatever the slots >= n[0] and the unkept slots
 *   hold (NaN and Inf included), and no store cube outside [cursor_in[0], cursor_in[0] + kept).
 *   Every workgroup derives its slot's rank from keep[0..b) itself (a count in LDS); workgroup 0 alone writes cursor_out.  Ordinary
 *   vector loads and stores only, no atomics, no workgroup waits for another; bit-identical run to run.  The copy uses 16-byte accesses
 *   where source, destination and size allow (always for P = 32 on 16-byte aligned stores), else a byte path.  The entry point
 *   allocates nothing and copies nothing.  VV_ERR_BAD_ARG without a launch: cap < 1, cells < 0, capacity < 0, a negative cube size; NULL
 *   n, keep, cursor_in, cursor_out, raw_slots, flow_slots, raw_store, flow_store, meta, meta_boxes or meta_cells; NULL masks with
 *   cells > 0; cursor_in == cursor_out. */
int vv_stream_append(const uint8_t* raw_slots, const float* flow_slots, const uint8_t* keep, const int32_t* n, int32_t cap,
                     int64_t raw_cube_bytes, int64_t flow_cube_bytes, const uint8_t* masks, int32_t cells, const int32_t* boxes,
                     int32_t frame, int32_t slot0, const int32_t* cursor_in, int32_t* cursor_out, int64_t capacity, uint8_t* raw_store,
                     float* flow_store, int32_t* meta, int32_t* meta_boxes, uint8_t* meta_cells, vv_stream stream);

/* ---- a streamed frame's score mask, its trailing-window mean and the tables its picture needs (StreamScorer with masks / smooth /
 * render): what test.py's paint, smooth and render stages compute for a finished split, for ONE issued frame, with the box count and
 * the motion boxes still on the device.  VV_STREAM_UNPAINTED (-100000.0, = VV_SMOOTH_UNPAINTED = VV_RENDER_UNPAINTED) is the background.
 * vv_stream_paint: one launch.  scores double [rows][width] = the box-score rows vv_stream_scores left (one row per scored block; rows
 *   or width may be 0); n int32 [1] on the device, clamped to [0, width] = the boxes of the frame (all rounds together).  For b < n:
 *   box_max[b] = max(unpainted, scores[0][b], ..., scores[rows-1][b]) and the rectangle of box b is rects[b] = (y0, y1, x0, x1) for
 *   b < n_host -- resolved by the host as for vv_paint_masks -- and else, from boxes int32 [width][4] = (x1, y1, x2, y2) (the
 *   boxes_out of vv_stream_boxes), y0, y1 = slice(y1, y2).indices(h)[:2] and x0, x1 = slice(x1, x2).indices(w)[:2] on integers (a
 *   negative bound counts from the end and clips at 0, a bound past the edge clips to it), which is WRITTEN to rects[b].  boxes == NULL:
 *   every rectangle is the host's.  mask double [h][w] is written whole: mask[y][x] = the largest box_max[b] over the boxes b < n whose
 *   rectangle holds y0 <= y < y1 and x0 <= x < x1, unpainted where there is none -- what vv_paint_masks paints with box_max over a
 *   background of unpainted; its maximum is the frame score of vv_stream_scores.  frame_off int32 [2] = (0, n), the CSR table
 *   vv_render_overlay wants for this one frame.  Slots >= n of scores, rects and boxes are never read and those of box_max and rects
 *   never written, whatever they hold.  Any number of boxes, staged through LDS VV_STREAM_PAINT_STAGE at a time; a thread owns two
 *   consecutive pixels; no atomics, no fill launch.  rects 16-byte aligned and distinct from boxes.  VV_ERR_BAD_ARG: negative sizes,
 *   h * w > 2^31 - 513, NULL n / frame_off, NULL mask with h * w > 0, NULL rects / box_max with width > 0, NULL scores with rows and
 *   width > 0, misaligned rects.  NaN scores are outside the domain.
 * vv_stream_smooth: the filter of vv_smooth_masks with a TRAILING temporal window, over a ring of the last masks.  ring double
 *   [K][h][w] (vv_stream_paint output per slot); win int32 [1 + kt] on the device = the number of frames of the window (clamped to
 *   1..kt), then their ring slots in ascending frame order (clamped to [0, K)), the last being the issued frame; entries behind the
 *   count are not read.  Two launches: (a) the X and Y passes of vv_smooth_masks -- the same V, N, A / a, B / b, ascending offsets from
 *   +0.0, through the same device function -- for the issued frame's slot ONLY, stored into that slot of Bsum double [K][h][w] and bcnt
 *   uint16 [K][h][w]; the sums of the window's earlier frames are the ones their own calls left there.  (b) C = sum of B over the
 *   window's slots in the table's order from +0.0, c likewise, out[y][x] = painted ? C / (double)c : unpainted with `painted` read from
 *   the issued frame's slot of the ring and one IEEE division, and partial[g] = the maximum of out over pixels [256 g, 256 g + 256):
 *   vv_stream_smooth_partials(h, w) = ceil(h * w / 256) doubles whose maximum is the smoothed frame score (a maximum does not round;
 *   no atomics).  The result equals vv_smooth_masks with the window 2 kt - 1 on a buffer that ends at the issued frame, read at its
 *   last frame, bit for bit.  A slot that no entry of win names is not read, whatever it holds.  1 <= kt <= VV_SMOOTH_MAX (any parity),
 *   ks odd in 1..VV_SMOOTH_MAX (c <= 33 * 33^2 < 2^16); K >= 1.  h * w == 0: VV_OK, nothing is written.  VV_ERR_BAD_ARG: bad windows,
 *   K < 1, negative sizes, h * w >= 2^31, a NULL pointer with something to do. */
#define VV_STREAM_PAINT_STAGE 256
#define VV_STREAM_UNPAINTED (-100000.0)
int vv_stream_paint(const double* scores, int32_t rows, int32_t width, const int32_t* n, int32_t n_host, int32_t* rects,
                    const int32_t* boxes, int32_t h, int32_t w, double* mask, double* box_max, int32_t* frame_off, vv_stream stream);
int64_t vv_stream_smooth_partials(int32_t h, int32_t w);
int vv_stream_smooth(const double* ring, int32_t K, int32_t h, int32_t w, const int32_t* win, int32_t kt, int32_t ks, double* Bsum,
                     uint16_t* bcnt, double* out, double* partial, vv_stream stream);

/* ---- a streamed frame's per-pixel error mask (StreamScorer with maps): where inside its boxes a frame is anomalous.  What
 * vv_error_zmaps followed by vv_paint_zmaps compute on the batch route, fused, for boxes whose number lives on the device.
 * vv_stream_zpaint: ONE block's share of ONE round of one frame, enqueued behind that block's vv_stream_scores over the same tables.
 *   e_raw / e_of float32 [cap][32][32] = the per-pixel errors of the round's scoring launch (vv_error_maps; e_of == NULL drops the flow
 *   term; both may be NULL with stats NULL); stats double [4] or NULL, w_raw, w_of, big as for vv_stream_scores; keep and mask uint8
 *   [cap] = the round's keep flags and the block's mask row; n int32 [1] on the device, clamped to [0, cap].  Slot b counts iff b < n,
 *   keep[b] and mask[b] (the rule of vv_stream_scores).  Its rectangle is row slot0 + b of the FRAME's table (slot0 = round * cap):
 *   rects int32 [..][4] = (y0, y1, x0, x1) for rows below n_host -- resolved by the host as for vv_paint_masks, inside the h x w mask --
 *   and else Python's slicing of boxes int32 [..][4] = (x1, y1, x2, y2) exactly as vv_stream_paint resolves it; boxes == NULL: every
 *   rectangle is the host's.  rects is only read.  Pixel (y, x) inside the rectangle of a counted slot b is max-combined with
 *     z = the score of vv_cube_scores' expression (the same device function) on 1024 * e_raw[b][q] (and 1024 * e_of[b][q]),
 *     q = py * 32 + px, py = ((2 (y - y0) + 1) * 32) / (2 (y1 - y0)), px likewise (the source pixel of vv_paint_zmaps),
 *   or with +big when stats is NULL -- the value vv_error_zmaps + vv_paint_zmaps give that pixel, bit for bit.
 *   first != 0: out double [h][w] is written whole, -big where no counted rectangle reaches (no fill launch, out is not read);
 *   first == 0: the launch max-accumulates into what out holds, so a frame is the maximum over its rounds and blocks in any order.
 *   cap = 0 or n = 0 with first set leaves a mask of -big.  The errors of a slot that does not count are never read: NaN or Inf in the
 *   padded slots of the scoring launch, in dropped boxes and in boxes of other blocks cannot reach the mask.  An empty rectangle paints
 *   nothing.  Tables are staged through LDS VV_STREAM_PAINT_STAGE slots at a time; a thread owns two consecutive pixels (one 16-byte
 *   store where aligned); no atomics.  VV_ERR_BAD_ARG without a launch: NULL out / n / rects, NULL keep / mask with cap > 0, e_raw
 *   NULL with stats, cap < 0, slot0 < 0, n_host < 0, h <= 0 or w <= 0, h * w > (2^31 - 1) / 64 - 512. */
int vv_stream_zpaint(const float* e_raw, const float* e_of, const double* stats, double w_raw, double w_of, double big,
                     const uint8_t* keep, const uint8_t* mask, const int32_t* n, int32_t cap, int32_t slot0, const int32_t* rects,
                     int32_t n_host, const int32_t* boxes, int32_t h, int32_t w, double* out, int32_t first, vv_stream stream);

/* ---- a streamed frame's boxes linked into tracks (StreamScorer with tracks): one launch behind the frame's last vv_stream_scores,
 * over the tables vv_stream_paint reads.  All geometry is in integers and every sum is taken in one stated order, so the result is
 * exact.  The state belongs to the caller (one camera): t_meta int32 [max_tracks][8] = (id, age, hits, y0, y1, x0, x1, 0), t_hist
 * double [max_tracks][window] and next_id int32 [1] (started at 1 by the caller; it never goes back).  A live slot has id > 0, age =
 * the issued frames since its last match, hits = its matched frames, its last matched rectangle and, at position (k - 1) % window of
 * its row of t_hist, the score of its k-th match; a free slot is all zeros, history included.
 * vv_stream_tracks, in this order:
 *   0. reset != 0 (the first frame of a video): every slot is freed, whatever it holds.
 *   1. n int32 [1] on the device, clamped to [0, width].  Box b < n has the score s_b = max(-big, scores[0][b], ..,
 *      scores[rows-1][b]) (vv_stream_paint's box_max) and vv_stream_paint's rectangle: rects[b] = (y0, y1, x0, x1) for b < n_host, else
 *      Python's slicing of boxes[b] = (x1, y1, x2, y2) in an h x w mask; boxes == NULL: every rectangle is the host's.  rects is only
 *      read here, and a host rectangle is clipped to the mask.  Box b is a detection iff its rectangle is not empty and s_b > -big.
 *   2. every live track: age += 1.
 *   3. track t and detection d are a candidate pair iff inter > 0 and 100 * inter >= iou_pct * (area_t + area_d - inter), in int64.
 *      Pairs are ordered by IoU descending (inter_a * union_b against inter_b * union_a in int64), then lower slot, then lower box;
 *      the matching is the greedy one under that order, computed as iterated mutual-best choice (at most min(live tracks, detections)
 *      rounds, each of which ends by construction).  A matched track takes the detection's rectangle, age = 0, hits += 1 and s_d at
 *      position (hits - 1) % window of its history.
 *   4. an unmatched track with age > max_age is freed.
 *   5. unmatched detections in ascending box index take the free slots in ascending slot order: id = next_id++, age 0, hits 1, their
 *      rectangle and score.  A detection that finds no free slot has no track and is counted in dropped.
 *   6. for b < n: box_track[b] = (id, hits) of the box's track, (0, 0) for a box that is no detection or was dropped;
 *      box_track_score[b] = the mean of the track's last min(hits, window) scores, summed from +0.0 from the oldest to the newest and
 *      divided once, -big for id 0.  frame_track_score[0] = the largest box_track_score[b] over the boxes whose track has hits >=
 *      min_hits, -big if there is none.  counts int32 [3] = (live slots, dropped, next_id).
 *   Slots >= n of scores, rects and boxes are never read and those of box_track and box_track_score never written.  One workgroup;
 *   rectangles and scores are staged through LDS VV_STREAM_TRACK_STAGE at a time, so any n <= width goes; ordinary stores only, nothing
 *   waits for another workgroup.  VV_ERR_BAD_ARG without a launch: max_tracks outside 1..VV_STREAM_MAX_TRACKS, window outside
 *   1..VV_STREAM_TRACK_WINDOW, iou_pct outside 1..100, max_age < 0, min_hits < 1, negative sizes, h * w > INT32_MAX, NULL t_meta /
 *   t_hist / next_id / n / frame_track_score / counts, NULL rects / box_track / box_track_score with width > 0, NULL scores with rows
 *   and width > 0.  NaN scores are outside the domain. */
#define VV_STREAM_TRACK_STAGE 256
#define VV_STREAM_MAX_TRACKS 1024
#define VV_STREAM_TRACK_WINDOW 32
int vv_stream_tracks(int32_t* t_meta, double* t_hist, int32_t* next_id, int32_t max_tracks, const double* scores, int32_t rows,
                     int32_t width, const int32_t* n, int32_t n_host, const int32_t* rects, const int32_t* boxes, int32_t h, int32_t w,
                     int32_t reset, int32_t iou_pct, int32_t max_age, int32_t window, int32_t min_hits, double big, int32_t* box_track,
                     double* box_track_score, double* frame_track_score, int32_t* counts, vv_stream stream);

/* ---- motion-based foreground boxes (fore_det/obj_det_with_motion.py:144-223 get_mt_bboxes), integer arithmetic throughout ----
 * vv_motion_mask: one launch for N windows of three frames.
 *   frames uint8 [F][H][W][C], C = 1 | 3, 4-byte aligned; win int32 [N][3] = frame indices of each window (a 'hard' border repeats
 *   frames; indices are clamped to [0, F)); ksize 3 | 5 = cv2.GaussianBlur(sigma 0): [1,2,1]/4 or [1,4,6,4,1]/16, separable,
 *   BORDER_REFLECT_101, rounded half up once after both passes (H, W > ksize/2); per channel d = (|b0-b1| + |b1-b2|) mod 256,
 *   set iff d > binary_thr; ap int32 [M][5] = window, x1, y1, x2, y2 (x2, y2 >= 0): every pixel of
 *   [max(0,y1-extend), min(y2+extend,H)] x [max(0,x1-extend), min(x2+extend,W)] (inclusive) of that window is cleared;
 *   mask uint8 [N][H][W] = 255 where any channel is set, else 0.  The blurred planes live in LDS only.
 * vv_mask_boxes: cv2.findContours(RETR_EXTERNAL) + boundingRect + the reference's filter on mask uint8 [N][H][W] (non-zero =
 *   foreground).  8-connected foreground components that touch the frame edge or are 4-adjacent to the 4-connected background
 *   region reaching the frame edge; x, y, w, h = bounding rectangle; kept iff (w+1)*(h+1) > area_thr, w < 10 h and h < 10 w;
 *   boxes int32 [N][cap][4] = max(0,x-extend), max(0,y-extend), min(x+w+extend,W), min(y+h+extend,H), in DESCENDING order of the
 *   component's smallest linear pixel index; count int32 [N] = boxes found, which may exceed cap (the excess is not written).
 *   workspace: vv_mask_boxes_workspace_bytes(N, H, W) bytes, 16-byte aligned (20 bytes per pixel).  Bit-identical run to run. */
int vv_motion_mask(const uint8_t* frames, int32_t F, int32_t H, int32_t W, int32_t C, const int32_t* win, int32_t N,
                   int32_t ksize, int32_t binary_thr, const int32_t* ap, int32_t M, int32_t extend, uint8_t* mask,
                   vv_stream stream);
int64_t vv_mask_boxes_workspace_bytes(int32_t N, int32_t H, int32_t W);
int vv_mask_boxes(const uint8_t* mask, int32_t N, int32_t H, int32_t W, int32_t area_thr, int32_t extend, int32_t cap,
                  void* workspace, int64_t workspace_bytes, int32_t* count, int32_t* boxes, vv_stream stream);

/* ---- score aggregation (test.py:330-358,387-399, utils.py:29-41) ----
 * vv_frame_scores: frame_scores[f] = max(frame_scores[f], max over cubes m in [frame_off[f], frame_off[f+1]) with
 *   paints[m] != 0 of  cube_stat[m] < 0 ? big : w_raw*(raw[m]-mu_r)/sd_r + w_of*(of[m]-mu_o)/sd_o ), float64;
 *   stats = double [S][4] (mu_r, sd_r, mu_o, sd_o) indexed by cube_stat[m]; of == NULL drops the flow term (useFlow=False).
 *   The caller initialises frame_scores to -big (the mask background).
 * vv_roc_auc_counts: out3[0] = 2*#{pos>neg} + #{pos==neg}, out3[1] = #pos, out3[2] = #neg; AUC = out3[0]/(2*P*N).     */
int vv_frame_scores(const float* raw, const float* of, const int32_t* frame_off, const int32_t* cube_stat,
                    const double* stats, const uint8_t* paints, double w_raw, double w_of, double big, int32_t n_frames,
                    double* frame_scores, vv_stream stream);
int vv_roc_auc_counts(const double* scores, const uint8_t* labels, int32_t n, uint64_t* out3, vv_stream stream);

/* ---- pixel-level evaluation (the criterion the reference's score_mask files exist for and test.py:362-365 never evaluates) ----
 * NaN cube scores (a zero training std with an error equal to the mean) are outside the domain of all of these, as they are for
 * vv_frame_scores: fmax drops them where numpy's maximum propagates them.
 * vv_cube_scores: out[m] = the z-normalised, weighted score of cube m exactly as vv_frame_scores forms it (one shared device
 *   function): cube_stat[m] < 0 ? big : w_raw*((double)raw[m]-mu_r)/sd_r [+ w_of*((double)of[m]-mu_o)/sd_o], products and sums
 *   rounded separately; of == NULL drops the flow term.  double [n].
 * vv_paint_masks: out[f][y][x] = max(out[f][y][x], scores[m]) for every cube m in [frame_off[f], frame_off[f+1]) whose rectangle
 *   rects[m] = (y0, y1, x0, x1) holds y0 <= y < y1 and x0 <= x < x1.  rects int32 [n][4], 16-byte aligned, already resolved by
 *   the host (ceil, Python slice wrapping and clipping: vec_vad_amd/scoring.py box_rects); the kernel rounds and wraps nothing.
 *   out double [n_frames][h][w], 16-byte aligned, initialised by the caller (to -big, the mask background); a frame whose cubes
 *   come from several block groups is painted by one call per group.  No atomics: a thread owns two consecutive pixels of the
 *   flat h*w frame and walks the frame's boxes; a frame without boxes is not touched.  h * w < 2^31 - 512.
 * vv_pixel_scores: per frame f, with G = the pixels where gt != 0 (gt uint8 [n_frames][h][w]) and P the mask vv_paint_masks
 *   would paint over a background of -big (it is never formed): gt_count[f] = |G|; out[f] = the k-th largest value of P over G,
 *   k = (|G| * pct + 99) / 100 in integers, when |G| > 0, else the maximum of P (= the frame score).  1 <= pct <= 100.  ALL
 *   cubes of a frame must be in the one call (a quantile is not max-decomposable).  One workgroup per frame, integer LDS
 *   histogram: bit-identical run to run.  max_boxes = the largest frame_off[f+1] - frame_off[f], which the caller knows from its
 *   host copy of the table (the entry point cannot read device memory); above 2048 (the LDS table) the call returns
 *   VV_ERR_UNSUPPORTED and launches nothing.  Against a table that breaks max_boxes the kernel only protects memory. */
int vv_cube_scores(const float* raw, const float* of, const int32_t* cube_stat, const double* stats, double w_raw, double w_of,
                   double big, int32_t n, double* out, vv_stream stream);
int vv_paint_masks(const double* scores, const int32_t* frame_off, const int32_t* rects, int32_t n_frames, int32_t h, int32_t w,
                   double* out, vv_stream stream);
int vv_pixel_scores(const uint8_t* gt, const double* scores, const int32_t* frame_off, const int32_t* rects, int32_t pct,
                    double big, int32_t n_frames, int32_t h, int32_t w, int32_t max_boxes, double* out, int32_t* gt_count,
                    vv_stream stream);

/* ---- per-pixel anomaly maps (where inside a box the anomaly lies: the per-pixel squared error the cube score is the sum of) ----
 * vv_error_maps: e_raw[b][p] = sum over the UNets g with tgt_src[g] == 0, in ascending g, of sum over c < oc[g], in ascending c, of
 *   (out4[g][b*HW+p][c] - tgt0[(b*HW+p)*tgt0_cstride + tgt_coff[g] + c])^2 in fp32; e_of the same over tgt_src[g] == 1 and tgt1.
 *   out4 [G][B*HW][4], 16-byte aligned, is the reconstruction vv_outconv_fwd stores when vv_outconv_params.out4 != NULL; oc, tgt_src,
 *   tgt_coff, tgt0 / tgt1 and their channel strides are the fields of vv_outconv_params of the same names.  e_raw, e_of: float
 *   [B][HW]; e_of == NULL (tgt1 may then be NULL too) skips the flow UNets.  The sum of e_raw[b] over p is the raw score of cube b
 *   up to the order of the fp32 sum.  One thread per pixel, one streaming pass, no atomics: bit-identical run to run.
 * vv_error_zmaps: out[m][q] = the score vv_cube_scores forms (the same device function) with 1024 * e_raw[m][q] (1024 * e_of[m][q])
 *   in place of the cube's raw (flow) error, q < 1024 pixels of the 32x32 patch: cube_stat[m] < 0 ? big : w_raw*((double)(1024*e_raw)
 *   - mu_r)/sd_r [+ ...].  A cube whose error is spread evenly over its pixels gets the constant map out[m][q] = its cube score, to the
 *   bit.  e_raw, e_of (NULL drops the flow term): float [n][1024]; out double [n][1024] (8 KB per cube).
 * vv_paint_zmaps: vv_paint_masks with a value that varies inside the rectangle: out[f][y][x] = max(out[f][y][x], z[m][py*32+px]) for
 *   every cube m of frame f whose rectangle (y0, y1, x0, x1) holds (y, x), with py = ((2*(y-y0)+1)*32) / (2*(y1-y0)) and px likewise
 *   in integer arithmetic (nearest source pixel; 0..31; the identity for a rectangle 32 wide).  z double [n][1024]; everything else as
 *   for vv_paint_masks, any number of boxes per frame, no atomics.  h * w < 2^25 - 512.
 * vv_mask_kth: vv_pixel_scores on formed masks (double [n_frames][h][w]): gt_count[f] = |G|; out[f] = the k-th largest value of
 *   masks[f] over G, k = (|G| * pct + 99) / 100, when |G| > 0, else the maximum of masks[f] (-big for a frame of no pixels).  Exact:
 *   a radix select on the order-preserving integer image of the doubles with integer LDS histograms, one workgroup per frame;
 *   bit-identical run to run and independent of ties.  NaN mask values are outside the domain. */
int vv_error_maps(int32_t G, int32_t B, int32_t HW, const float* out4, const int32_t* oc, const int32_t* tgt_src,
                  const int32_t* tgt_coff, const float* tgt0, int32_t tgt0_cstride, const float* tgt1, int32_t tgt1_cstride,
                  float* e_raw, float* e_of, vv_stream stream);
int vv_error_zmaps(const float* e_raw, const float* e_of, const int32_t* cube_stat, const double* stats, double w_raw, double w_of,
                   double big, int32_t n, double* out, vv_stream stream);
int vv_paint_zmaps(const double* z, const int32_t* frame_off, const int32_t* rects, int32_t n_frames, int32_t h, int32_t w,
                   double* out, vv_stream stream);
int vv_mask_kth(const uint8_t* gt, const double* masks, int32_t pct, double big, int32_t n_frames, int32_t h, int32_t w,
                double* out, int32_t* gt_count, vv_stream stream);

/* ---- region- and track-based detection criteria (RBDC / TBDC): exact integer geometry; the curves are the host's ----
 * A region is an 8-connected component of the non-zero pixels of a frame's ground truth; the regions of a frame are numbered 1..R in
 * raster order of each component's first pixel, 0 is background.  The match and link tables hold VV_REGION_MAX regions per frame.
 * vv_label_regions: gt uint8 [n_frames][h][w] -> labels int32 [n_frames][h][w] (the numbering above) and n_regions[f] = R, the true
 *   count even above VV_REGION_MAX (labels are then still the raster ranks; the calls below ignore those above the cap).  Union-find on
 *   pixel indices with atomicMin (a parent never lies above its child, so every walk and every join ends by construction; no workgroup
 *   waits for another), then one workgroup per frame ranks the roots with a block scan.  The result is canonical: bit-identical run to
 *   run.  h * w <= 2^31 - 1 (VV_ERR_UNSUPPORTED within 1024 of it).
 * vv_region_match: a detection is a cube m of frame f (frame_off CSR [n_frames + 1] into scores double [n_boxes] and rects int32
 *   [n_boxes][4] rows (y0, y1, x0, x1), as for vv_paint_masks) whose rectangle is non-empty; it matches region r of its frame iff
 *   inter > 0 and 100 * inter >= iou_pct * (area_m + area_r - inter) in int64, inter = pixels of r inside the rectangle, area_m =
 *   (y1-y0)*(x1-x0).  region_area int32 [n_frames][64] (0 past R), region_score double [n_frames][64] = the largest score among the
 *   detections that match the region, -big if none does; box_state uint8 [n_boxes] = 0 empty rectangle, 1 matched a region, 2 false
 *   positive.  1 <= iou_pct <= 100.  One workgroup per frame, integer LDS histograms, any number of boxes per frame.
 * vv_region_links: links[f][r-1] gets bit q-1 when region r of frame f and region q of the frame before it share a pixel position;
 *   the frame before frame 0 is prev_labels int32 [h][w] (NULL: none).  same_video uint8 [n_frames]: a frame with 0 gets no links.
 *   links uint64 [n_frames][64] is written whole (zeros where nothing links).  LDS table per 2048 positions, 64-bit atomicOr.
 * Empty shapes (n_frames == 0; h * w == 0; n_boxes == 0) are VV_OK; NULL pointers with non-empty shapes, negative sizes, iou_pct
 * outside 1..100 and h * w > INT32_MAX are VV_ERR_BAD_ARG. */
#define VV_REGION_MAX 64
int vv_label_regions(const uint8_t* gt, int32_t* labels, int32_t* n_regions, int32_t n_frames, int32_t h, int32_t w,
                     vv_stream stream);
int vv_region_match(const int32_t* labels, const double* scores, const int32_t* frame_off, const int32_t* rects, int32_t iou_pct,
                    double big, int32_t n_frames, int32_t h, int32_t w, int32_t n_boxes, int32_t* region_area, double* region_score,
                    uint8_t* box_state, vv_stream stream);
int vv_region_links(const int32_t* prev_labels, const int32_t* labels, const uint8_t* same_video, int32_t n_frames, int32_t h,
                    int32_t w, uint64_t* links, vv_stream stream);

/* ---- spatio-temporal smoothing of score masks ([mi355x] smooth_masks): the 3-D mean filter the object-centric VAD protocol runs over
 * the painted map volume before it thresholds anything, restricted to the painted pixels ----
 * masks double [F][h][w]: a buffer of F consecutive frames (vv_paint_masks output), VV_SMOOTH_UNPAINTED (-100000.0) = "unpainted";
 * vid int32 [F]: the video of every frame of the buffer.  With p = (M != unpainted), V = p ? M : +0.0, N = p ? 1 : 0, rt = kt / 2,
 * rs = ks / 2, three separable passes, every sum taken in ascending offset order, left to right in float64, from +0.0 (counts are
 * integers):
 *   X:  A[f][y][x] = sum over dx = -rs..rs with 0 <= x+dx < w of V[f][y][x+dx];                          a = the same sum over N
 *   Y:  B[f][y][x] = sum over dy = -rs..rs with 0 <= y+dy < h of A[f][y+dy][x];                          b = the same sum over a
 *   T:  C[f][y][x] = sum over dt = -rt..rt with 0 <= f+dt < F and vid[f+dt] == vid[f] of B[f+dt][y][x];  c = the same sum over b
 *   S[f][y][x] = p[f][y][x] ? C / (double)c : unpainted      (one correctly rounded division, never a reciprocal multiply)
 * The order is part of the contract: the result equals the plain-numpy restatement (tests/smooth_restatement.py) bit for bit.  The
 * support is preserved, a frame without a box stays unpainted, kt = ks = 1 returns the masks.  A +big box (a block without a trained
 * model) raises the mean of every painted pixel whose window reaches it: it floods its neighbourhood, on purpose -- "certainly
 * anomalous" spreads like any other score.
 * out double [f1-f0][h][w] receives frames [f0, f1) of the buffer: the caller supplies the temporal halo (frames [f0-rt, f1+rt) cut to
 * the buffer are read; frames outside the buffer or of another video are left out of the T pass).  fmax double [f1-f0] (NULL: not
 * wanted) receives the maximum of every output frame, exact (unpainted for a frame without a painted pixel or of no pixels).  work:
 * vv_smooth_masks_work(F, h, w, kt, ks) bytes, 8-byte aligned (the X/Y sums as double and their counts as uint16 -- b <= 33^2, c <= 33^3
 * < 2^16 --, and one partial maximum per workgroup: no atomics, bit-identical run to run); -1 for sizes vv_smooth_masks refuses.
 * VV_ERR_BAD_ARG: NULL masks / vid / out / work with something to do, negative sizes, h * w >= 2^31, f0 < 0, f0 > f1, f1 > F, an even
 * window or one outside 1..VV_SMOOTH_MAX (at 33 a 32x32 tile with its halo of 16 still fits a workgroup's LDS: a stated condition, not
 * a measured optimum).  F == 0 or f0 == f1: nothing to do, VV_OK, no pointer is looked at.  NaN mask values are outside the domain. */
#define VV_SMOOTH_MAX 33
#define VV_SMOOTH_UNPAINTED (-100000.0)
int64_t vv_smooth_masks_work(int32_t F, int32_t h, int32_t w, int32_t kt, int32_t ks);
int vv_smooth_masks(const double* masks, const int32_t* vid, int32_t F, int32_t h, int32_t w, int32_t f0, int32_t f1, int32_t kt,
                    int32_t ks, double* out, double* fmax, void* work, vv_stream stream);

/* ---- macro AUROC and bootstrap intervals ([mi355x] auc_statistics): weighted Mann-Whitney counts per replicate and group ----
 * The weighted form of vv_roc_auc_counts.  For replicate r = r0 + k (k < R) and group g, out[k][g] = (U2, P, N) as int64 with
 *   P  = sum of w_i over the positive frames of the group, N = the same over its negative frames,
 *   U2 = sum over its positive frames i of w_i * (2 * Nbelow_i + Ntie_i), Nbelow_i / Ntie_i = the weighted number of negative frames of
 *        the group with a strictly smaller / an equal score;             the group's AUROC is U2 / (2 * P * N), undefined when P * N == 0.
 * All arithmetic is integer (LDS and global integer atomics, integer scans): bit-identical run to run and independent of the launch.
 * Tables, all device pointers, built once per score vector (vec_vad_amd/scoring.py auc_tables):
 *   order int32 [n]: frame indices, grouped by group and ascending by score inside a group (stable sort);
 *   tie int32 [n]: dense rank of the score inside its group, along order (equal scores of different groups never share a rank);
 *   label uint8 [n], in frame order (non-zero = positive); group_off int32 [G+1]: CSR offsets into order;
 *   video_off int32 [V+1]: the frames of video v are [video_off[v], video_off[v+1]) (test frames are contiguous per video);
 *   stratum_off int32 [S+1]: CSR offsets over the videos (VV_AUC_UNIT_VIDEO only).  Every group must be a union of whole videos.
 * The frame weights w_i of replicate r:
 *   VV_AUC_UNIT_NONE : w_i = 1, the full sample; R must be 1 (seed, the video tables and work are not looked at).
 *   VV_AUC_UNIT_VIDEO: cluster bootstrap.  In stratum s of V_s videos, draw j = 0..V_s-1 picks video stratum_off[s] + draw(seed, r, s, j,
 *     V_s); w_i = the number of times the video of frame i was picked.
 *   VV_AUC_UNIT_BLOCK: moving-block bootstrap inside every video (every video is kept).  For video v of L frames, b = min(block, L) and
 *     k = ceil(L / b); block j = 0..k-1 covers the b frames from draw(seed, r, 2^32 + v, j, L - b + 1) on; w_i = the number of blocks
 *     that cover frame i.  The weighted length of the video is k * b >= L: it is NOT trimmed to L.
 * draw is counter based and stateless, all arithmetic mod 2^64:
 *   mix(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; return x ^ x >> 31
 *   draw(seed, r, s, j, m) = ((mix(mix(mix(mix(seed) ^ r) ^ s) ^ j) >> 32) * m) >> 32,   in 0..m-1.
 * The multiply-shift is biased: a value's probability differs from 1 / m by less than 2^-32 (relative bias below m / 2^32).  This is
 * documented, not corrected.  The draws do not depend on the scores: two score vectors with the same seed get the same weights.
 * work: vv_auc_boot_work(n, V, R, unit) bytes, 8-byte aligned: the weights as uint32 [R][n] and, for VV_AUC_UNIT_VIDEO, the
 * multiplicities as uint32 [R][V]; 0 for VV_AUC_UNIT_NONE, -1 for sizes vv_auc_boot_counts refuses.  A caller bounds it by splitting the
 * replicates over calls (r0): replicates r0..r0+R-1 in one call equal the same replicates in several.
 * Capacity: a group and a video may hold any number of frames (tiles of 1024 / 4096); U2 fits int64 when max(V_s) * n < 2^31 (the
 * caller's check).  V > VV_AUC_BOOT_MAX_VIDEOS, R * G > INT32_MAX or R * V > INT32_MAX: VV_ERR_UNSUPPORTED, nothing is launched.
 * R == 0 or G == 0: VV_OK, nothing is looked at; n == 0: out is zeroed; an empty group gives (0, 0, 0).  VV_ERR_BAD_ARG: NULL order / tie
 * / label / group_off / out with n > 0, NULL video_off / work (or stratum_off for VV_AUC_UNIT_VIDEO) with a unit that resamples, negative
 * sizes, r0 < 1, block < 1, an unknown unit, VV_AUC_UNIT_NONE with R > 1.  Against tables that are no CSRs the kernels only protect
 * memory. */
#define VV_AUC_UNIT_NONE 0
#define VV_AUC_UNIT_VIDEO 1
#define VV_AUC_UNIT_BLOCK 2
#define VV_AUC_BOOT_MAX_VIDEOS 65536
int64_t vv_auc_boot_work(int32_t n, int32_t V, int32_t R, int32_t unit);
int vv_auc_boot_counts(const int32_t* order, const int32_t* tie, const uint8_t* label, const int32_t* group_off,
                       const int32_t* video_off, const int32_t* stratum_off, int32_t n, int32_t G, int32_t V, int32_t S, uint64_t seed,
                       int64_t r0, int32_t R, int32_t unit, int32_t block, int64_t* out, void* work, vv_stream stream);

/* ---- pictures ([mi355x] render): flow fields in the Middlebury colour coding, and frames with the score mask, the scored boxes and
 * the ground-truth contour drawn over them.  Both outputs are uint8 [n][h][w][3] in RGB order ----
 * vv_flow_color: flow float [n][h][w][2] (u, v), 8-byte aligned -> out.  Per image, in float32:
 *   a pixel with |u| > 1e7 or |v| > 1e7 is "unknown": it counts as (0, 0) for the maximum and is painted (0, 0, 0).  A pixel with a NaN
 *   component is treated the same way -- a stated deviation: in the original flow_to_image one NaN turns the whole image black;
 *   R = maxrad when maxrad > 0 (one fixed radius for every image, so that a video does not flicker; the original has no such mode), else
 *     R = max(-1, max over the image of sqrt(u*u + v*v)), product and sum rounded separately (no fused multiply-add), one reduction per
 *     image through one partial maximum per 4096 pixels in `work`: exact, bit-identical run to run, and an image never sees another's;
 *   u, v /= (R + 2^-52); rad = sqrt(u*u + v*v); a = atan2(-v, -u) / pi; fk = (a + 1) / 2 * 54 + 1; k0 = floor(fk); k1 = k0 + 1 (56 -> 1);
 *   f = fk - k0; per channel col = (1 - f) * wheel[k0-1] / 255 + f * wheel[k1-1] / 255; rad <= 1 ? col = 1 - rad * (1 - col) : col *= 0.75;
 *   the byte is floor(255 * col).  wheel: the 55 x 3 Middlebury table (RY 15, YG 6, GC 4, CB 11, BM 13, MR 6), in constant memory.
 *   The sign of a zero counts: v = +0.0 and v = -0.0 with u > 0 land on opposite ends of the wheel (atan2(-/+0, -u) = -/+pi), as in the
 *   original.  Against the float64 original a byte differs by at most 1, except where rad lies within rounding of 1 (the branch above).
 *   work: vv_flow_color_work(n, h, w) bytes, 4-byte aligned; not looked at (NULL allowed) when maxrad > 0; -1 for sizes vv_flow_color
 *   refuses.  VV_ERR_BAD_ARG: negative sizes, h * w > 2^31 - 4097, a NaN maxrad, NULL flow / out (/ work in per-image mode) with something
 *   to do, a misaligned flow or work.  n == 0 or h * w == 0: VV_OK, no pointer is looked at.
 * vv_render_overlay: frames uint8 [n][h][w][c], c = 1 (grey, replicated) or 3 (bgr != 0: stored B, G, R, the project's order; else R, G,
 *   B); mask double [n][h][w] (vv_paint_masks / vv_smooth_masks output), VV_RENDER_UNPAINTED = unpainted; gt uint8 [n][h][w] or NULL;
 *   rects int32 [n_boxes][4] rows (y0, y1, x0, x1), 16-byte aligned and resolved by the host as for vv_paint_masks, scores double
 *   [n_boxes], frame_off int32 [n + 1] CSR offsets of every frame's boxes (n_boxes == 0: none of the three is looked at, NULL allowed);
 *   lut uint8 [256][3] RGB.  With q(v) = 0 for v <= lo, 255 for v >= hi, else (int)floor((v - lo) / (hi - lo) * 255.0) in double, every
 *   operation rounded once (a +100000 box comes out as 255), later rules win, per pixel:
 *     1. the frame's RGB;
 *     2. mask != unpainted: every channel becomes (base * (256 - alpha) + lut[q(mask)] * alpha + 128) >> 8;
 *     3. the pixel lies on the outline of a non-empty rectangle of its frame -- inside it and on row y0 or y1 - 1 or column x0 or x1 - 1
 *        --: lut[q(s)], opaque, s = the largest score among those rectangles;
 *     4. gt given, gt != 0 here and a 4-neighbour is zero or outside the frame: white.
 *   Integer arithmetic and single IEEE double operations: the result is exact (tests/render_restatement.py, bit for bit).  Any number
 *   of boxes per frame, staged through LDS 256 at a time; no atomics; no work buffer.  NaN mask values and scores are outside the
 *   domain.  VV_ERR_BAD_ARG: negative sizes, h * w > 2^31 - 1025, c outside {1, 3}, alpha outside 0..256, hi <= lo (or a NaN), NULL
 *   frames / mask / lut / out with something to do, NULL rects / scores / frame_off with n_boxes > 0, misaligned rects; nothing is
 *   written.  n == 0 or h * w == 0: VV_OK. */
#define VV_RENDER_UNPAINTED (-100000.0)
int64_t vv_flow_color_work(int32_t n, int32_t h, int32_t w);
int vv_flow_color(const float* flow, int32_t n, int32_t h, int32_t w, float maxrad, uint8_t* out, void* work, vv_stream stream);
int vv_render_overlay(const uint8_t* frames, int32_t c, int32_t bgr, const double* mask, const uint8_t* gt, const int32_t* rects,
                      const double* scores, const int32_t* frame_off, int32_t n_boxes, const uint8_t* lut, double lo, double hi,
                      int32_t alpha, int32_t n, int32_t h, int32_t w, uint8_t* out, vv_stream stream);

/* library self-description */
const char* vv_version(void);
/* text for a value returned by any entry point (a pure function of its argument: pointer to a static string; for
 * VV_ERR_LAUNCH the HIP runtime's own text for the hipError_t carried in bits 8..); never printed by the library */
const char* vv_status_string(int status);
int vv_device_arch_ok(void); /* 1 when the current device is gfx950 */
/* compute units of the current device (256 on an MI355X in SPX mode; 256 when there is no device to ask): what the persistent kernels
 * size their grids with and what a host-side launch policy (k-splits, kernel routing) should use instead of a constant */
int vv_num_cus(void);
/* sizeof of a parameter struct as THIS library was compiled (which: 0 vv_view, 1 vv_conv_params, 2 vv_wgrad_params, 3 vv_pack_entry,
 * 4 vv_reduce_entry, 5 vv_fold_entry, 6 vv_bnbwd_params, 7 vv_outconv_params, 8 vv_conv2d_params; anything else: -1).  A binding
 * (cgo / ctypes) checks its own mirror of the struct against it once at load: vv_conv_params grew at its end in round 4. */
int vv_abi_sizeof(int32_t which);

/* ---- FlowNet2 fp16 mode (FlowNet2(fp16=True); FlowNet2_src/main.py:123-125 "fp16 storage fp32 math") ----
 * The exception to "all tensors are fp32": activations and weight panels below are IEEE fp16 (uint16_t bit patterns), NHWC with
 * channel strides in halves that are multiples of 8 (16 B).  Arithmetic is fp32; a result is rounded to fp16 where the module graph
 * after .half() materialises a tensor: a conv / deconv output is (acc + bias) rounded, LeakyReLU'd and rounded again; bias and the
 * fp32 weights of the two-channel heads hold fp16-rounded values.
 *  vv_conv2d_f16        : vv_conv2d_mfma's layer forms (kinds 0 / 1 / 2, ksplit) on v_mfma_f32_32x32x16_f16 (16x16x32 for Cout <= 16).
 *                         `p` is the vv_conv2d_params of vv_conv2d_mfma with src.ptr / out.ptr pointing at fp16 data (cstride / coff in
 *                         halves, src cstride % 8 == 0), w = a vv_pack_conv2d_f16 panel; CinP % 32 == 0 (kind 2: the flattened (kx, c)
 *                         run of an 8-half pixel, CinP = 64 for 7x7 s2 or 32 for 3x3 s1).  With ksplit > 1, out is an fp32 workspace
 *                         [ksplit][B*OH*OW][CoutP] finished by vv_conv2d_splitk_finish_f16.
 *  vv_pack_conv2d_f16   : fp32 Conv2d [N][K][taps] / ConvTranspose2d [K][N][taps] weight -> fp16 panel [taps][KP/8][NP][8] (KP % 16,
 *                         NP % 32 == 0; zero padding).
 *  vv_conv3x3_n2_f16 / vv_deconv4x4_c2_f16 / vv_correlation_nhwc_f16 / vv_flownet_prep_f16 / vv_warp_pack12_f16 /
 *  vv_fusion_pack11_f16 : the fp32 entry points above on fp16 maps (images and flows of 8-half pixels, packed outputs of 16).
 *                         vv_conv3x3_n2_f16 refuses a src_cstride that is no multiple of 8 halves (VV_ERR_BAD_ARG).  Pad channels
 *                         [Cin, ceil8(Cin)) of a conv source must be finite (they meet zero weights), not zero.
 *  vv_out8_to_nchw_f16  : vv_out4_to_nchw from an 8-half pixel map to NCHW fp16 (dst_f16 = 1) or fp32 (dst_f16 = 0). */
int vv_conv2d_f16(const vv_conv2d_params* p, vv_stream stream);
int vv_pack_conv2d_f16(const float* w, uint16_t* packed, int32_t taps, int32_t K, int32_t KP, int32_t N, int32_t NP,
                       int32_t transposed, vv_stream stream);
int vv_conv2d_splitk_finish_f16(const float* ws, int32_t ksplit, int64_t M, int32_t Cout, int32_t CoutP, const float* bias,
                                float slope, uint16_t* out, int32_t out_cstride, int32_t out_coff, vv_stream stream);
int vv_conv3x3_n2_f16(const uint16_t* src, int32_t src_cstride, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* wq,
                      int32_t C4P, const float* bias, float slope, uint16_t* out, int32_t out_cstride, int32_t out_coff,
                      vv_stream stream);
int vv_deconv4x4_c2_f16(const uint16_t* src, int32_t src_cstride, int32_t B, int32_t H, int32_t W, const float* w, const float* bias,
                        float slope, uint16_t* out, int32_t out_cstride, int32_t out_coff, vv_stream stream);
int vv_correlation_nhwc_f16(const uint16_t* f1, const uint16_t* f2, int32_t cstride, int32_t B, int32_t C, int32_t H, int32_t W,
                            uint16_t* out, int32_t out_cstride, int32_t out_coff, float slope, vv_stream stream);
int vv_flownet_prep_f16(const float* inputs, int32_t B, int32_t H, int32_t W, float rgb_max, void* workspace,
                        int64_t workspace_bytes, uint16_t* x6, uint16_t* img0, uint16_t* img1, vv_stream stream);
int vv_warp_pack12_f16(const uint16_t* x6, const uint16_t* img1, const uint16_t* flow2, int32_t flow_cstride, int32_t B, int32_t H,
                       int32_t W, int32_t mode, float scale, float div_flow, uint16_t* out16, vv_stream stream);
int vv_fusion_pack11_f16(const uint16_t* x6, const uint16_t* img1, const uint16_t* s2_flow2, int32_t s2_cstride,
                         const uint16_t* sd_flow2, int32_t sd_cstride, int32_t B, int32_t H, int32_t W, float div_flow,
                         uint16_t* out16, vv_stream stream);
int vv_out8_to_nchw_f16(int32_t B, int32_t HW, int32_t oc, const uint16_t* out8, void* dst, int32_t dst_f16, int32_t Ctot,
                        int32_t choff, vv_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VECVAD_HIP_H */
