"""Restatements of FlowNet2's fp16 conv stack (include/vecvad_hip.h, "FlowNet2 fp16 mode": vv_conv2d_f16, vv_pack_conv2d_f16,
vv_conv2d_splitk_finish_f16, vv_conv3x3_n2_f16, vv_deconv4x4_c2_f16, vv_out8_to_nchw_f16), written from the header and the header
comment of vv_conv2d_f16.hip -- "products of fp16 operands summed in fp32, the fp32 bias added in fp32, the sum rounded to fp16,
LeakyReLU applied to the rounded value and rounded again" -- not from the kernels' index arithmetic.  The convolutions themselves are
those of tests/flownet2_ops_restatement.py, evaluated in float64 on the exact fp16 operand values.
tests/test_flownet2_f16_ops_host.py checks everything here on the CPU.
"""
import torch

from flownet2_ops_restatement import (ceil_to, conv_nhwc, conv_out_size, deconv_nhwc, n2_weight, rowk_weight,  # noqa: F401
                                      view_fill, view_read)


def rn_f16(t):
    """(vv_h)(float): ONE rounding to float32, then nearest-even to fp16 (11 significant bits, subnormals kept, 65520 -> inf)"""
    return t.float().half()


def act_out_f16(pre64, slope):
    """vv_act_out<vv_h>: r = rn_f16(pre); r > 0 ? r : rn_f16(float32(r * slope)).  r has 11 significant bits and float32(slope) 24, so
    their product is exact in float64; .float() is then the kernel's one fp32 multiply rounding and .half() the second fp16 rounding."""
    r = rn_f16(pre64)
    s = torch.tensor(float(slope), dtype=torch.float32).double()
    return torch.where(r > 0, r, rn_f16(r.double() * s))


def pre64(de, x16, w16, bias, stride):
    """float64 conv2d / conv_transpose2d(k4, s2, p1) of the fp16 source and panel values plus float64(bias): the bias is the fp32
    number the ABI passes, added unrounded.  x16 [B, H, W, Cin]; w16 Conv2d [Cout, Cin, R, R] or ConvTranspose2d [Cin, Cout, 4, 4]."""
    assert x16.dtype == torch.float16 and w16.dtype == torch.float16 and (bias is None or bias.dtype == torch.float32)
    b = None if bias is None else bias.double()
    return deconv_nhwc(x16.double(), w16.double(), b, 1.0) if de else conv_nhwc(x16.double(), w16.double(), b, stride, 1.0)


def pack_panel_f16(w, KP, NP, transposed):
    """The fp16 panel of the header: [taps][KP / 8][NP][8], k = kq * 8 + j, zero padded, values rn_f16(w).  w: Conv2d [N][K][taps...]
    or, transposed, ConvTranspose2d [K][N][taps...] (tap = ky * R + kx), float32."""
    if transposed:
        K, N = w.shape[0], w.shape[1]
        wt = w.reshape(K, N, -1).permute(2, 0, 1)                          # [tap][k][n]
    else:
        N, K = w.shape[0], w.shape[1]
        wt = w.reshape(N, K, -1).permute(2, 1, 0)
    taps = wt.shape[0]
    full = torch.zeros(taps, KP, NP, dtype=w.dtype)
    full[:, :K, :N] = wt
    # k = kq * 8 + j  ->  [tap][kq][j][n]  ->  [tap][kq][n][j]
    return rn_f16(full.view(taps, KP // 8, 8, NP).permute(0, 1, 3, 2).contiguous().reshape(-1))


ROWK_KP = {(7, 2): 64, (3, 1): 32}      # kind 2: the flattened (kx, c) run of an 8-half pixel, padded


def rowk_weight_f16(w):
    """the row-K rearrangement for 8-half pixels: [N][Cin][ky][kx] -> [N][kx * 8 + c][ky], KP = 64 (7x7 s2) / 32 (3x3 s1)"""
    Rk = w.shape[-1]
    return rowk_weight(w, 8, ROWK_KP[(Rk, 2 if Rk == 7 else 1)])


def splitk_finish_f16(ws, ksplit, M, Cout, CoutP, bias, slope):
    """float32, fixed order: bias, += slab 0, += slab 1 ..., then act_out_f16.  ws: flat float32 workspace [ksplit][M][CoutP]"""
    assert ws.dtype == torch.float32
    slabs = ws[:ksplit * M * CoutP].view(ksplit, M, CoutP)
    v = (bias.float() if bias is not None else torch.zeros(Cout)).expand(M, Cout).clone()
    for k in range(ksplit):
        v = v + slabs[k, :, :Cout]
    return act_out_f16(v.double(), slope)


def out8_to_nchw(out8, B, HW, oc, dst, Ctot, choff):
    """channels [0, oc) of the 8-half pixel map out8 [B * HW][8] into planes [choff, choff + oc) of dst [B][Ctot][HW] (fp16 or fp32:
    widening is exact); every other plane stays"""
    dst = dst.clone()
    dst.view(B, Ctot, HW)[:, choff:choff + oc] = out8.view(B, HW, 8)[:, :, :oc].permute(0, 2, 1).to(dst.dtype)
    return dst


# ---------------------------------------------------------------------------------------------- dispatch
CK_F16 = {(1, 1): 32, (3, 1): 32, (3, 2): 16, (5, 2): 16, (7, 2): 16, 'deconv': 32}      # vv_conv2d_f16.hip:295-310 (the entry's launches)


def expected_form_f16(de, Rk, stride, W, Cout, CoutP, rowk):
    """The instantiation launch_f16 selects (vv_conv2d_f16.hip:253-281): narrow = LW <= 16 && !CP (line 258), wide = CoutP % 64 == 0 &&
    Cout > 32 (260), CAN16 = !CP && CK % 32 == 0 (262: (1,1), (3,1) and the deconv), the chain narrow -> wide -> N16 -> NR = 1 (266-278):
    narrow wins over N16."""
    LW = W if de else conv_out_size(W, Rk, stride)
    narrow = LW <= 16 and not rowk
    wide = CoutP % 64 == 0 and Cout > 32
    can16 = not rowk and (32 if rowk else CK_F16['deconv' if de else (Rk, stride)]) % 32 == 0
    if narrow:
        return 'tw16_nr2' if wide else 'tw16_nr1'
    if wide:
        return 'nr2'
    if can16 and Cout <= 16:
        return 'n16'
    return 'nr1'


def n2_form_f16(npix, Cin):
    """The form launch_n2<vv_h> selects (vv_conv2d.hip:794-841): the fp32 chain without its 8 x 32 branch (line 814 is `F32 &&`), so
    npix >= 100000 with Cin > 32 falls through to split<8> (820)."""
    if npix >= 20000 and Cin <= 32:
        return 'tile16' if Cin <= 16 else 'tile32'
    if npix >= 20000:
        return 'split8'
    if Cin >= 320:
        return 'tap16' if npix >= 4096 else ('tap32' if npix >= 1024 else 'tap64')
    return 'split32' if npix >= 4096 else 'split64'
