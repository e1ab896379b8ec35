"""Restatements of the FlowNet2 fp32 conv stack's operations (include/vecvad_hip.h: vv_conv2d_mfma, vv_conv2d_splitk_finish,
vv_pack_conv2d, vv_conv3x3_n2, vv_deconv4x4_c2, vv_conv2d_wino, vv_upsample4), written from the operations' definitions and the
layouts the header states -- not from the kernels.  Every function works in the dtype of its inputs: float64 is the reference,
float32 the reference arithmetic the kernels are measured against.  tests/test_flownet2_ops_host.py checks them against
torch.nn.functional.conv2d / conv_transpose2d / interpolate in float64 on the CPU (no GPU needed).
"""
import torch


def ceil_to(c, q):
    return (c + q - 1) // q * q


# ---------------------------------------------------------------------------------------------- NHWC views
def view_read(buf, npix, cstride, coff, C):
    """channels [coff, coff + C) of the npix pixels of an NHWC view (ptr, cstride, coff) over the flat buffer ``buf``"""
    return buf[:npix * cstride].view(npix, cstride)[:, coff:coff + C]


def view_fill(buf, x, cstride, coff):
    """x [..., C] written into channels [coff, coff + C) of the view; everything else of ``buf`` stays"""
    C = x.shape[-1]
    npix = x.numel() // C
    buf[:npix * cstride].view(npix, cstride)[:, coff:coff + C] = x.reshape(npix, C)
    return buf


def act(v, slope):
    """y = v > 0 ? v : slope * v, slope rounded to the dtype of v (the C ABI passes a float)"""
    return torch.where(v > 0, v, v * torch.tensor(float(slope), dtype=v.dtype))


# ---------------------------------------------------------------------------------------------- conv / transposed conv
def conv_out_size(H, R, stride):
    pad = (R - 1) // 2
    return (H + 2 * pad - R) // stride + 1


def conv_nhwc(x, w, bias, stride, slope):
    """nn.Conv2d(k = R, stride, padding = (R - 1) // 2) on x [B, H, W, Cin] with w [Cout, Cin, R, R]:
    out[b, oy, ox, n] = bias[n] + sum_{ky, kx, c} x[b, oy * stride + ky - pad, ox * stride + kx - pad, c] * w[n, c, ky, kx]
    (zero outside the image), then the activation."""
    B, H, W, Cin = x.shape
    Cout, _, R, _ = w.shape
    pad = (R - 1) // 2
    OH, OW = conv_out_size(H, R, stride), conv_out_size(W, R, stride)
    xp = torch.zeros(B, H + 2 * pad, W + 2 * pad, Cin, dtype=x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = torch.zeros(B, OH, OW, Cout, dtype=x.dtype)
    for ky in range(R):
        for kx in range(R):
            xs = xp[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride]
            out += xs @ w[:, :, ky, kx].t()
    if bias is not None:
        out += bias
    return act(out, slope)


def deconv_nhwc(x, w, bias, slope):
    """nn.ConvTranspose2d(k4, s2, p1) on x [B, H, W, Cin] with w [Cin, Cout, 4, 4]:
    out[b, 2 iy - 1 + ky, 2 ix - 1 + kx, n] += x[b, iy, ix, c] * w[c, n, ky, kx] (positions outside 2H x 2W dropped)."""
    B, H, W, Cin = x.shape
    Cout = w.shape[1]
    full = torch.zeros(B, 2 * H + 2, 2 * W + 2, Cout, dtype=x.dtype)      # index = output position + 1
    for ky in range(4):
        for kx in range(4):
            full[:, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += x @ w[:, :, ky, kx]
    out = full[:, 1:1 + 2 * H, 1:1 + 2 * W].clone()
    if bias is not None:
        out += bias
    return act(out, slope)


# ---------------------------------------------------------------------------------------------- weight layouts
def pack_panel(w, KP, NP, transposed):
    """The packed panel of the header: [taps][KP / 8][2][NP][4], zero padded, k = kq * 8 + half * 4 + j.  w: Conv2d [N][K][R][R]
    (tap = ky * R + kx) or, transposed, ConvTranspose2d [K][N][4][4] (tap = ky * 4 + kx); any trailing tap shape, flattened."""
    if transposed:
        K, N = w.shape[0], w.shape[1]
        wt = w.reshape(K, N, -1).permute(2, 0, 1)                          # [tap][k][n]
    else:
        N, K = w.shape[0], w.shape[1]
        wt = w.reshape(N, K, -1).permute(2, 1, 0)
    taps = wt.shape[0]
    full = torch.zeros(taps, KP, NP, dtype=w.dtype)
    full[:, :K, :N] = wt
    # k = kq * 8 + half * 4 + j  ->  [tap][kq][half][j][n]  ->  [tap][kq][half][n][j]
    return full.view(taps, KP // 8, 2, 4, NP).permute(0, 1, 2, 4, 3).contiguous().reshape(-1)


def rowk_weight(w, cstride, KP):
    """The row-K rearrangement: Conv2d weight [N][Cin][ky][kx] -> [N][kx * cstride + c][ky], zeros at the pad channels and beyond
    kx = R - 1; packed with taps = R and K = KP it gives the kind-2 panel."""
    N, Cin, R, _ = w.shape
    out = torch.zeros(N, KP, R, dtype=w.dtype)
    for kx in range(R):
        for c in range(Cin):
            out[:, kx * cstride + c, :] = w[:, c, :, kx]
    return out


def n2_weight(w, C4P):
    """The two-channel head's layout: Conv2d weight [2][Cin][3][3] -> [tap 9][C4P][out 2][4], Cin zero padded to 4 * C4P"""
    Cin = w.shape[1]
    out = torch.zeros(9, C4P, 2, 4, dtype=w.dtype)
    for c in range(Cin):
        out[:, c // 4, :, c % 4] = w[:, c].reshape(2, 9).t()
    return out.reshape(-1)


# ---------------------------------------------------------------------------------------------- split-K finish
def splitk_finish_f32(ws, ksplit, M, Cout, CoutP, bias, slope):
    """float32, fixed order: bias, += slab 0, += slab 1 ..., then the activation.  ws: flat workspace [ksplit][M][CoutP]"""
    assert ws.dtype == torch.float32
    slabs = ws[:ksplit * M * CoutP].view(ksplit, M, CoutP)
    v = (bias.float() if bias is not None else torch.zeros(Cout)).expand(M, Cout).clone()
    for k in range(ksplit):
        v = v + slabs[k, :, :Cout]
    return act(v, slope)


# ---------------------------------------------------------------------------------------------- x4 up-sampling
def upsample4(x, mode, scale):
    """nn.Upsample(scale_factor=4) on planes x [BC, H, W] times ``scale``: mode 0 nearest (src = dst // 4), 1 bilinear with
    align_corners=False (src = max((dst + 0.5) / 4 - 0.5, 0)), 2 bilinear with align_corners=True (src = dst * (in - 1) / (out - 1),
    0 for a single input row / column)."""
    BC, H, W = x.shape
    OH, OW = 4 * H, 4 * W
    dt = x.dtype
    if mode == 0:
        return x[:, torch.arange(OH) // 4][:, :, torch.arange(OW) // 4] * scale

    def coords(n_in, n_out):
        o = torch.arange(n_out, dtype=dt)
        if mode == 2:
            s = o * ((n_in - 1) / (n_out - 1)) if n_in > 1 else torch.zeros(n_out, dtype=dt)
        else:
            s = torch.clamp((o + 0.5) / 4 - 0.5, min=0)
        i0 = torch.clamp(s.floor().long(), max=n_in - 1)
        i1 = torch.clamp(i0 + 1, max=n_in - 1)
        return i0, i1, s - i0.to(dt)

    y0, y1, ly = coords(H, OH)
    x0, x1, lx = coords(W, OW)
    ly, lx = ly.view(1, OH, 1), lx.view(1, 1, OW)
    top = x[:, y0][:, :, x0] * (1 - lx) + x[:, y0][:, :, x1] * lx
    bot = x[:, y1][:, :, x0] * (1 - lx) + x[:, y1][:, :, x1] * lx
    return (top * (1 - ly) + bot * ly) * scale
