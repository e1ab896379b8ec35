"""Restatements of the operations between FlowNet2's conv stacks (include/vecvad_hip.h: vv_correlation_fwd, vv_correlation_nhwc,
vv_resample2d_fwd, vv_channelnorm_fwd, vv_flownet_prep, vv_warp_pack12, vv_fusion_pack11 and the _f16 forms), written from the
operations' definitions and the layouts the header states -- not from the kernels.  Every function takes a ``dtype``: float64 is the
reference (everything is float64 then, the sampling coordinate x + dx included), float32 the reference arithmetic the kernels are
measured against (err_ref32).  tests/test_flow_ops_host.py checks them in float64 against oracle/flow_ops_oracle.py, a second
formulation of the correlation, torch.nn.functional.grid_sample / interpolate and torch.linalg.vector_norm on the CPU (no GPU needed).
"""
import torch

from flownet2_ops_restatement import act, upsample4, view_fill, view_read  # noqa: F401  (re-exported for the tests)

F32_SLOPE = float(torch.tensor(0.1, dtype=torch.float32))      # the C ABI passes slopes as float


# ---------------------------------------------------------------------------------------------- correlation
def correlation_out_shape(H, W, pad, k, md, s1, s2):
    """(D * D, oH, oW) by the reference's rule: the padded extent minus a border of kernel radius + max_displacement each side,
    divided by stride1 and rounded up"""
    br = (k - 1) // 2 + md
    D = 2 * (md // s2) + 1
    return D * D, -(-(H + 2 * pad - 2 * br) // s1), -(-(W + 2 * pad - 2 * br) // s1)


def correlation(a, b, pad, k, md, s1, s2, dtype):
    """a, b [B, C, H, W] -> [B, D * D, oH, oW]:
        out[n, (tj + dr) D + (ti + dr), y, x] = 1 / (k^2 C) sum_{j, i, c} A[n, c, y1 + j, x1 + i] B[n, c, y1 + tj s2 + j, x1 + ti s2 + i]
    A, B the maps zero-padded by ``pad`` on every side, y1 = y s1 + md + (k - 1) / 2 (x1 alike), dr = md // s2, D = 2 dr + 1, tj the
    row and ti the column displacement in [-dr, dr], j and i in [-(k - 1) / 2, (k - 1) / 2]."""
    B_, C, H, W = a.shape
    oC, oH, oW = correlation_out_shape(H, W, pad, k, md, s1, s2)
    kr, dr = (k - 1) // 2, md // s2
    D = 2 * dr + 1
    # padded far enough that every index below is in range whatever pad and md are (the extra ring is zeros, as the definition's)
    ext = max(0, md + kr - pad) + s1 + dr * s2
    A = torch.zeros(B_, H + 2 * (pad + ext), W + 2 * (pad + ext), C, dtype=dtype)
    Bp = torch.zeros_like(A)
    A[:, pad + ext:pad + ext + H, pad + ext:pad + ext + W] = a.to(dtype).permute(0, 2, 3, 1)
    Bp[:, pad + ext:pad + ext + H, pad + ext:pad + ext + W] = b.to(dtype).permute(0, 2, 3, 1)
    ys = torch.arange(oH) * s1 + md + kr + ext
    xs = torch.arange(oW) * s1 + md + kr + ext
    out = torch.zeros(B_, oC, oH, oW, dtype=dtype)
    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            acc = torch.zeros(B_, oH, oW, dtype=dtype)
            for j in range(-kr, kr + 1):
                for i in range(-kr, kr + 1):
                    pa = A[:, ys + j][:, :, xs + i]
                    pb = Bp[:, ys + tj * s2 + j][:, :, xs + ti * s2 + i]
                    acc = acc + torch.einsum('nyxc,nyxc->nyx', pa, pb)
            out[:, (tj + dr) * D + (ti + dr)] = acc / (k * k * C)
    return out


def correlation_nhwc(buf1, buf2, cstride, coff, B, C, H, W, slope, dtype):
    """FlowNetC's correlation (pad 20, kernel 1, max_displacement 20, stride1 1, stride2 2) of the NHWC slices (buf + coff, cstride):
    channels [coff, coff + C) of pixels cstride wide, then y = v > 0 ? v : slope v; [B, H, W, 441] with channel (tj + 10) 21 + (ti + 10)"""
    a = view_read(buf1, B * H * W, cstride, coff, C).reshape(B, H, W, C).permute(0, 3, 1, 2)
    b = view_read(buf2, B * H * W, cstride, coff, C).reshape(B, H, W, C).permute(0, 3, 1, 2)
    return act(correlation(a, b, 20, 1, 20, 1, 2, dtype), slope).permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------- fp16 roundings
def nbrs16(r16):
    """the fp16 values just above and just below each element of the fp16 tensor r16"""
    i = r16.contiguous().view(torch.int16).to(torch.int32)
    o = torch.where(i >= 0, i, -(i & 0x7fff))                     # sign-magnitude -> ordered
    back = lambda q: torch.where(q >= 0, q, (-q) | 0x8000).to(torch.int16).view(torch.float16)
    return back(o + 1), back(o - 1)


def act16(r16, slope):
    """LeakyReLU of a half tensor: the float product of the rounded value and the float slope, rounded"""
    return torch.where(r16 > 0, r16, (r16.float() * torch.tensor(float(slope), dtype=torch.float32)).half())


def ulp16(a):
    """fp16 ulp of |a| (float64 tensor); 2^-24 below the smallest normal number"""
    a = a.abs().clamp_min(2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 10)


def correlation_nhwc_f16(buf1, buf2, cstride, coff, B, C, H, W, slope):
    """the fp16 form: maps widened, the float64 value v (already divided by C) rounded to fp16, LeakyReLU on the rounded value, rounded.
    With w = 8 * 2^-24 * sum |a| |b| / C, returns (ref, lo, hi, excused, share): ref, lo, hi = that definition applied to v, v - w and
    v + w; ``excused`` where v lies within w of a rounding boundary of fp16 (the midpoint between round(v) and either neighbour), which
    is where lo, ref and hi are not all one value; ``share`` = their fraction of all elements."""
    v = correlation_nhwc(buf1, buf2, cstride, coff, B, C, H, W, 1.0, torch.float64)
    w = 8 * 2.0 ** -24 * correlation_nhwc(buf1.abs(), buf2.abs(), cstride, coff, B, C, H, W, 1.0, torch.float64)
    r = v.half()
    up, dn = nbrs16(r)
    bu, bd = (r.double() + up.double()) / 2, (r.double() + dn.double()) / 2
    excused = torch.minimum((v - bu).abs(), (v - bd).abs()) <= w
    return act16(r, slope), act16((v - w).half(), slope), act16((v + w).half(), slope), excused, float(excused.double().mean())


def check_f16_correlation(got, ref, lo, hi, excused):
    """the fp16 correlation bar.  An element that is not excused equals ``ref`` bit for bit (+0 and -0 are one value: a float32 sum
    that cancels may reach zero from the other side).  An excused element is what the definition gives for some value within the
    allowance of the float64 one: lo <= got <= hi (rounding and LeakyReLU with slope >= 0 are monotone).  Where the allowance is below
    half an fp16 step that is one step at the first rounding; the second rounding can turn it into two ulp of a negative output (slope
    0.1: a step of r is 1.6 steps of 0.1 r when r's mantissa is below 1.28), and among subnormal outputs, whose step of 2^-24 is below
    the allowance itself, into several steps of r.  Returns (differing share, share more than one fp16 ulp of ref away)."""
    def bits(t):
        return torch.where(t == 0, torch.zeros_like(t), t).contiguous().view(torch.int16)
    same = bits(got) == bits(ref)
    g64 = got.double()
    ok = same | (excused & (lo.double() <= g64) & (g64 <= hi.double()))
    assert bool(torch.isfinite(got.float()).all())
    assert bool(ok.all()), ('elements outside the allowance', int((~ok).sum()), got[~ok][:6], ref[~ok][:6], lo[~ok][:6], hi[~ok][:6],
                            excused[~ok][:6])
    far = (g64 - ref.double()).abs() > ulp16(ref.double())
    return float((~same).double().mean()), float(far.double().mean())


# ---------------------------------------------------------------------------------------------- Resample2d, ChannelNorm
def resample2d(img, flow, dtype):
    """img [B, C, H, W], flow [B, 2, fH, fW] (dx, dy) -> [B, C, fH, fW]: the bilinear sample of img at (x + dx, y + dy); the weights
    come from the un-clamped coordinate, the four corner indices are clamped to the flow's extents [0, fW - 1] x [0, fH - 1]"""
    B, C, H, W = img.shape
    fH, fW = flow.shape[2:]
    img, flow = img.to(dtype), flow.to(dtype)
    xf = torch.arange(fW, dtype=dtype).view(1, 1, fW) + flow[:, 0]
    yf = torch.arange(fH, dtype=dtype).view(1, fH, 1) + flow[:, 1]
    fx, fy = xf.floor(), yf.floor()
    al, be = (xf - fx).unsqueeze(1), (yf - fy).unsqueeze(1)
    xL, xR = fx.clamp(0, fW - 1).long(), (fx + 1).clamp(0, fW - 1).long()
    yT, yB = fy.clamp(0, fH - 1).long(), (fy + 1).clamp(0, fH - 1).long()
    flat = img.reshape(B, C, H * W)
    at = lambda yy, xx: torch.gather(flat, 2, (yy * W + xx).reshape(B, 1, fH * fW).expand(B, C, fH * fW)).view(B, C, fH, fW)
    return (1 - al) * (1 - be) * at(yT, xL) + al * (1 - be) * at(yT, xR) + (1 - al) * be * at(yB, xL) + al * be * at(yB, xR)


def channelnorm(x, dtype):
    """x [B, C, H, W] -> [B, 1, H, W]: the L2 norm over the channels"""
    x = x.to(dtype)
    return (x * x).sum(1, keepdim=True).sqrt()


def flow_up4(flow2, mode, scale, dtype):
    """flow2 [B, h, w, 2] -> nn.Upsample(scale_factor=4) of its two channels times ``scale``, [B, 2, 4h, 4w]; the three modes of
    flow_up4's comment: 0 nearest, 1 bilinear with align_corners=False, 2 bilinear with align_corners=True"""
    B, h, w, _ = flow2.shape
    planes = flow2.to(dtype).permute(0, 3, 1, 2).reshape(B * 2, h, w)
    return upsample4(planes, mode, torch.tensor(float(scale), dtype=dtype)).view(B, 2, 4 * h, 4 * w)


# ---------------------------------------------------------------------------------------------- the glue kernels
def prep(inputs, rgb_max, dtype):
    """inputs [B, 3, 2, H, W] float32 -> (x6 [B, H, W, 8], img0 [B, H, W, 4], img1 [B, H, W, 4]): x = (inputs - mean) / rgb_max with the
    mean over (frame, H, W) per image and colour taken in float64; x6 = frame 0's colours, frame 1's colours, two zero channels;
    img0 / img1 = one frame's colours and a zero channel"""
    B, _, _, H, W = inputs.shape
    mean = inputs.double().mean(dim=(2, 3, 4), keepdim=True).to(dtype)
    x = (inputs.to(dtype) - mean) / torch.tensor(float(rgb_max), dtype=dtype)
    f0, f1 = x[:, :, 0].permute(0, 2, 3, 1), x[:, :, 1].permute(0, 2, 3, 1)
    z = torch.zeros(B, H, W, 1, dtype=dtype)
    return torch.cat((f0, f1, z, z), 3), torch.cat((f0, z), 3), torch.cat((f1, z), 3)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def warp_pack12(x6, img1, flow2, mode, scale, div_flow, dtype):
    """x6 [B, H, W, >= 6], img1 [B, H, W, >= 3], flow2 [B, H/4, W/4, 2] -> [B, H, W, 12] =
    cat(x6[0:6], Resample2d(img1, flow), flow / div_flow, ChannelNorm(x6[0:3] - warped)), flow = Upsample x4 (mode) of flow2 times scale"""
    fl = flow_up4(flow2, mode, scale, dtype)
    x = _nchw(x6[..., :6].to(dtype))
    warped = resample2d(_nchw(img1[..., :3]), fl, dtype)
    nrm = channelnorm(x[:, :3] - warped, dtype)
    return torch.cat((x, warped, fl / torch.tensor(float(div_flow), dtype=dtype), nrm), 1).permute(0, 2, 3, 1)


def fusion_pack11(x6, img1, s2_flow2, sd_flow2, div_flow, dtype):
    """-> [B, H, W, 12] = cat(x1, sd, s2, |sd|, |s2|, |x1 - warp(img1, sd)|, |x1 - warp(img1, s2)|, 0) with x1 = x6[0:3],
    s2 = nearest x4 of s2_flow2 times div_flow, sd = nearest x4 of sd_flow2 divided by div_flow"""
    div = torch.tensor(float(div_flow), dtype=dtype)
    s2 = flow_up4(s2_flow2, 0, div_flow, dtype)
    sd = flow_up4(sd_flow2, 0, 1.0, dtype) / div
    x1, im = _nchw(x6[..., :3].to(dtype)), _nchw(img1[..., :3])
    n_sd = channelnorm(x1 - resample2d(im, sd, dtype), dtype)
    n_s2 = channelnorm(x1 - resample2d(im, s2, dtype), dtype)
    z = torch.zeros_like(n_sd)
    return torch.cat((x1, sd, s2, channelnorm(sd, dtype), channelnorm(s2, dtype), n_sd, n_s2, z), 1).permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------- the half graph of the glue kernels
def half_warp_pack12(x, f2, mode, scale, div_flow, step=(0, 0)):
    """the half graph tests/test_flownet2_fp16.py uses (flownet2.py:76-86): x [B, 6, H, W] and f2 [B, 2, h, w] halves -> [B, 12, H, W];
    every materialised tensor is computed from widened inputs and rounded once.  ``step`` moves the up-sampled flow (dx, dy) by that
    many fp16 steps (-1, 0, 1) before it is used: what the tensors behind it become when the flow itself is one ulp off."""
    import torch.nn.functional as F
    import flownet2_fp16_restatement as HR
    kw = dict(mode='nearest') if mode == 0 else dict(mode='bilinear', align_corners=mode == 2)
    fl = F.interpolate((f2.float() * scale).half(), scale_factor=4, **kw)
    up, dn = nbrs16(fl)
    fl = torch.stack([(dn, fl, up)[step[c] + 1][:, c] for c in (0, 1)], 1)
    warped = torch.from_numpy(HR.resample2d_fwd(x[:, 3:].numpy(), fl.numpy()))
    nrm = torch.from_numpy(HR.channelnorm_fwd((x[:, :3] - warped).numpy()))
    return torch.cat([x, warped, (fl.float() / div_flow).half(), nrm], 1)


def half_fusion_pack11(x, s2f2, sdf2, div_flow):
    """the half graph of flownet2.py:105-136 -> [B, 11, H, W]"""
    import torch.nn.functional as F
    import flownet2_fp16_restatement as HR
    up = lambda t: F.interpolate(t, scale_factor=4, mode='nearest')
    s2 = up((s2f2.float() * div_flow).half())
    sd = up((sdf2.float() / div_flow).half())
    cn = lambda t: torch.from_numpy(HR.channelnorm_fwd(t.numpy()))
    rs = lambda f: torch.from_numpy(HR.resample2d_fwd(x[:, 3:].numpy(), f.numpy()))
    return torch.cat((x[:, :3], sd, s2, cn(sd), cn(s2), cn(x[:, :3] - rs(sd)), cn(x[:, :3] - rs(s2))), 1)


# ---------------------------------------------------------------------------------------------- cases shared by the host and GPU tests
def gen(*key):
    return torch.Generator(device='cpu').manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


# vv_correlation_fwd, kernel_size 1: (B, C, H, W, pad, md, s1, s2)
K1_CASES = [(1, 80, 9, 33, 20, 20, 1, 2), (2, 5, 12, 70, 4, 4, 2, 1), (1, 24, 8, 40, 3, 5, 1, 2), (1, 16, 7, 20, 8, 4, 1, 2),
            (1, 8, 6, 34, 22, 22, 1, 2), (1, 384, 3, 32, 20, 20, 1, 2)]
# kernel_size > 1: (B, C, H, W, pad, k, md, s1, s2); the first three are tests/test_flow_ops.py's
GENERIC_CASES = [(1, 16, 10, 14, 5, 3, 4, 1, 2), (2, 8, 9, 11, 4, 3, 2, 1, 1), (1, 5, 12, 12, 8, 5, 4, 2, 2), (2, 7, 11, 13, 3, 3, 4, 2, 2)]
# vv_correlation_nhwc / _f16: (B, C, H, W, wide, out_coff, slope); wide: the maps are channels [q, q + C) of pixels C + q wide, q one
# 16-byte step (4 floats / 8 halves); the destination's pixel stride is out_coff + 446 (never 476 / 480)
NHWC_CASES = [(1, 16, 1, 64, False, 3, F32_SLOPE), (2, 48, 5, 128, True, 32, 1.0), (3, 32, 44, 64, False, 0, 0.0),
              (1, 32, 43, 128, True, 3, F32_SLOPE), (1, 256, 6, 128, False, 32, 1.0), (1, 256, 6, 64, True, 0, 0.0)]
NHWC_SLACK = 64


def nhwc_geometry(case, half):
    B, C, H, W, wide, ocoff, slope = case
    q = (8 if half else 4) if wide else 0
    return C + q, q, ocoff + 446, ocoff


def nhwc_maps(case, gi, half):
    """the two feature maps [B, H, W, C] of group gi, N(0, 0.7^2) (rounded to fp16 for the half form), and the case's generator, which
    the tests go on drawing filler from"""
    B, C, H, W = case[:4]
    g = gen(B, C, H, W, gi, int(half))
    a, b = torch.randn(B, H, W, C, generator=g) * 0.7, torch.randn(B, H, W, C, generator=g) * 0.7
    return (a.half(), b.half(), g) if half else (a, b, g)


def nhwc_buffer(x, cstride, coff, g):
    """x inside pixels cstride wide, pad channels and NHWC_SLACK elements behind the tensor drawn from g (finite)"""
    npix = x.numel() // x.shape[-1]
    buf = (torch.randn(npix * cstride + NHWC_SLACK, generator=g) * 0.7).to(x.dtype)
    return view_fill(buf, x, cstride, coff)
