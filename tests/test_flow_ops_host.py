"""The restatements of tests/flow_ops_restatement.py in float64 against independent formulations on the CPU (no GPU): the numpy oracle
on the new geometries, a second formulation of the correlation (shifted slices of the un-padded maps and a sum over channels),
grid_sample where the two definitions of the warp agree, torch.linalg.vector_norm, F.interpolate in the three modes and plain torch
arithmetic for the prep.  It also asserts the conditions tests/test_gpu_flow_ops.py relies on: the warp is continuous across every
clamp (so no input needs nudging), and on the GPU test's own fp16 correlation inputs the float32 restatement alone stays within the
excused and differing shares of docs/flownet2_ops_parity.md."""
import pytest
import torch
import torch.nn.functional as F

import flow_ops_restatement as R
from oracle import flow_ops_oracle as O

D64 = torch.float64


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(float(b.abs().max()), 1e-300), float((a - b).abs().max())


def _corr_slices(a, b, pad, k, md, s1, s2):
    """second formulation: no padded copies; for every displacement and tap the valid output range is worked out and the product of
    two strided slices of the un-padded maps, summed over the channels, is added into it"""
    B, C, H, W = a.shape
    oC, oH, oW = R.correlation_out_shape(H, W, pad, k, md, s1, s2)
    kr, dr = (k - 1) // 2, md // s2
    D = 2 * dr + 1
    out = torch.zeros(B, oC, oH, oW, dtype=D64)

    def rng(n_out, n_in, off1, off2):
        """outputs o with 0 <= o s1 + off1 < n_in and 0 <= o s1 + off2 < n_in"""
        lo = max(0, -(min(off1, off2) // s1))                     # ceil(-min / s1)
        hi = min(n_out - 1, (n_in - 1 - max(off1, off2)) // s1)
        return lo, hi

    for tj in range(-dr, dr + 1):
        for ti in range(-dr, dr + 1):
            for j in range(-kr, kr + 1):
                for i in range(-kr, kr + 1):
                    ya, xa = md + kr - pad + j, md + kr - pad + i          # un-padded offset of the first factor at output 0
                    yb, xb = ya + tj * s2, xa + ti * s2
                    y0, y1 = rng(oH, H, ya, yb)
                    x0, x1 = rng(oW, W, xa, xb)
                    if y1 < y0 or x1 < x0:
                        continue
                    sl = lambda t, oy, ox: t[:, :, y0 * s1 + oy:y1 * s1 + oy + 1:s1, x0 * s1 + ox:x1 * s1 + ox + 1:s1]
                    out[:, (tj + dr) * D + ti + dr, y0:y1 + 1, x0:x1 + 1] += (sl(a, ya, xa) * sl(b, yb, xb)).sum(1)
    return out / (k * k * C)


ALL_CORR = [(B, C, H, W, pad, 1, md, s1, s2) for (B, C, H, W, pad, md, s1, s2) in R.K1_CASES] + R.GENERIC_CASES


@pytest.mark.parametrize('B,C,H,W,pad,k,md,s1,s2', ALL_CORR)
def test_correlation_restatement_vs_oracle_and_second_formulation(B, C, H, W, pad, k, md, s1, s2):
    g = R.gen(B, C, H, W, pad, k, md)
    a, b = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    ref = R.correlation(a, b, pad, k, md, s1, s2, D64)
    orc = O.correlation_fwd(a.numpy(), b.numpy(), pad, k, md, s1, s2)
    assert tuple(ref.shape[1:]) == O.correlation_out_shape(C, H, W, pad, k, md, s1, s2)
    _close(ref, torch.from_numpy(orc), 2.0 ** -23)                # the oracle accumulates in float64 and rounds its output once
    _close(ref, _corr_slices(a.double(), b.double(), pad, k, md, s1, s2))
    # wherever a term of the sum is not padding the output is not zero (random data), so the zeros are the all-padding positions
    s = R.correlation(a.abs(), b.abs(), pad, k, md, s1, s2, D64)
    assert bool(((ref == 0) == (s == 0)).all())


def test_correlation_nhwc_restatement_reads_the_slice_and_applies_the_slope():
    case = R.NHWC_CASES[1]
    B, C, H, W = case[:4]
    cs, coff, _, _ = R.nhwc_geometry(case, False)
    a, b, g = R.nhwc_maps(case, 0, False)
    ba, bb = R.nhwc_buffer(a, cs, coff, g), R.nhwc_buffer(b, cs, coff, g)
    plain = R.correlation(a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), 20, 1, 20, 1, 2, D64).permute(0, 2, 3, 1)
    for slope in (R.F32_SLOPE, 1.0, 0.0):
        _close(R.correlation_nhwc(ba, bb, cs, coff, B, C, H, W, slope, D64), torch.where(plain > 0, plain, plain * slope))


@pytest.mark.parametrize('case', R.NHWC_CASES, ids=['%dx%dx%dx%d' % c[:4] for c in R.NHWC_CASES])
def test_fp16_correlation_shares_of_the_float32_restatement(case):
    """on the GPU test's inputs, float32 accumulation alone: every element bit-equal to the float64 rounding, or excused and
    the rounding of a value within the allowance; excused share <= 8 %, differing share <= 0.5 %"""
    B, C, H, W, _, _, slope = case
    cs, coff, _, _ = R.nhwc_geometry(case, True)
    for gi in range(2):
        a, b, g = R.nhwc_maps(case, gi, True)
        ba, bb = R.nhwc_buffer(a, cs, coff, g), R.nhwc_buffer(b, cs, coff, g)
        ref, lo, hi, excused, share = R.correlation_nhwc_f16(ba, bb, cs, coff, B, C, H, W, slope)
        got = R.act16(R.correlation_nhwc(ba, bb, cs, coff, B, C, H, W, 1.0, torch.float32).half(), slope)
        differing, far = R.check_f16_correlation(got, ref, lo, hi, excused)
        print('C', C, 'excused', share, 'differing', differing, 'more than one ulp', far)
        assert share <= 0.08 and differing <= 0.005, (share, differing)


def test_nbrs16_and_act16():
    r = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0 ** -24, 65504.0, -0.5], dtype=torch.float16)
    up, dn = R.nbrs16(r)
    assert up.tolist() == [2.0 ** -24, 2.0 ** -24, 1 + 2.0 ** -10, -1 + 2.0 ** -11, 2.0 ** -23, float('inf'), -0.5 + 2.0 ** -12]
    assert dn.tolist() == [-2.0 ** -24, -2.0 ** -24, 1 - 2.0 ** -11, -1 - 2.0 ** -10, 0.0, 65472.0, -0.5 - 2.0 ** -11]
    assert torch.equal(R.act16(r, 1.0), r) and R.act16(r, 0.0).tolist() == [0.0, 0.0, 1.0, 0.0, 2.0 ** -24, 65504.0, 0.0]
    assert R.act16(r, R.F32_SLOPE)[3].item() == torch.tensor(-0.1, dtype=torch.float32).half().item()


# ---------------------------------------------------------------------------------------------- Resample2d, ChannelNorm, up-sampling
@pytest.mark.parametrize('H,W,fH,fW', [(9, 13, 9, 13), (9, 13, 6, 7)])
def test_resample2d_restatement_vs_oracle_and_grid_sample(H, W, fH, fW):
    g = R.gen(H, W, fH, fW)
    img = torch.randn(2, 3, H, W, generator=g)
    flow = torch.randn(2, 2, fH, fW, generator=g) * 4
    flow[0, :, 0] = 1e6
    flow[1, :, -1] = -1e6
    ref = R.resample2d(img, flow, D64)
    orc = torch.from_numpy(O.resample2d_fwd(img.numpy(), flow.numpy()))
    # the oracle forms x + dx in float32: |x + dx| < 32 moves the sample by at most 2^-20 of a pixel, times the image's slope
    assert float((ref - orc).abs().max()) <= 2.0 ** -19 * float(img.abs().max()) * 4
    # grid_sample (align_corners, border) on the top-left fH x fW corner of the image: the same function while the sample stays inside
    inside = torch.rand(2, 2, fH, fW, generator=g, dtype=D64)
    xs = inside[:, 0] * (fW - 1)
    ys = inside[:, 1] * (fH - 1)
    fl = torch.stack((xs - torch.arange(fW, dtype=D64).view(1, 1, fW), ys - torch.arange(fH, dtype=D64).view(1, fH, 1)), 1)
    grid = torch.stack((2 * xs / (W - 1) - 1, 2 * ys / (H - 1) - 1), -1)
    _close(R.resample2d(img, fl, D64), F.grid_sample(img.double(), grid, mode='bilinear', padding_mode='border', align_corners=True), 1e-11)


def test_resample2d_is_continuous_across_every_clamp_and_integer():
    """the gate-free claim: on either side of every integer coordinate (where floor() steps) and of both clamps the restatement's
    values differ by no more than the step times the image's largest slope"""
    g = R.gen(5, 7)
    H, W = 5, 7
    img = torch.randn(1, 2, H, W, generator=g).double()
    slope = float(max((img[..., 1:] - img[..., :-1]).abs().max(), (img[:, :, 1:] - img[:, :, :-1]).abs().max()))
    eps = 1e-9
    # a uniform flow of every integer from -(W + 2) to W + 2 sends every pixel over every integer coordinate and over both clamps of
    # its axis; the other axis sits on an integer, between two, and beyond either clamp
    for axis, n in ((0, W), (1, H)):
        for shift in range(-(n + 2), n + 3):
            for other in (0.0, 0.3, -30.0, 30.0):
                vals = []
                for side in (-eps, eps):
                    fl = torch.full((1, 2, H, W), other, dtype=D64)
                    fl[0, axis] = shift + side
                    vals.append(R.resample2d(img, fl, D64))
                assert float((vals[0] - vals[1]).abs().max()) <= 4 * eps * slope, (axis, shift, other)


def test_leaky_relu_is_continuous_at_zero():
    for slope in (R.F32_SLOPE, 1.0, 0.0):
        v = torch.tensor([-1e-12, 0.0, 1e-12], dtype=D64)
        assert float(R.act(v, slope).abs().max()) <= 1e-12


@pytest.mark.parametrize('C', [1, 2, 3, 64])
def test_channelnorm_restatement(C):
    x = torch.randn(2, C, 5, 7, generator=R.gen(C), dtype=D64)
    x[0, :, 0, 0] = 0
    ref = R.channelnorm(x, D64)
    _close(ref, torch.linalg.vector_norm(x, dim=1, keepdim=True))
    assert float(ref[0, 0, 0, 0]) == 0
    orc = O.channelnorm_fwd(x.float().numpy())
    _close(R.channelnorm(x.float(), D64), torch.from_numpy(orc), 2.0 ** -22)


@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 7)])
def test_flow_up4_restatement_vs_interpolate(h, w):
    f = torch.randn(2, h, w, 2, generator=R.gen(h, w), dtype=D64)
    n = f.permute(0, 3, 1, 2)
    _close(R.flow_up4(f, 0, 20.0, D64), F.interpolate(n, scale_factor=4, mode='nearest') * 20.0)
    _close(R.flow_up4(f, 1, 20.0, D64), F.interpolate(n, scale_factor=4, mode='bilinear', align_corners=False) * 20.0)
    _close(R.flow_up4(f, 2, 0.05, D64), F.interpolate(n, scale_factor=4, mode='bilinear', align_corners=True) * 0.05)


# ---------------------------------------------------------------------------------------------- the glue kernels
def test_prep_restatement():
    g = R.gen(3, 4, 6)
    inp = torch.randn(3, 3, 2, 4, 6, generator=g) * 5 + 200
    x6, i0, i1 = R.prep(inp, 255.0, D64)
    d = inp.double()
    x = (d - d.reshape(3, 3, -1).mean(-1).view(3, 3, 1, 1, 1)) / 255.0
    for c in range(3):
        _close(x6[..., c], x[:, c, 0])
        _close(x6[..., 3 + c], x[:, c, 1])
    assert float(x6[..., 6:].abs().max()) == 0 and float(i0[..., 3].abs().max()) == 0 and float(i1[..., 3].abs().max()) == 0
    assert torch.equal(i0[..., :3], x6[..., :3]) and torch.equal(i1[..., :3], x6[..., 3:6])
    assert float(x6[..., :6].reshape(3, -1, 2, 3).sum((1, 2)).abs().max()) < 1e-12                  # every colour has zero mean


def test_pack_orders_vs_the_oracle_ops():
    """the concatenation orders the header gives, composed from the numpy oracle's ops and F.interpolate"""
    g = R.gen(8, 12)
    B, H, W = 2, 8, 12
    x6 = torch.rand(B, H, W, 8, generator=g) - 0.5
    img1 = x6[..., 3:6].contiguous()
    fa, fb = torch.randn(B, 2, 3, 2, generator=g) * 0.1, torch.randn(B, 2, 3, 2, generator=g) * 2
    tol = 1e-5
    xn, im = x6[..., :6].permute(0, 3, 1, 2), img1.permute(0, 3, 1, 2).contiguous().numpy()
    for mode, kw in ((0, dict(mode='nearest')), (1, dict(mode='bilinear', align_corners=False)), (2, dict(mode='bilinear', align_corners=True))):
        fl = F.interpolate(fa.permute(0, 3, 1, 2), scale_factor=4, **kw) * 20.0
        wr = torch.from_numpy(O.resample2d_fwd(im, fl.numpy()))
        nrm = torch.from_numpy(O.channelnorm_fwd((xn[:, :3] - wr).numpy()))
        _close(R.warp_pack12(x6, img1, fa, mode, 20.0, 20.0, D64), torch.cat((xn, wr, fl / 20.0, nrm), 1).permute(0, 2, 3, 1), tol)
    up = lambda t: F.interpolate(t.permute(0, 3, 1, 2), scale_factor=4, mode='nearest')
    s2, sd = up(fa) * 20.0, up(fb) / 20.0
    cn = lambda t: torch.from_numpy(O.channelnorm_fwd(t.numpy()))
    rs = lambda f: torch.from_numpy(O.resample2d_fwd(im, f.numpy()))
    ref = torch.cat((xn[:, :3], sd, s2, cn(sd), cn(s2), cn(xn[:, :3] - rs(sd)), cn(xn[:, :3] - rs(s2)), torch.zeros(B, 1, H, W)), 1)
    _close(R.fusion_pack11(x6, img1, fa, fb, 20.0, D64), ref.permute(0, 2, 3, 1), tol)
