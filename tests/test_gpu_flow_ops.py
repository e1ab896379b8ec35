"""Kernel-level parity of the kernels between FlowNet2's conv stacks through the C ABI: vv_correlation_fwd (correlation_k1_kernel and
correlation_generic_kernel), vv_correlation_nhwc / _f16, vv_resample2d_fwd, vv_channelnorm_fwd, vv_flownet_prep, vv_warp_pack12,
vv_fusion_pack11 and their _f16 forms against the float64 restatements of tests/flow_ops_restatement.py (checked on the CPU by
tests/test_flow_ops_host.py).

Common to every case: sources sit inside wider pixels or buffers; pad channels, 64 elements in front of and 64 behind every buffer hold
finite random numbers.  Destinations are sentinel-filled with the same slack; everything outside the promised channels keeps the
sentinel bit for bit.  Every launch is repeated with all filler redrawn and must give the same bits.  Two groups of data per case, no
element left out, and every test asserts the dispatch condition it is meant to reach.

Bars (docs/flownet2_ops_parity.md): fp32 sums and interpolations meet the float-summation rule err_hip <= max(8 err_ref32, 16 * 2^-23),
err = max |x - ref64| / max |ref64| per output group, err_ref32 from the float32 evaluation of the same restatement.  Copied and zero
channels, nearest up-sampling times scale, img0 / img1 against x6, all-padding positions of the correlations, sentinels, refused calls
and repeated launches are bit-equal.  The fp16 correlation is bit-equal to the twice-rounded float64 value except where that value
lies within 8 * 2^-24 * sum |a| |b| / C of an fp16 rounding boundary (there the element may be the rounding of any value within that allowance; excused share <= 8 %,
differing share <= 0.5 %).  The fp16 glue kernels keep the one-ulp bar against the half graph of tests/test_flownet2_fp16.py.
"""
import numpy as np
import pytest
import torch

import flow_ops_restatement as R
from _util import FLOOR, SENT, err as _err, observe
from oracle import flow_ops_oracle as O

pytestmark = pytest.mark.gpu

SLACK = FRONT = 64
OK, BAD_ARG, UNSUPPORTED = 0, 1, 3
D64, D32 = torch.float64, torch.float32


def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _rule(op, what, got, ref64, ref32):
    e_hip, e_32 = _err(got, ref64), _err(ref32, ref64)
    observe('flow_ops:' + op, err_hip=e_hip, err_ref32=e_32, ratio=e_hip / max(8 * e_32, FLOOR))
    assert e_hip <= max(8 * e_32, FLOOR), (op, what, e_hip, e_32)


def _one_ulp(op, what, got, ref):
    d = (got.double() - ref.double()).abs()
    r = float((d / R.ulp16(ref.double())).max())
    observe('flow_ops:' + op, max_ulp=r, equal_share=float((got == ref).double().mean()))
    assert bool(torch.isfinite(got.float()).all()) and r <= 1.0, (op, what, r)


def _put(x, g, scale=1.0):
    """x flat (CPU) between FRONT and SLACK elements of fresh filler on the device: (buffer, pointer to x)"""
    buf = (torch.randn(FRONT + x.numel() + SLACK, generator=g) * scale).to(x.dtype)
    buf[FRONT:FRONT + x.numel()] = x.reshape(-1)
    d = buf.cuda()
    return d, d.data_ptr() + FRONT * d.element_size()


def _dst(n, dtype=D32):
    d = torch.full((FRONT + n + SLACK,), SENT, dtype=dtype, device='cuda')
    return d, d.data_ptr() + FRONT * d.element_size()


def _take(d, n):
    """the n elements behind FRONT; the slack on either side must hold the sentinel"""
    c = d.cpu()
    assert bool((c[:FRONT] == SENT).all()) and bool((c[FRONT + n:] == SENT).all()), 'slack around the destination changed'
    return c[FRONT:FRONT + n].clone()


def _take_slice(d, npix, ocs, ocoff, C):
    body = _take(d, npix * ocs).view(npix, ocs)
    keep = torch.ones(ocs, dtype=torch.bool)
    keep[ocoff:ocoff + C] = False
    assert bool((body[:, keep] == SENT).all()), 'channels beside the slice changed'
    return body[:, ocoff:ocoff + C].clone()


def _same(outs):
    a, b = outs
    if not isinstance(a, (tuple, list)):
        a, b = [a], [b]
    for p, q in zip(a, b):
        assert torch.equal(p, q) and p.dtype == q.dtype, 'the output depends on filler or slack'


# ================================================================================================ vv_correlation_fwd
def _k1_form(C, pad, md, s1, s2):
    """(D, lds bytes) of correlation_k1_kernel's launch (vv_flow.hip)"""
    dr = md // s2
    span = 31 * s1 + 2 * dr * s2 + 1
    return 2 * dr + 1, (C * 32 + 64 * (span | 1)) * 4


def _corr_fwd_case(op, B, C, H, W, pad, k, md, s1, s2):
    L, lib = _L()
    oC, oH, oW = R.correlation_out_shape(H, W, pad, k, md, s1, s2)
    n = B * oC * oH * oW
    zeros = None
    for gi in range(2):
        g = R.gen(B, C, H, W, pad, k, md, s1, s2, gi)
        a, b = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
        ref64, ref32 = R.correlation(a, b, pad, k, md, s1, s2, D64), R.correlation(a, b, pad, k, md, s1, s2, D32)
        zeros = R.correlation(a.abs(), b.abs(), pad, k, md, s1, s2, D64) == 0          # every term is padding
        outs = []
        for rep in range(2):
            (da, pa), (db, pb) = _put(a, g), _put(b, g)
            out, po = _dst(n)
            L.check(lib.vv_correlation_fwd(pa, pb, po, B, C, H, W, pad, k, md, s1, s2, 1, _st()), op)
            _sync()
            outs.append(_take(out, n).view(B, oC, oH, oW))
        _same(outs)
        _rule(op, (gi,), outs[0], ref64, ref32)
        assert bool((outs[0][zeros] == 0).all()), 'an all-padding position is not exactly 0'
    return oW, zeros


@pytest.mark.parametrize('idx', range(len(R.K1_CASES)), ids=['%dx%dx%dx%d-p%d-m%d-s%d%d' % c for c in R.K1_CASES])
def test_correlation_k1(idx):
    B, C, H, W, pad, md, s1, s2 = R.K1_CASES[idx]
    D, lds = _k1_form(C, pad, md, s1, s2)
    assert D <= 24 and lds <= 160 * 1024
    oW, zeros = _corr_fwd_case('corr_k1', B, C, H, W, pad, 1, md, s1, s2)
    assert (lds > 64 * 1024) == (idx == 5)                                   # the opt-in LDS size: the last case only
    if idx == 0:
        assert C > 64 and C % 64 == 16 and oW == 33
    elif idx == 1:
        assert s1 == 2 and C < 64 and oW == 35
    elif idx == 2:
        assert pad < md and md % s2 != 0 and md // s2 == 2
    elif idx == 3:
        assert pad > md and bool(zeros[:, :, :pad - md].all()) and bool(zeros[:, :, -(pad - md):].all())
    elif idx == 4:
        assert D == 23


def test_correlation_fwd_refused_calls_write_nothing():
    L, lib = _L()
    g = R.gen(77)

    def call(want, C=8, H=3, W=32, pad=20, k=1, md=20, s1=1, s2=2, mul=1):
        oC, oH, oW = R.correlation_out_shape(H, W, pad, k, md, s1, s2)
        n = oC * oH * oW
        (da, pa), (db, pb) = _put(torch.randn(C * H * W, generator=g), g), _put(torch.randn(C * H * W, generator=g), g)
        out, po = _dst(n)
        st = lib.vv_correlation_fwd(pa, pb, po, 1, C, H, W, pad, k, md, s1, s2, mul, _st())
        _sync()
        assert st == want, (st, want, C, k, md, mul)
        assert bool((out == SENT).all())

    assert _k1_form(8, 24, 24, 1, 2)[0] == 25 and _k1_form(1300, 20, 20, 1, 2)[1] > 160 * 1024
    call(UNSUPPORTED, pad=24, md=24)             # D = 25
    call(UNSUPPORTED, C=1300)                    # more than 160 KiB of LDS
    call(UNSUPPORTED, mul=0)
    call(UNSUPPORTED, k=2)
    call(UNSUPPORTED, k=0)


@pytest.mark.parametrize('B,C,H,W,pad,k,md,s1,s2', R.GENERIC_CASES)
def test_correlation_generic(B, C, H, W, pad, k, md, s1, s2):
    assert k > 1 and k % 2 == 1
    if (B, C, H, W, pad, k, md, s1, s2) == R.GENERIC_CASES[-1]:
        assert k == 3 and s1 == 2 and pad != md
    _corr_fwd_case('corr_generic', B, C, H, W, pad, k, md, s1, s2)


# ================================================================================================ vv_correlation_nhwc / _f16
def _nhwc_conditions(idx, case, half):
    B, C, H, W, wide, ocoff, slope = case
    cs, coff, ocs, _ = R.nhwc_geometry(case, half)
    assert ocs not in (476, 480) and (cs > C) == wide == (coff > 0) and (coff * (2 if half else 4)) % 16 == 0
    assert [idx == 0, idx == 1, idx in (2, 3)] == [C == 16 and H == 1, C == 48, H >= 41]      # one chunk; three; all 21 rows valid at once
    assert (W == 64) == (idx in (0, 2, 5))


def _nhwc_launch(case, half, a, b, g):
    L, lib = _L()
    B, C, H, W, wide, ocoff, slope = case
    cs, coff, ocs, _ = R.nhwc_geometry(case, half)
    ba, bb = R.nhwc_buffer(a, cs, coff, g), R.nhwc_buffer(b, cs, coff, g)
    (da, pa), (db, pb) = _put(ba, g, 0.7), _put(bb, g, 0.7)
    es = 2 if half else 4
    out, po = _dst(B * H * W * ocs, torch.float16 if half else D32)
    fn = lib.vv_correlation_nhwc_f16 if half else lib.vv_correlation_nhwc
    L.check(fn(pa + coff * es, pb + coff * es, cs, B, C, H, W, po, ocs, ocoff, slope, _st()), 'correlation_nhwc')
    _sync()
    return _take_slice(out, B * H * W, ocs, ocoff, 441).view(B, H, W, 441), ba, bb


def _row_zeros(case, a, b):
    """all-padding positions; a row displacement wholly outside the image is among them in every case"""
    B, C, H, W = case[:4]
    z = R.correlation_nhwc(a.abs().reshape(-1), b.abs().reshape(-1), C, 0, B, C, H, W, 1.0, D64) == 0
    assert bool(z.view(B, H, W, 21, 21).all(4).all(2).any()), 'no row displacement lies wholly outside'
    if H == 1:
        assert bool(z.view(B, H, W, 21, 21)[:, :, :, [t for t in range(21) if t != 10]].all())
    return z


@pytest.mark.parametrize('idx', range(len(R.NHWC_CASES)), ids=['%dx%dx%dx%d' % c[:4] for c in R.NHWC_CASES])
def test_correlation_nhwc(idx):
    """out_coff = 3 is allowed: the header asks no alignment of out_cstride / out_coff (the kernel stores single elements)"""
    case = R.NHWC_CASES[idx]
    _nhwc_conditions(idx, case, False)
    B, C, H, W, wide, ocoff, slope = case
    cs, coff = R.nhwc_geometry(case, False)[:2]
    for gi in range(2):
        a, b, g = R.nhwc_maps(case, gi, False)
        outs, bufs = [], None
        for rep in range(2):
            got, ba, bb = _nhwc_launch(case, False, a, b, g)
            outs.append(got)
            bufs = bufs or (ba, bb)
        _same(outs)
        ref64 = R.correlation_nhwc(bufs[0], bufs[1], cs, coff, B, C, H, W, slope, D64)
        ref32 = R.correlation_nhwc(bufs[0], bufs[1], cs, coff, B, C, H, W, slope, D32)
        _rule('corr_nhwc_w%d' % W, (gi,), outs[0], ref64, ref32)
        assert bool((outs[0][_row_zeros(case, a, b)] == 0).all())


@pytest.mark.parametrize('idx', range(len(R.NHWC_CASES)), ids=['%dx%dx%dx%d' % c[:4] for c in R.NHWC_CASES])
def test_correlation_nhwc_f16(idx):
    case = R.NHWC_CASES[idx]
    _nhwc_conditions(idx, case, True)
    B, C, H, W, wide, ocoff, slope = case
    cs, coff = R.nhwc_geometry(case, True)[:2]
    for gi in range(2):
        a, b, g = R.nhwc_maps(case, gi, True)
        outs, bufs = [], None
        for rep in range(2):
            got, ba, bb = _nhwc_launch(case, True, a, b, g)
            outs.append(got)
            bufs = bufs or (ba, bb)
        _same(outs)
        ref, lo, hi, excused, share = R.correlation_nhwc_f16(bufs[0], bufs[1], cs, coff, B, C, H, W, slope)
        differing, far = R.check_f16_correlation(outs[0], ref, lo, hi, excused)
        observe('flow_ops:corr_nhwc_f16_w%d_c%d' % (W, C), excused=share, differing=differing, beyond_one_ulp=far)
        assert share <= 0.08 and differing <= 0.005, (share, differing)
        z = _row_zeros(case, a.float(), b.float())
        assert bool((outs[0][z].view(torch.int16) == 0).all())                # +0, bit for bit


@pytest.mark.parametrize('half', [False, True])
def test_correlation_nhwc_refused_calls_write_nothing(half):
    L, lib = _L()
    g = R.gen(5, int(half))
    dt, es = (torch.float16, 2) if half else (D32, 4)
    B, C, H = 1, 32, 2
    (da, pa), (db, pb) = _put(torch.randn(H * 128 * 48, generator=g).to(dt), g), _put(torch.randn(H * 128 * 48, generator=g).to(dt), g)
    out, po = _dst(H * 128 * 480, dt)
    fn = lib.vv_correlation_nhwc_f16 if half else lib.vv_correlation_nhwc
    q = 8 if half else 4

    def call(want, pa=pa, pb=pb, cs=C + q, C=C, W=128):
        st = fn(pa, pb, cs, B, C, H, W, po, 480, 32, 0.1, _st())
        assert st == want, (st, want, cs, C, W)

    call(UNSUPPORTED, W=96)
    call(UNSUPPORTED, C=24, cs=24 + q)
    call(UNSUPPORTED, cs=C - q)                  # cstride < C
    call(UNSUPPORTED, cs=C + q // 2)             # a pixel stride that is no multiple of 16 bytes
    call(BAD_ARG, pa=pa + es)                    # misaligned
    call(BAD_ARG, pb=pb + 8)
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_resample2d_fwd, vv_channelnorm_fwd
def _edge_flows(B, fH, fW, g):
    """random flows of a few pixels with rows / columns of special values: exact integers, -0.0, samples 2^-10 inside and outside every
    edge, +-1e6"""
    f = torch.randn(B, 2, fH, fW, generator=g) * 3
    d = 2.0 ** -10
    xs, ys = torch.arange(fW, dtype=D32), torch.arange(fH, dtype=D32).view(fH, 1)
    f[:, :, 0] = f[:, :, 0].round()
    f[0, :, 0, :2] = -0.0
    for r, t in enumerate((-d, d, fW - 1 + d, fW - 1 - d), start=1):          # x lands at t in row r
        f[:, 0, r] = t - xs
    for c, t in enumerate((-d, d, fH - 1 + d, fH - 1 - d), start=1):          # y lands at t in column c
        f[:, 1, :, c] = t - ys[:, 0]
    f[:, :, 5, :3], f[:, :, 5, 3:] = 1e6, -1e6
    f[:, 0, :, 5], f[:, 1, :, 5] = -1e6, 1e6
    f[:, 1, 5, 5] = -1e6
    assert float(f.abs().max()) < 2 ** 31
    return f


@pytest.mark.parametrize('B,C,H,W,fH,fW', [(2, 3, 9, 13, 9, 13), (2, 1, 9, 13, 6, 7), (3, 3, 20, 28, 20, 28), (1, 5, 33, 20, 31, 9)])
def test_resample2d(B, C, H, W, fH, fW):
    """flows stay far inside the int range: above it the kernel relies on the float-to-int conversion saturating (not launched)"""
    L, lib = _L()
    assert [fH < H and fW < W, C == 1] == [(H, W) != (fH, fW), (C, fH) == (1, 6)]
    for gi in range(2):
        g = R.gen(B, C, H, W, fH, fW, gi)
        img, flow = torch.randn(B, C, H, W, generator=g), _edge_flows(B, fH, fW, g)
        ref64, ref32 = R.resample2d(img, flow, D64), R.resample2d(img, flow, D32)
        outs = []
        for rep in range(2):
            (di, pi), (df, pf) = _put(img, g), _put(flow, g)
            out, po = _dst(B * C * fH * fW)
            L.check(lib.vv_resample2d_fwd(pi, pf, po, B, C, H, W, fH, fW, 1, _st()), 'resample2d')
            _sync()
            outs.append(_take(out, B * C * fH * fW).view(B, C, fH, fW))
        _same(outs)
        assert np.array_equal(outs[0].numpy(), O.resample2d_fwd(img.numpy(), flow.numpy()))      # bit exact: the same operation order
        _rule('resample2d', (gi,), outs[0], ref64, ref32)


def test_resample2d_refused():
    L, lib = _L()
    g = R.gen(3)
    (di, pi), (df, pf) = _put(torch.randn(3 * 8 * 8, generator=g), g), _put(torch.randn(2 * 9 * 9, generator=g), g)
    out, po = _dst(3 * 9 * 9)
    assert lib.vv_resample2d_fwd(pi, pf, po, 1, 3, 8, 8, 9, 8, 1, _st()) == BAD_ARG          # flow taller than the image
    assert lib.vv_resample2d_fwd(pi, pf, po, 1, 3, 8, 8, 8, 9, 1, _st()) == BAD_ARG
    assert lib.vv_resample2d_fwd(pi, pf, po, 1, 3, 8, 8, 8, 8, 2, _st()) == UNSUPPORTED
    _sync()
    assert bool((out == SENT).all())


@pytest.mark.parametrize('C', [1, 2, 3, 64])
def test_channelnorm(C):
    L, lib = _L()
    B, H, W = 2, 9, 31
    assert (H * W) % 256 != 0 and B * H * W > 512
    for gi in range(2):
        g = R.gen(C, gi)
        x = torch.randn(B, C, H, W, generator=g)
        x[0, :, 0, 0] = 0
        x[1, :, H - 1, W - 1] = 0
        outs = []
        for rep in range(2):
            dx, px = _put(x, g)
            out, po = _dst(B * H * W)
            L.check(lib.vv_channelnorm_fwd(px, po, B, C, H, W, 2, _st()), 'channelnorm')
            _sync()
            outs.append(_take(out, B * H * W).view(B, 1, H, W))
        _same(outs)
        _rule('channelnorm', (gi, C), outs[0], R.channelnorm(x, D64), R.channelnorm(x, D32))
        assert float(outs[0][0, 0, 0, 0]) == 0 and float(outs[0][1, 0, H - 1, W - 1]) == 0
    out, po = _dst(B * H * W)
    assert lib.vv_channelnorm_fwd(px, po, B, C, H, W, 1, _st()) == UNSUPPORTED
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_flownet_prep
PREP = [(2, 4, 4), (2, 8, 12), (3, 20, 28), (1, 192, 192)]


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
@pytest.mark.parametrize('B,H,W', PREP)
def test_flownet_prep(B, H, W, half):
    """inputs of mean 200 and standard deviation 5 per colour: x - mean cancels.  The fp16 form gets inputs that fp16 holds exactly
    (as 8-bit frames are), so that the half graph's mean of the rounded inputs is the kernel's mean of the inputs."""
    L, lib = _L()
    HW = H * W
    assert (2 * HW // 4 > 64 * 256) == (HW == 192 * 192)              # a lane of prep_sum_kernel adds more than one float4
    assert HW % 2 == 0
    dt, ics = (torch.float16, 8) if half else (D32, 4)
    wsb = int(lib.vv_flownet_prep_workspace_bytes(B))
    assert wsb == B * 3 * 64 * 8
    fn = lib.vv_flownet_prep_f16 if half else lib.vv_flownet_prep
    for gi in range(2):
        g = R.gen(B, H, W, gi)
        inp = torch.randn(B, 3, 2, H, W, generator=g) * 5 + 200
        if half:
            inp = inp.half().float()
        outs = []
        for rep in range(2):
            di, pi = _put(inp, g, 200.0)
            ws, pw = _dst(wsb // 8, D64)
            (x6, p6), (i0, p0), (i1, p1) = _dst(B * HW * 8, dt), _dst(B * HW * ics, dt), _dst(B * HW * ics, dt)
            L.check(fn(pi, B, H, W, 255.0, pw, wsb, p6, p0, p1, _st()), 'prep')
            _sync()
            _take(ws, wsb // 8)
            outs.append((_take(x6, B * HW * 8).view(B, H, W, 8), _take(i0, B * HW * ics).view(B, H, W, ics),
                         _take(i1, B * HW * ics).view(B, H, W, ics)))
        _same(outs)
        x6, i0, i1 = outs[0]
        assert bool((x6[..., 6:] == 0).all()) and bool((i0[..., 3] == 0).all()) and bool((i1[..., 3] == 0).all())
        assert torch.equal(i0[..., :3], x6[..., :3]) and torch.equal(i1[..., :3], x6[..., 3:6])
        if half:
            assert bool((i0[..., 4:] == SENT).all()) and bool((i1[..., 4:] == SENT).all())
            x = inp.half()
            mean = x.double().view(B, 3, -1).mean(-1).half().view(B, 3, 1, 1, 1)
            xn = ((x - mean).float() / 255.0).half()
            ref = torch.cat((xn[:, :, 0], xn[:, :, 1]), 1).permute(0, 2, 3, 1)
            _one_ulp('prep_f16', (gi,), x6[..., :6], ref)
        else:
            _rule('prep', (gi,), x6[..., :6], R.prep(inp, 255.0, D64)[0][..., :6], R.prep(inp, 255.0, D32)[0][..., :6])


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
def test_flownet_prep_refused_calls_write_nothing(half):
    """an odd H * W is refused: prep_sum_kernel loads float4 from the start of every (image, colour) block of 2 H W floats, which is
    16-byte aligned only when H W is even"""
    L, lib = _L()
    g = R.gen(9, int(half))
    dt = torch.float16 if half else D32
    fn = lib.vv_flownet_prep_f16 if half else lib.vv_flownet_prep
    B, H, W = 2, 8, 12
    di, pi = _put(torch.randn(B * 6 * H * W, generator=g), g)
    wsb = int(lib.vv_flownet_prep_workspace_bytes(B))
    ws, pw = _dst(wsb // 8, D64)
    (x6, p6), (i0, p0), (i1, p1) = _dst(B * H * W * 8, dt), _dst(B * H * W * 8, dt), _dst(B * H * W * 8, dt)
    assert fn(pi, B, 5, 7, 255.0, pw, wsb, p6, p0, p1, _st()) == UNSUPPORTED            # odd H * W
    assert fn(pi, B, H, W, 255.0, pw, wsb - 8, p6, p0, p1, _st()) == BAD_ARG           # short workspace
    assert fn(pi + 4, B, H, W, 255.0, pw, wsb, p6, p0, p1, _st()) == BAD_ARG           # misaligned pointers
    assert fn(pi, B, H, W, 255.0, pw, wsb, p6 + 8, p0, p1, _st()) == BAD_ARG
    assert fn(pi, B, H, W, 255.0, pw, wsb, p6, p0 + 8, p1, _st()) == BAD_ARG
    assert fn(pi, B, H, W, 255.0, pw, wsb, p6, p0, p1 + 8, _st()) == BAD_ARG
    assert fn(pi, B, 0, W, 255.0, pw, wsb, p6, p0, p1, _st()) == BAD_ARG
    _sync()
    for t in (ws, x6, i0, i1):
        assert bool((t == SENT).all())


# ================================================================================================ vv_warp_pack12, vv_fusion_pack11
GLUE = [(2, 4, 4, 2), (2, 8, 12, 4), (3, 20, 28, 8)]            # (B, H, W, flow pixel stride)


def _flow2(B, h, w, W, per_unit, g, gi):
    """flow2 [B, h, w, 2] whose up-sampled, scaled values span a fraction of a pixel, a few pixels and +-(W + 5) (off the image);
    per_unit = flow2 units per pixel of the final flow"""
    f = torch.randn(B, h, w, 2, generator=g)
    kind = (torch.arange(B * h * w).view(B, h, w, 1) + gi) % 3
    px = torch.where(kind == 0, f * 0.3, torch.where(kind == 1, f * 3.0, torch.sign(f) * (W + 5)))
    return px * per_unit


def _pixels(x, cs, g, amp=0.5):
    """x [B, H, W, C] inside pixels cs wide with random pad channels, flat"""
    B, H, W, C = x.shape
    buf = ((torch.rand(B, H, W, cs, generator=g) - 0.5) * 2 * amp).to(x.dtype)
    buf[..., :C] = x
    return buf.reshape(-1)


def _check_warp_f32(op, gi, mode, got, x6, img1, f2, scale, div):
    ref64, ref32 = (R.warp_pack12(x6, img1, f2, mode, scale, div, dt) for dt in (D64, D32))
    assert torch.equal(got[..., :6], x6[..., :6]), 'copied channels'
    _rule(op + '_warped', (gi, mode), got[..., 6:9], ref64[..., 6:9], ref32[..., 6:9])
    _rule(op + '_flow', (gi, mode), got[..., 9:11], ref64[..., 9:11], ref32[..., 9:11])
    _rule(op + '_norm', (gi, mode), got[..., 11], ref64[..., 11], ref32[..., 11])
    if mode == 0:         # nearest times scale is one float product; the division by div_flow is correctly rounded
        assert torch.equal(got[..., 9:11], R.flow_up4(f2, 0, scale, D32).permute(0, 2, 3, 1) / torch.tensor(div, dtype=D32))


@pytest.mark.parametrize('B,H,W,fcs', GLUE)
def test_warp_pack12(B, H, W, fcs):
    L, lib = _L()
    h, w, npix = H // 4, W // 4, B * H * W
    assert (h == 1 and w == 1) == (H == 4) and (npix > 512) == (H == 20)
    for gi in range(2):
        g = R.gen(B, H, W, fcs, gi)
        scale, div = (20.0, 20.0) if gi == 0 else (5.0, 20.0)
        x6, img1 = torch.rand(B, H, W, 6, generator=g) - 0.5, torch.rand(B, H, W, 3, generator=g) - 0.5
        f2 = _flow2(B, h, w, W, 1 / scale, g, gi)
        for mode in (0, 1, 2):
            outs = []
            for rep in range(2):
                (d6, p6), (d1, p1), (df, pf) = _put(_pixels(x6, 8, g), g), _put(_pixels(img1, 4, g), g), _put(_pixels(f2, fcs, g, 2.0), g)
                out, po = _dst(npix * 12)
                L.check(lib.vv_warp_pack12(p6, p1, pf, fcs, B, H, W, mode, scale, div, po, _st()), 'warp_pack12')
                _sync()
                outs.append(_take(out, npix * 12).view(B, H, W, 12))
            _same(outs)
            _check_warp_f32('warp_pack12_mode%d' % mode, gi, mode, outs[0], x6, img1, f2, scale, div)


@pytest.mark.parametrize('B,H,W,fcs', GLUE)
def test_fusion_pack11(B, H, W, fcs):
    L, lib = _L()
    h, w, npix = H // 4, W // 4, B * H * W
    sdcs = {2: 8, 4: 2, 8: 4}[fcs]
    div = 20.0
    for gi in range(2):
        g = R.gen(B, H, W, fcs, gi, 11)
        x6, img1 = torch.rand(B, H, W, 6, generator=g) - 0.5, torch.rand(B, H, W, 3, generator=g) - 0.5
        s2f, sdf = _flow2(B, h, w, W, 1 / div, g, gi), _flow2(B, h, w, W, div, g, gi + 1)
        outs = []
        for rep in range(2):
            (d6, p6), (d1, p1) = _put(_pixels(x6, 8, g), g), _put(_pixels(img1, 4, g), g)
            (ds, ps), (dd, pd) = _put(_pixels(s2f, fcs, g, 2.0), g), _put(_pixels(sdf, sdcs, g, 2.0), g)
            out, po = _dst(npix * 12)
            L.check(lib.vv_fusion_pack11(p6, p1, ps, fcs, pd, sdcs, B, H, W, div, po, _st()), 'fusion_pack11')
            _sync()
            outs.append(_take(out, npix * 12).view(B, H, W, 12))
        _same(outs)
        got = outs[0]
        ref64, ref32 = (R.fusion_pack11(x6, img1, s2f, sdf, div, dt) for dt in (D64, D32))
        assert torch.equal(got[..., :3], x6[..., :3]), 'copied channels'
        assert torch.equal(got[..., 5:7], R.flow_up4(s2f, 0, div, D32).permute(0, 2, 3, 1)), 'nearest up-sampling times div_flow'
        assert bool((got[..., 11] == 0).all())
        _rule('fusion_pack11_sd', (gi,), got[..., 3:5], ref64[..., 3:5], ref32[..., 3:5])
        for c, name in ((7, 'norm_sd'), (8, 'norm_s2'), (9, 'diff_sd'), (10, 'diff_s2')):
            _rule('fusion_pack11_' + name, (gi,), got[..., c], ref64[..., c], ref32[..., c])


def _warp_f16_bar(op, gi, got, x, f2, mode, scale, div):
    """One ulp per materialised tensor.  The flow channels are within one ulp of the half graph's.  The warped image and the norm are
    computed FROM the up-sampled flow, which the kernel forms in float32: where that lands on the other side of an fp16 rounding
    boundary (modes 1 and 2; about 2^-24 * 64 of the flow against half a step of 2^-11, some 1e-3 of the elements) the flow is one
    ulp off and what is warped with it moves by far more than an ulp.  Such a pixel is held to the half graph evaluated with the flow
    moved by one fp16 step in dx and / or dy; at most 1 % of the pixels may need that."""
    import itertools
    ref = R.half_warp_pack12(x, f2, mode, scale, div)
    ulps = lambda r: (got.double() - r.double()).abs() / R.ulp16(r.double())
    d = ulps(ref)
    _one_ulp(op + '_copied_and_flow', (gi,), got[:, [0, 1, 2, 3, 4, 5, 9, 10]], ref[:, [0, 1, 2, 3, 4, 5, 9, 10]])
    direct = (d[:, [6, 7, 8, 11]] <= 1).all(1)
    ok = direct.clone()
    if not bool(ok.all()):
        for step in itertools.product((-1, 0, 1), repeat=2):
            ok |= (ulps(R.half_warp_pack12(x, f2, mode, scale, div, step))[:, [6, 7, 8, 11]] <= 1).all(1)
    share = 1 - float(direct.double().mean())
    observe('flow_ops:' + op, max_ulp=float(d.max()), equal_share=float((got == ref).double().mean()), flow_step_share=share)
    assert bool(ok.all()) and share <= 0.01 and (mode != 0 or share == 0), (op, gi, share, int((~ok).sum()))


@pytest.mark.parametrize('B,H,W,fcs', GLUE)
def test_warp_pack12_f16(B, H, W, fcs):
    L, lib = _L()
    h, w, npix = H // 4, W // 4, B * H * W
    for gi in range(2):
        g = R.gen(B, H, W, fcs, gi, 16)
        scale = div = 20.0
        x = (torch.rand(B, 6, H, W, generator=g) - 0.5).half()
        f2 = _flow2(B, h, w, W, 1 / scale, g, gi).half()
        xn = x.permute(0, 2, 3, 1)
        for mode in (0, 1, 2):
            outs = []
            for rep in range(2):
                (d6, p6), (d1, p1) = _put(_pixels(xn, 8, g), g), _put(_pixels(xn[..., 3:], 8, g), g)
                df, pf = _put(_pixels(f2, fcs, g, 2.0), g)
                out, po = _dst(npix * 16, torch.float16)
                L.check(lib.vv_warp_pack12_f16(p6, p1, pf, fcs, B, H, W, mode, scale, div, po, _st()), 'warp_pack12_f16')
                _sync()
                outs.append(_take_slice(out, npix, 16, 0, 12).view(B, H, W, 12))
            _same(outs)
            assert torch.equal(outs[0][..., :6], xn), 'copied channels'
            _warp_f16_bar('warp_pack12_f16_mode%d' % mode, gi, outs[0].permute(0, 3, 1, 2), x, f2.permute(0, 3, 1, 2), mode, scale, div)


@pytest.mark.parametrize('B,H,W,fcs', GLUE)
def test_fusion_pack11_f16(B, H, W, fcs):
    L, lib = _L()
    h, w, npix = H // 4, W // 4, B * H * W
    sdcs = {2: 8, 4: 2, 8: 4}[fcs]
    div = 20.0
    for gi in range(2):
        g = R.gen(B, H, W, fcs, gi, 17)
        x = (torch.rand(B, 6, H, W, generator=g) - 0.5).half()
        s2f, sdf = _flow2(B, h, w, W, 1 / div, g, gi).half(), _flow2(B, h, w, W, div, g, gi + 1).half()
        xn = x.permute(0, 2, 3, 1)
        outs = []
        for rep in range(2):
            (d6, p6), (d1, p1) = _put(_pixels(xn, 8, g), g), _put(_pixels(xn[..., 3:], 8, g), g)
            (ds, ps), (dd, pd) = _put(_pixels(s2f, fcs, g, 2.0), g), _put(_pixels(sdf, sdcs, g, 2.0), g)
            out, po = _dst(npix * 16, torch.float16)
            L.check(lib.vv_fusion_pack11_f16(p6, p1, ps, fcs, pd, sdcs, B, H, W, div, po, _st()), 'fusion_pack11_f16')
            _sync()
            outs.append(_take_slice(out, npix, 16, 0, 12).view(B, H, W, 12))
        _same(outs)
        got = outs[0]
        assert torch.equal(got[..., :3], xn[..., :3]) and bool((got[..., 11] == 0).all())
        _one_ulp('fusion_pack11_f16', (gi,), got[..., :11].permute(0, 3, 1, 2),
                 R.half_fusion_pack11(x, s2f.permute(0, 3, 1, 2), sdf.permute(0, 3, 1, 2), div))


@pytest.mark.parametrize('half', [False, True], ids=['f32', 'f16'])
def test_pack_refused_calls_write_nothing(half):
    L, lib = _L()
    g = R.gen(21, int(half))
    dt = torch.float16 if half else D32
    B, H, W = 1, 8, 8
    mk = lambda n: _put(torch.randn(n, generator=g).to(dt), g)
    (d6, p6), (d1, p1), (df, pf), (dg, pg) = mk(B * H * W * 8), mk(B * H * W * 8), mk(B * 4 * 8), mk(B * 4 * 8)
    out, po = _dst(B * H * W * 16, dt)
    warp = lib.vv_warp_pack12_f16 if half else lib.vv_warp_pack12
    fus = lib.vv_fusion_pack11_f16 if half else lib.vv_fusion_pack11
    assert warp(p6, p1, pf, 4, B, 6, W, 1, 20.0, 20.0, po, _st()) == BAD_ARG            # H = 6
    assert warp(p6, p1, pf, 4, B, H, 6, 1, 20.0, 20.0, po, _st()) == BAD_ARG
    assert warp(p6, p1, pf, 4, B, H, W, 3, 20.0, 20.0, po, _st()) == BAD_ARG            # mode = 3
    assert warp(p6, p1, pf, 4, B, H, W, -1, 20.0, 20.0, po, _st()) == BAD_ARG
    assert warp(p6, p1, pf, 3, B, H, W, 1, 20.0, 20.0, po, _st()) == BAD_ARG            # an odd flow stride
    assert warp(p6, p1, pf, 0, B, H, W, 1, 20.0, 20.0, po, _st()) == BAD_ARG
    assert fus(p6, p1, pf, 4, pg, 4, B, 6, W, 20.0, po, _st()) == BAD_ARG
    assert fus(p6, p1, pf, 3, pg, 4, B, H, W, 20.0, po, _st()) == BAD_ARG
    assert fus(p6, p1, pf, 4, pg, 5, B, H, W, 20.0, po, _st()) == BAD_ARG
    _sync()
    assert bool((out == SENT).all())
