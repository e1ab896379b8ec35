"""The float64 restatements of tests/flownet2_ops_restatement.py against torch.nn.functional in float64 on the CPU (no GPU), and their
layouts against the index formulas of include/vecvad_hip.h evaluated element by element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flownet2_ops_restatement as R
from _util import gen

F64 = torch.float64


def _close(a, b):
    scale = float(b.abs().max())
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * scale, float((a - b).abs().max()) / scale


# (R, stride, B, H, W, Cin, Cout, cstride, coff, slope, bias): stride 2 on odd and even sizes, coff != 0, Cin not a multiple of 4
CONV = [(1, 1, 2, 5, 7, 19, 6, 28, 4, 0.1, True), (3, 1, 2, 6, 9, 5, 7, 12, 4, 0.1, True), (3, 2, 3, 11, 14, 19, 5, 28, 4, 0.1, True),
        (3, 2, 1, 12, 13, 7, 4, 8, 0, 1.0, False), (5, 2, 2, 9, 10, 3, 6, 12, 8, 0.1, True), (7, 2, 2, 21, 22, 3, 8, 4, 0, 0.1, True),
        (7, 2, 1, 22, 21, 6, 3, 16, 4, 0.3, True)]


@pytest.mark.parametrize('Rk,stride,B,H,W,Cin,Cout,cs,coff,slope,has_bias', CONV)
def test_conv_restatement_vs_torch(Rk, stride, B, H, W, Cin, Cout, cs, coff, slope, has_bias):
    g = gen(Rk, stride, B, H, W, Cin, Cout)
    buf = torch.randn(B * H * W * cs + 64, generator=g, dtype=F64)
    w = torch.randn(Cout, Cin, Rk, Rk, generator=g, dtype=F64)
    bias = torch.randn(Cout, generator=g, dtype=F64) if has_bias else None
    x = R.view_read(buf, B * H * W, cs, coff, Cin).reshape(B, H, W, Cin)
    ref = F.leaky_relu(F.conv2d(x.permute(0, 3, 1, 2), w, bias, stride=stride, padding=(Rk - 1) // 2), slope).permute(0, 2, 3, 1)
    _close(R.conv_nhwc(x, w, bias, stride, slope), ref)
    assert ref.shape[1:3] == (R.conv_out_size(H, Rk, stride), R.conv_out_size(W, Rk, stride))
    # the view round trip: what view_fill writes is what view_read returns, the rest of the buffer stays
    buf2 = torch.full_like(buf, 3.0)
    R.view_fill(buf2, x, cs, coff)
    assert torch.equal(R.view_read(buf2, B * H * W, cs, coff, Cin).reshape(x.shape), x)
    assert int((buf2 != 3.0).sum()) <= x.numel() and torch.equal(buf2[B * H * W * cs:], torch.full((64,), 3.0, dtype=F64))


@pytest.mark.parametrize('B,H,W,Cin,Cout,slope,has_bias', [(2, 4, 6, 2, 2, 1.0, False), (3, 5, 7, 19, 6, 0.1, True), (1, 1, 3, 5, 4, 0.1, True)])
def test_deconv_restatement_vs_torch(B, H, W, Cin, Cout, slope, has_bias):
    g = gen(B, H, W, Cin, Cout)
    x = torch.randn(B, H, W, Cin, generator=g, dtype=F64)
    w = torch.randn(Cin, Cout, 4, 4, generator=g, dtype=F64)
    bias = torch.randn(Cout, generator=g, dtype=F64) if has_bias else None
    ref = F.leaky_relu(F.conv_transpose2d(x.permute(0, 3, 1, 2), w, bias, stride=2, padding=1), slope).permute(0, 2, 3, 1)
    _close(R.deconv_nhwc(x, w, bias, slope), ref)


@pytest.mark.parametrize('transposed', [0, 1])
def test_packed_panel_layout(transposed):
    """every element of the panel against the header's index formula: [taps][KP/8][2][NP][4], k = kq*8 + half*4 + j"""
    K, KP, N, NP, Rk = 11, 16, 35, 64, 4 if transposed else 3
    g = gen(K, N, transposed)
    w = torch.randn(*((K, N) if transposed else (N, K)), Rk, Rk, generator=g, dtype=F64)
    p = R.pack_panel(w, KP, NP, transposed).view(Rk * Rk, KP // 8, 2, NP, 4)
    for tap in range(Rk * Rk):
        ky, kx = tap // Rk, tap % Rk
        for kq in range(KP // 8):
            for half in range(2):
                for j in range(4):
                    k = kq * 8 + half * 4 + j
                    for n in range(NP):
                        want = 0.0 if (k >= K or n >= N) else float(w[k, n, ky, kx] if transposed else w[n, k, ky, kx])
                        assert float(p[tap, kq, half, n, j]) == want


def test_rowk_and_n2_layouts():
    g = gen(7, 3)
    w = torch.randn(5, 3, 7, 7, generator=g, dtype=F64)
    r = R.rowk_weight(w, 4, 32)
    for kx in range(7):
        for c in range(4):
            for ky in range(7):
                want = w[:, c, ky, kx] if c < 3 else torch.zeros(5, dtype=F64)
                assert torch.equal(r[:, kx * 4 + c, ky], want)
    assert float(r[:, 28:].abs().max()) == 0
    # a row-K panel convolves like the filter it came from: out = sum_ky sum_(kx, c) x[oy*s + ky - pad, run kx * cs + c] * r[n, kx * cs + c, ky]
    x = torch.randn(1, 9, 11, 4, generator=g, dtype=F64)
    ref = R.conv_nhwc(x[..., :3], w, None, 2, 1.0)
    xp = torch.zeros(1, 9 + 6, 11 + 6 + 1, 4, dtype=F64)
    xp[:, 3:12, 3:14] = x
    flat = xp.reshape(1, 15, -1)
    out = torch.zeros_like(ref)
    for oy in range(ref.shape[1]):
        for ox in range(ref.shape[2]):
            for ky in range(7):
                run = flat[0, oy * 2 + ky, ox * 2 * 4:ox * 2 * 4 + 32]
                out[0, oy, ox] += r[:, :, ky] @ run
    _close(out, ref)
    w2 = torch.randn(2, 19, 3, 3, generator=g, dtype=F64)
    q = R.n2_weight(w2, 8).view(9, 8, 2, 4)
    for t in range(9):
        for c in range(32):
            for o in range(2):
                assert float(q[t, c // 4, o, c % 4]) == (float(w2[o, c, t // 3, t % 3]) if c < 19 else 0.0)


def test_splitk_finish_restatement():
    g = gen(5)
    ks, M, Cout, CoutP = 3, 7, 5, 32
    ws = torch.randn(ks * M * CoutP + 9, generator=g)
    bias = torch.randn(Cout, generator=g)
    out = R.splitk_finish_f32(ws, ks, M, Cout, CoutP, bias, 0.1)
    assert out.dtype == torch.float32
    s = ws[:ks * M * CoutP].view(ks, M, CoutP).numpy()
    b = bias.numpy()
    for m in range(M):
        for c in range(Cout):
            v = np.float32(b[c])
            for k in range(ks):
                v = np.float32(v + s[k, m, c])
            v = v if v > 0 else np.float32(v * np.float32(0.1))
            assert out[m, c].item() == float(v)
    t = torch.from_numpy(s)
    assert torch.equal(R.splitk_finish_f32(ws, ks, M, Cout, CoutP, None, 1.0), ((0 + t[0, :, :Cout]) + t[1, :, :Cout]) + t[2, :, :Cout])


@pytest.mark.parametrize('H,W', [(9, 13), (1, 7), (5, 1)])
@pytest.mark.parametrize('BC', [1, 6])
def test_upsample4_restatement_vs_torch(BC, H, W):
    g = gen(BC, H, W)
    x = torch.randn(BC, H, W, generator=g, dtype=F64)
    for mode in (0, 1, 2):
        kw = {} if mode == 0 else {'align_corners': mode == 2}
        ref = F.interpolate(x[None], scale_factor=4, mode='nearest' if mode == 0 else 'bilinear', **kw)[0] * 20.0
        got = R.upsample4(x, mode, 20.0)
        if mode == 0:
            assert torch.equal(got, ref)
        else:
            _close(got, ref)
