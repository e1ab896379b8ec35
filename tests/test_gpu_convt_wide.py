"""64-wide N tiles of the fp32 transposed-conv family on the 128-pixel tiles (vv_conv_mfma VV_CONVT_FWD / VV_CONVT_DGRAD with
Cout % 64 == 0): the launch forced wide (VV_CONV_CONVT_WIDE) must leave the very bits of the same launch forced narrow
(VV_CONV_CONVT_NARROW) -- output, `stats` rows and bn_partial rows -- since every accumulator sees the same chunk -> tap -> k-pair
order and every row the same sums in the same order.  Through the C ABI with G = 2 groups of different data and a real group stride,
sentinel-filled outputs with slack, like tests/test_gpu_train_ops.py.

Shapes (H = input side of the transposed conv, K = GEMM-K channels, N = output channels of the launch, B images): one partial tile of
8 images and a ragged batch over two wide N tiles on the 4x4 level, an odd image count on the 2-image tiles of the 8x8 level, one
tile per half image at 16x16.  N = 96 has no wide form: the force-wide bit must give the narrow launch.  One forward and one data
gradient wide case are also held to the float64 restatement at the bar of tests/test_gpu_train_ops.py (2e-5), so the narrow form is
not the only witness.
"""
import ctypes as C

import pytest
import torch

import train_ops_restatement as R
from _util import SENT, away_from_zero as _away_from_zero, err as _err, gen as _gen

pytestmark = pytest.mark.gpu

G = 2


def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _pack(L, lib, w, mode, K, N):
    ent = (L.PackEntry * 1)(L.PackEntry(0, 0, mode, K, K, N))
    tab = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).cuda()
    out = torch.zeros(G, 9 * K * N + 16, device='cuda')
    L.check(lib.vv_pack_weights(tab.data_ptr(), 1, G, w.data_ptr(), w[0].numel(), out.data_ptr(), out.stride(0), 9 * K * N, _st()), 'pack')
    return out


# ================================================================================================ forward

def _fwd_inputs(H, K, N, B):
    g = _gen(H, K, N, B, 71)
    x = torch.randn(G, B * H * H, K, generator=g)
    wt = torch.randn(G, K, N, 3, 3, generator=g) * 0.1                        # nn.ConvTranspose2d layout per group
    bias = torch.randn(G, N, generator=g)
    a = torch.rand(G, K, generator=g) + 0.5
    b = torch.randn(G, K, generator=g) * 0.2
    return x, wt, bias, a, b


def _fwd_run(H, K, N, B, sliced, flag, ins):
    """the launch with pad0 = flag; returns the whole sentinel-filled buffer [G][B * 2H * 2H * cs + 64] on the host"""
    L, lib = _L()
    xd, wd, bd, ad, b_d = (t.cuda() for t in ins)
    pk = _pack(L, lib, wd, 2, K, N)
    cs, coff = (N + 64, 32) if sliced else (N, 0)
    y = torch.full((G, B * 4 * H * H * cs + 64), SENT, device='cuda')
    cp = L.ConvParams(L.CONVT_FWD, L.IN_ACT, G, B, H, H, K, K, N, L.view(xd, K, 0, xd.stride(0)), ad.data_ptr(), b_d.data_ptr(),
                      K, L.NULL_VIEW, 0, flag, None, pk.data_ptr(), pk.stride(0), bd.data_ptr(), N, L.view(y, cs, coff, y.stride(0)), None)
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'convT')
    return y.cpu(), cs, coff


@pytest.mark.parametrize('H,K,N,B,sliced', [(4, 16, 64, 3, False), (4, 32, 128, 9, False), (8, 16, 64, 3, False), (8, 16, 64, 3, True),
                                            (4, 16, 96, 3, False)])
def test_forward_wide_equals_narrow(H, K, N, B, sliced):
    """bit-equal buffers (sentinels round and beside the output included); N = 96: the wide bit falls back to the narrow launch"""
    L, _ = _L()
    ins = _fwd_inputs(H, K, N, B)
    yn, cs, coff = _fwd_run(H, K, N, B, sliced, L.CONV_CONVT_NARROW, ins)
    yw, _, _ = _fwd_run(H, K, N, B, sliced, L.CONV_CONVT_WIDE, ins)
    assert torch.equal(yw[:, -64:], torch.full((G, 64), SENT))
    v = yw[:, :-64].view(G, B, 2 * H, 2 * H, cs)
    assert not (v[..., coff:coff + N] == SENT).any()                          # every output element was written
    if sliced:
        assert torch.equal(v[..., :coff], torch.full_like(v[..., :coff], SENT))
        assert torch.equal(v[..., coff + N:], torch.full_like(v[..., coff + N:], SENT))
    assert torch.equal(yw, yn)


def test_forward_wide_float64():
    H, K, N, B = 4, 32, 128, 9
    L, _ = _L()
    x, wt, bias, a, b = ins = _fwd_inputs(H, K, N, B)
    y, _, _ = _fwd_run(H, K, N, B, False, L.CONV_CONVT_WIDE, ins)
    y = y[:, :-64].view(G, B, 2 * H, 2 * H, N)
    for gi in range(G):
        ref = R.convT_forward(R.act_in(x[gi].view(B, H, H, K).double(), a[gi].double(), b[gi].double()), wt[gi].double(), bias[gi].double())
        err = _err(y[gi], ref)
        print('convT forward, 64-wide: err', err)
        assert err <= 2e-5, (gi, err)


# ================================================================================================ data gradient

def _dgrad_inputs(H, K, N, B):
    """K = the transposed conv's output channels (GEMM-K of its data gradient), N = its input channels (the launch's output)"""
    g = _gen(H, K, N, B, 72)
    wt = torch.randn(G, N, K, 3, 3, generator=g) * 0.1
    dy = torch.randn(G, B * 4 * H * H, K, generator=g)
    a = torch.rand(G, N, generator=g) + 0.5
    b = torch.randn(G, N, generator=g) * 0.3
    mean = torch.randn(G, N, generator=g) * 0.1
    inv = torch.rand(G, N, generator=g) + 0.5
    z = _away_from_zero(torch.randn(G, B * H * H, N, generator=g), a[:, None], b[:, None])
    return wt, dy, a, b, mean, inv, z


def _dgrad_run(H, K, N, B, form, flag, ins):
    """form: 'plain', 'stats' or 'bn_partial'; returns (sentinel-filled output, rows or None, reported tiles) on the host"""
    L, lib = _L()
    wd, dyd, ad, bd, md, ivd, zd = (t.cuda() for t in ins)
    pk = _pack(L, lib, wd, 3, K, N)
    nt = lib.vv_convt_dgrad_ntiles(B, H, H, 0)
    assert nt > 0 and nt == lib.vv_conv_ntiles2(B, H, H, L.CONVT_DGRAD, 0)
    out = torch.full((G, B * H * H * N + 64), SENT, device='cuda')
    rows = torch.full((G * nt + 3, 2, N), SENT, device='cuda') if form != 'plain' else None      # dense [G][ntiles][2][N] + slack rows
    cp = L.ConvParams(L.CONVT_DGRAD, L.IN_PLAIN, G, B, H, H, K, K, N, L.view(dyd, K, 0, dyd.stride(0)), None, None, 0,
                      L.NULL_VIEW, 0, flag, None, pk.data_ptr(), pk.stride(0), None, 0, L.view(out, N, 0, out.stride(0)), None)
    if form == 'stats':
        cp.stats = rows.data_ptr()
    if form == 'bn_partial':
        cp.bn_z, cp.bn_z_gstride = zd.data_ptr(), zd.stride(0)
        cp.bn_a, cp.bn_b, cp.bn_mean, cp.bn_invstd, cp.bn_gstride = ad.data_ptr(), bd.data_ptr(), md.data_ptr(), ivd.data_ptr(), N
        cp.bn_partial = rows.data_ptr()
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'dgradT ' + form)
    return out.cpu(), (rows.cpu() if rows is not None else None), nt


@pytest.mark.parametrize('form', ['plain', 'stats', 'bn_partial'])
@pytest.mark.parametrize('H,K,N,B', [(16, 16, 64, 2), (8, 16, 64, 3), (4, 16, 128, 9), (8, 16, 96, 3)])
def test_data_gradient_wide_equals_narrow(H, K, N, B, form):
    """output and rows bit-equal; the rows behind vv_convt_dgrad_ntiles keep the sentinel.  N = 96: fallback to the narrow launch"""
    L, _ = _L()
    ins = _dgrad_inputs(H, K, N, B)
    on, rn, nt = _dgrad_run(H, K, N, B, form, L.CONV_CONVT_NARROW, ins)
    ow, rw, _ = _dgrad_run(H, K, N, B, form, L.CONV_CONVT_WIDE, ins)
    assert torch.equal(ow[:, -64:], torch.full((G, 64), SENT))
    assert not (ow[:, :-64] == SENT).any()
    assert torch.equal(ow, on)
    if form != 'plain':
        assert torch.equal(rw[G * nt:], torch.full_like(rw[G * nt:], SENT))
        assert not (rw[:G * nt] == SENT).any()
        assert torch.equal(rw, rn)


def test_data_gradient_wide_float64():
    H, K, N, B = 4, 16, 128, 9
    L, _ = _L()
    ins = _dgrad_inputs(H, K, N, B)
    wt, dy = ins[0], ins[1]
    out, _, _ = _dgrad_run(H, K, N, B, 'bn_partial', L.CONV_CONVT_WIDE, ins)
    for gi in range(G):
        ref = R.convT_data_gradient(dy[gi].view(B, 2 * H, 2 * H, K).double(), wt[gi].double())
        err = _err(out[gi, :-64].view(B, H, H, N), ref)
        print('convT data gradient, 64-wide: err', err)
        assert err <= 2e-5, (gi, err)
