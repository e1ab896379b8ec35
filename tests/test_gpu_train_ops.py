"""Kernel-level parity of what an fp32 train step launches besides its 3x3 convolutions (tests/test_gpu_unet.py) and the 1x1 output
conv (tests/test_gpu_outconv.py): the fp32
transposed-conv family (vv_conv_mfma VV_CONVT_FWD / VV_CONVT_DGRAD, vv_wgrad_mfma + vv_wgrad_reduce with kind = VV_CONVT_FWD), BatchNorm
(vv_bn_finalize, vv_bn_bwd_reduce + vv_bn_bwd_apply, vv_bn_bwd_sums), the reductions, adapters and layout copies of vv_elem.hip and the
optimiser (vv_adam_tick + vv_adam_bucketed, vv_adam) -- each through the C ABI with G = 2 groups of different data (a wrong *_gstride
shows) against the float64 restatement of its own operation (tests/train_ops_restatement.py, checked against torch autograd by
tests/test_train_ops_host.py).  Shapes are the smallest that reach every instantiation and every ragged edge.

Bars:
  * exact (bit-equal) where the arithmetic is exact: gather, erase, layout copies, counter, refused calls, eval-mode running buffers,
    sentinels round every output; vv_pool_act fp32 within one float ulp of the rounded float64 value (fmaf + max; double rounding);
  * transposed-conv forward / data gradient 2e-5, weight gradient 5e-5 of the float64 reference's maximum -- the bars every fp32
    convolution of the project is held to (tests/test_flownet2.py, test_winograd_conv_matches_direct_conv,
    test_winograd_weight_gradient_matches_direct);
  * everything else that sums in float (`_bar`): with err = max |x - ref64| / max |ref64|, err_hip of the kernel against err_ref32 of the
    SAME restatement evaluated by torch on the CPU in float32 on the same inputs: err_hip <= max(8 err_ref32, 16 * 2^-23).  The measure
    is the reference arithmetic, never the kernel; the worst figures per operation are recorded in docs/train_ops_parity.md.
  * vv_bn_finalize accumulates in fp64 (include/vecvad_hip.h), and with partial sums at mean 50 / std 1 the float32 evaluation of
    E[x^2] - mean^2 loses three digits, so the rule above is loose there: the fp64 promise is held directly as well, every output
    within 16 * 2^-23 of the float64 restatement (fp32 inputs are exact in fp64; one rounding to float on the way out).

Gates decide discontinuously: inputs are nudged until no |a y + b| is below 1e-3 and the two largest activations of a pooling window
differ by at least 1e-3 (unless tied on purpose), asserted in the test; no element is left out of any comparison.

The 32x32 transposed-conv forward is supported by dispatch<> but unused by the bank; it is tested as any other level.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_ops_restatement as R
from _util import FLOOR, SENT, away_from_zero as _away_from_zero, bar as _bar, err as _err, gen as _gen, observe

pytestmark = pytest.mark.gpu

G = 2
F64 = torch.float64
CONVT_SHAPES = [(16, 64, 32, 3), (8, 128, 64, 5), (8, 64, 32, 4), (4, 256, 128, 17), (4, 128, 64, 8)]


def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _f64(*ts):
    return [t.cpu().double() if t is not None else None for t in ts]


def _pack(L, lib, w, mode, K, N):
    ent = (L.PackEntry * 1)(L.PackEntry(0, 0, mode, K, K, N))
    tab = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).cuda()
    out = torch.zeros(G, 9 * K * N + 16, device='cuda')
    L.check(lib.vv_pack_weights(tab.data_ptr(), 1, G, w.data_ptr(), w[0].numel(), out.data_ptr(), out.stride(0), 9 * K * N, _st()), 'pack')
    return out


# ================================================================================================ transposed conv, fp32

def _convT_inputs(H, Cin, Cout, B, salt):
    g = _gen(H, Cin, Cout, B, salt)
    x = torch.randn(G, B * H * H, Cin, generator=g)
    wt = torch.randn(G, Cin, Cout, 3, 3, generator=g) * 0.1                   # nn.ConvTranspose2d layout per group
    bias = torch.randn(G, Cout, generator=g)
    a = torch.rand(G, Cin, generator=g) + 0.5
    b = torch.randn(G, Cin, generator=g) * 0.2
    dy = torch.randn(G, B * 4 * H * H, Cout, generator=g)
    return x, wt, bias, a, b, dy


@pytest.mark.parametrize('H,Cin,Cout,B,sliced', [s + (False,) for s in CONVT_SHAPES] + [(32, 16, 32, 1, False)] +
                         [(16, 64, 32, 3, True), (8, 64, 32, 4, True), (4, 128, 64, 8, True)])
def test_transposed_conv_forward_fp32(H, Cin, Cout, B, sliced):
    """ConvTranspose2d(k3, s2, p1, op1) of relu(a x + b), all four output phases, odd and exact multiples of the images per tile; sliced:
    into channels [32, 32 + Cout) of a wider buffer (the upsampled half of a concat buffer), whose other channels must stay."""
    L, lib = _L()
    x, wt, bias, a, b, _ = _convT_inputs(H, Cin, Cout, B, 1)
    xd, wd, bd, ad, b_d = (t.cuda() for t in (x, wt, bias, a, b))
    pk = _pack(L, lib, wd, 2, Cin, Cout)
    cs, coff = (Cout + 64, 32) if sliced else (Cout, 0)
    y = torch.full((G, B * 4 * H * H * cs + 64), SENT, device='cuda')
    cp = L.ConvParams(L.CONVT_FWD, L.IN_ACT, G, B, H, H, Cin, Cin, Cout, L.view(xd, Cin, 0, xd.stride(0)), ad.data_ptr(), b_d.data_ptr(),
                      Cin, L.NULL_VIEW, 0, 0, None, pk.data_ptr(), pk.stride(0), bd.data_ptr(), Cout, L.view(y, cs, coff, y.stride(0)), None)
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'convT')
    y = y.cpu()
    assert torch.equal(y[:, -64:], torch.full((G, 64), SENT))
    y = y[:, :-64].view(G, B, 2 * H, 2 * H, cs)
    if sliced:
        assert torch.equal(y[..., :coff], torch.full_like(y[..., :coff], SENT))
        assert torch.equal(y[..., coff + Cout:], torch.full_like(y[..., coff + Cout:], SENT))
    for gi in range(G):
        x64, w64, b64, a64, bb64 = _f64(x[gi].view(B, H, H, Cin), wt[gi], bias[gi], a[gi], b[gi])
        ref = R.convT_forward(R.act_in(x64, a64, bb64), w64, b64)
        err = _err(y[gi, ..., coff:coff + Cout], ref)
        observe('train_ops:convT_fwd', err_hip=err)
        assert err <= 2e-5, (gi, err)


def _dgrad_params(L, dyd, pk, out, H, Cin, Cout, B):
    return L.ConvParams(L.CONVT_DGRAD, L.IN_PLAIN, G, B, H, H, Cout, Cout, Cin, L.view(dyd, Cout, 0, dyd.stride(0)), None, None, 0,
                        L.NULL_VIEW, 0, 0, None, pk.data_ptr(), pk.stride(0), None, 0, L.view(out, Cin, 0, out.stride(0)), None)


@pytest.mark.parametrize('H,Cin,Cout,B', CONVT_SHAPES)
def test_transposed_conv_data_gradient_fp32(H, Cin, Cout, B):
    """the stride-2 gather over the 2H x 2W output gradient (128-pixel tiles on all three levels)"""
    L, lib = _L()
    _, wt, _, _, _, dy = _convT_inputs(H, Cin, Cout, B, 2)
    dyd, wd = dy.cuda(), wt.cuda()
    pk = _pack(L, lib, wd, 3, Cout, Cin)
    out = torch.full((G, B * H * H * Cin + 64), SENT, device='cuda')
    cp = _dgrad_params(L, dyd, pk, out, H, Cin, Cout, B)
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'dgradT')
    out = out.cpu()
    assert torch.equal(out[:, -64:], torch.full((G, 64), SENT))
    for gi in range(G):
        ref = R.convT_data_gradient(dy[gi].view(B, 2 * H, 2 * H, Cout).double(), wt[gi].double())
        err = _err(out[gi, :-64].view(B, H, H, Cin), ref)
        observe('train_ops:convT_dgrad', err_hip=err)
        assert err <= 2e-5, (gi, err)


@pytest.mark.parametrize('H,Cin,Cout,B', [(16, 64, 32, 3), (8, 128, 64, 5), (4, 256, 128, 17)])
def test_transposed_conv_data_gradient_stats_rows(H, Cin, Cout, B):
    """a `stats` launch of the fp32 stride-2 gather: vv_conv_ntiles2 reports the rows the launch writes -- those rows add up to the column
    sums / sums of squares of the stored output, the rows behind them keep the sentinel.  The buffer is sized by the larger of
    vv_conv_ntiles2 and vv_convt_dgrad_ntiles (the 128-pixel tiles dispatch<> launches) plus slack, so a wrong count cannot overrun."""
    L, lib = _L()
    _, wt, _, _, _, dy = _convT_inputs(H, Cin, Cout, B, 3)
    dyd, wd = dy.cuda(), wt.cuda()
    pk = _pack(L, lib, wd, 3, Cout, Cin)
    nt = lib.vv_conv_ntiles2(B, H, H, L.CONVT_DGRAD, 0)
    rows = G * max(nt, lib.vv_convt_dgrad_ntiles(B, H, H, 0)) + 3          # (`stats` is dense: [G][ntiles][2][Cout], no group stride)
    assert nt > 0
    out = torch.zeros(G, B * H * H * Cin, device='cuda')
    stats = torch.full((rows, 2, Cin), SENT, device='cuda')
    cp = _dgrad_params(L, dyd, pk, out, H, Cin, Cout, B)
    cp.stats = stats.data_ptr()
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'dgradT+stats')
    out, stats = out.cpu().view(G, -1, Cin), stats.cpu()
    assert torch.equal(stats[G * nt:], torch.full_like(stats[G * nt:], SENT))          # nothing behind the reported rows
    tot = stats[:G * nt].view(G, nt, 2, Cin).double().sum(1)
    for gi in range(G):
        # the stored gradient against the restatement (the convolution bar), then the rows against the sums of what was stored: the
        # header defines `stats` as sums over the OUTPUT, and this way the summation is measured apart from the convolution's round-off
        ref = R.convT_data_gradient(dy[gi].view(B, 2 * H, 2 * H, Cout).double(), wt[gi].double())
        err = _err(out[gi].view(B, H, H, Cin), ref)
        observe('train_ops:convT_dgrad', err_hip=err)
        assert err <= 2e-5, (gi, err)
        _bar('convT_dgrad_stats', 'sum', tot[gi, 0], out[gi].double().sum(0), out[gi].sum(0))
        _bar('convT_dgrad_stats', 'sumsq', tot[gi, 1], (out[gi].double() ** 2).sum(0), (out[gi] ** 2).sum(0))


@pytest.mark.parametrize('bf16', [False, True])
def test_transposed_conv_forward_refuses_stats(bf16):
    """VV_CONVT_FWD keeps no column sums (its four-phase store loop never accumulates them): stats != NULL is VV_ERR_UNSUPPORTED, fp32
    and bf16, and nothing is launched"""
    L, lib = _L()
    H, Cin, Cout, B = 8, 64, 32, 2
    x, wt, bias, a, b, _ = _convT_inputs(H, Cin, Cout, B, 4)
    xd, wd, bd, ad, b_d = (t.cuda() for t in (x, wt, bias, a, b))
    pk = _pack(L, lib, wd, 2 | (L.PACK_BF16 if bf16 else 0), Cin, Cout)
    y = torch.full((G, B * 4 * H * H * Cout), SENT, device='cuda')
    stats = torch.full((G, 2 * B + 8, 2, Cout), SENT, device='cuda')           # (more rows than any tiling of this launch has)
    cp = L.ConvParams(L.CONVT_FWD, L.IN_ACT, G, B, H, H, Cin, Cin, Cout, L.view(xd, Cin, 0, xd.stride(0)), ad.data_ptr(), b_d.data_ptr(),
                      Cin, L.NULL_VIEW, 0, L.CONV_BF16 if bf16 else 0, None, pk.data_ptr(), pk.stride(0), bd.data_ptr(), Cout,
                      L.view(y, Cout, 0, y.stride(0)), stats.data_ptr())
    assert lib.vv_conv_mfma(C.byref(cp), _st()) == 3            # VV_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.full(y.shape, SENT)) and torch.equal(stats.cpu(), torch.full(stats.shape, SENT))
    cp.stats = None
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'convT')                     # the same launch without stats runs
    assert not torch.equal(y.cpu(), torch.full(y.shape, SENT))


@pytest.mark.parametrize('H,Cin,Cout,B', [(16, 64, 32, 3), (8, 128, 64, 5), (4, 256, 128, 17)])
def test_transposed_conv_data_gradient_bn_partial(H, Cin, Cout, B):
    """the bn_partial epilogue (S16 == 4): the gradient itself, and the rows (vv_convt_dgrad_ntiles of them) add up to sum dz and
    sum dz xhat, dz = dA [a z + b > 0], of the BatchNorm in front of the transposed conv"""
    L, lib = _L()
    _, wt, _, _, _, dy = _convT_inputs(H, Cin, Cout, B, 5)
    g = _gen(H, Cin, Cout, B, 55)
    a = torch.rand(G, Cin, generator=g) + 0.5
    b = torch.randn(G, Cin, generator=g) * 0.3
    mean = torch.randn(G, Cin, generator=g) * 0.1
    inv = torch.rand(G, Cin, generator=g) + 0.5
    z = _away_from_zero(torch.randn(G, B * H * H, Cin, generator=g), a[:, None], b[:, None])
    dyd, wd, zd, ad, bd, md, ivd = (t.cuda() for t in (dy, wt, z, a, b, mean, inv))
    pk = _pack(L, lib, wd, 3, Cout, Cin)
    nt = lib.vv_convt_dgrad_ntiles(B, H, H, 0)
    out = torch.full((G, B * H * H * Cin + 64), SENT, device='cuda')
    part = torch.full((G * nt + 3, 2, Cin), SENT, device='cuda')          # dense [G][ntiles][2][Cout] + slack rows
    cp = _dgrad_params(L, dyd, pk, out, H, Cin, Cout, B)
    cp.bn_z, cp.bn_z_gstride = zd.data_ptr(), zd.stride(0)
    cp.bn_a, cp.bn_b, cp.bn_mean, cp.bn_invstd, cp.bn_gstride = ad.data_ptr(), bd.data_ptr(), md.data_ptr(), ivd.data_ptr(), Cin
    cp.bn_partial = part.data_ptr()
    L.check(lib.vv_conv_mfma(C.byref(cp), _st()), 'dgradT+bn_partial')
    out, part = out.cpu(), part.cpu()
    assert torch.equal(out[:, -64:], torch.full((G, 64), SENT))
    assert torch.equal(part[G * nt:], torch.full_like(part[G * nt:], SENT))
    tot = part[:G * nt].view(G, nt, 2, Cin).double().sum(1)

    def sums(dyg, wg, zg, ag, bg, mg, ig):
        dA = R.convT_data_gradient(dyg.view(B, 2 * H, 2 * H, Cout), wg)
        _, dgamma, dbeta, _ = R.bn_relu_pool_backward(zg.view(B, H, H, Cin), ag, bg, mg, ig, torch.ones_like(ag), dA)
        return dA, dbeta, dgamma

    for gi in range(G):
        args = (dy[gi], wt[gi], z[gi], a[gi], b[gi], mean[gi], inv[gi])
        dA, s1, s2 = sums(*_f64(*args))
        _, s1f, s2f = sums(*args)
        err = _err(out[gi, :-64].view(B, H, H, Cin), dA)
        observe('train_ops:convT_dgrad', err_hip=err)
        assert err <= 2e-5, (gi, err)
        _bar('convT_dgrad_bn_partial', 'sum dz', tot[gi, 0], s1, s1f)
        _bar('convT_dgrad_bn_partial', 'sum dz xhat', tot[gi, 1], s2, s2f)


def _wgradT_case(H, Cin, Cout, B, ksel):
    L, lib = _L()
    x, _, _, a, b, dy = _convT_inputs(H, Cin, Cout, B, 6)
    xd, dyd, ad, bd = (t.cuda() for t in (x, dy, a, b))
    nt = lib.vv_wgrad_ntiles(L.CONVT_FWD, B, H, H)
    assert nt > 0
    ks = {'one': 1, 'three': 3, 'over': nt + 1}[ksel]
    nci, nco = Cin // 32, Cout // 32
    part = torch.full((G, nci * nco * ks * 9 * 1024 + 64), 7.0, device='cuda')
    grad = torch.full((G, Cin * Cout * 9 + 64), SENT, device='cuda')
    wp = L.WgradParams(L.CONVT_FWD, L.IN_ACT, G, B, H, H, Cin, Cin, Cout, ks, L.view(xd, Cin, 0, xd.stride(0)), ad.data_ptr(), bd.data_ptr(),
                       Cin, L.NULL_VIEW, 0, 0, None, L.View(dyd.data_ptr(), dyd.stride(0), Cout, 0), part.data_ptr(), part.stride(0))
    L.check(lib.vv_wgrad_mfma(C.byref(wp), _st()), 'wgradT')
    L.check(lib.vv_wgrad_reduce(L.CONVT_FWD, G, Cin, Cin, Cout, ks, part.data_ptr(), part.stride(0), grad.data_ptr(), grad.stride(0), _st()),
            'reduce')
    grad, part = grad.cpu(), part.cpu()
    assert torch.equal(grad[:, -64:], torch.full((G, 64), SENT)) and torch.equal(part[:, -64:], torch.full((G, 64), 7.0))
    if ks > nt:                                                      # the workgroup without a tile left a slab of zeros, not the fill
        slabs = part[:, :-64].view(G, nci * nco, ks, 9 * 1024)
        assert (slabs.abs().amax(-1) == 0).sum().item() >= G * nci * nco
        assert not (slabs == 7.0).any()
    worst = 0.0
    for gi in range(G):
        act = R.act_in(x[gi].view(B, H, H, Cin).double(), a[gi].double(), b[gi].double())
        ref = R.convT_weight_gradient(act, dy[gi].view(B, 2 * H, 2 * H, Cout).double())
        worst = max(worst, _err(grad[gi, :-64].view(Cin, Cout, 3, 3), ref))          # every entry
    return worst


@pytest.mark.parametrize('ksel', ['one', 'three', 'over'])
@pytest.mark.parametrize('H,Cin,Cout,B', CONVT_SHAPES)
def test_transposed_conv_weight_gradient_fp32(H, Cin, Cout, B, ksel):
    """vv_wgrad_mfma + vv_wgrad_reduce, kind = VV_CONVT_FWD, into the nn.ConvTranspose2d layout [Cin][Cout][3][3]; k-split 1, 3 and one
    more than there are pixel tiles.  These run the 64-pixel tiles (the first launch_w<.., VV_CONVT_FWD> group, the default)."""
    err = _wgradT_case(H, Cin, Cout, B, ksel)
    observe('train_ops:convT_wgrad', err_hip=err)
    assert err <= 5e-5, err


def test_transposed_conv_weight_gradient_fp32_128_pixel_tiles():
    """the second launch_w<.., VV_CONVT_FWD> group (128-pixel tiles, one LDS buffer) is chosen by VV_WGRADT_TILE64=0, which the library
    reads once per process: the same five shapes (k-split 3) in a child process -- the only way to reach that group"""
    env = dict(os.environ, VV_WGRADT_TILE64='0')
    code = ('import sys; sys.path[:0] = %r; import test_gpu_train_ops as T\n'
            'for s in T.CONVT_SHAPES:\n'
            '    e = T._wgradT_case(*s, "three"); print("ERR", s, e); assert e <= 5e-5, (s, e)\n' % [os.path.dirname(__file__), os.path.dirname(os.path.dirname(__file__))])
    r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and r.stdout.count('ERR') == len(CONVT_SHAPES)


# ================================================================================================ BatchNorm

@pytest.mark.parametrize('ntiles', [1, 31, 33, 129, 300])
@pytest.mark.parametrize('C_', [32, 48, 256, 512])
def test_bn_finalize(C_, ntiles):
    """train (count = the pixel count, and count = 1) and eval mode; partial sums of 8 pixels per tile at mean 50 / std 1"""
    L, lib = _L()
    g = _gen(C_, ntiles, 7)
    P, CP = 8, C_ + 16                                           # group strides wider than the rows
    MOM, EPSBN = float(np.float32(0.1)), float(np.float32(1e-5))      # the float arguments as the kernel receives them
    xs = torch.randn(G, ntiles, P, C_, generator=g, dtype=F64) + 50.0
    stats = torch.stack([xs.sum(2), (xs * xs).sum(2)], 2).float()             # [G, ntiles, 2, C]
    par = [torch.rand(G, CP, generator=g) + 0.5, torch.randn(G, CP, generator=g), torch.randn(G, CP, generator=g) * 3 + 40,
           torch.rand(G, CP, generator=g) + 0.5]                               # gamma, beta, running_mean, running_var
    sd = torch.cat([stats.reshape(G, -1), torch.full((G, 32), SENT)], 1).cuda()
    cases = [('train', 1, ntiles * P), ('eval', 0, ntiles * P)] + ([('count1', 1, 1)] if ntiles == 1 else [])
    for name, train, count in cases:
        gm, bt, rm, rv = (t.clone().cuda() for t in par)
        outs = [torch.full((G, CP), SENT, device='cuda') for _ in range(4)]
        L.check(lib.vv_bn_finalize(G, C_, ntiles, count, train, 0.1, 1e-5, sd.data_ptr(), sd.stride(0), gm.data_ptr(), bt.data_ptr(), CP,
                                   rm.data_ptr(), rv.data_ptr(), CP, *(o.data_ptr() for o in outs), CP, _st()), 'bn_finalize')
        outs, rm, rv = [o.cpu() for o in outs], rm.cpu(), rv.cpu()
        for t in outs:
            assert torch.equal(t[:, C_:], torch.full((G, CP - C_), SENT))
        assert torch.equal(rm[:, C_:], par[2][:, C_:]) and torch.equal(rv[:, C_:], par[3][:, C_:])
        if not train:                                            # eval mode leaves the running buffers alone, bit for bit
            assert torch.equal(rm, par[2]) and torch.equal(rv, par[3])
        for gi in range(G):
            args = (stats[gi], count, par[0][gi, :C_], par[1][gi, :C_], par[2][gi, :C_], par[3][gi, :C_], MOM, EPSBN, bool(train))
            ref64 = R.bn_finalize(*[t.double() if torch.is_tensor(t) else t for t in args])
            ref32 = R.bn_finalize(*args)
            got = [o[gi, :C_] for o in outs] + [rm[gi, :C_], rv[gi, :C_]]
            for what, x, r64, r32 in zip(('a', 'b', 'mean', 'invstd', 'running_mean', 'running_var'), got, ref64, ref32):
                _bar('bn_finalize', (name, what), x, r64, r32)
                assert _err(x, r64) <= FLOOR, (name, what, _err(x, r64))          # the fp64 accumulation the header promises


def _bn_bwd_inputs(H, C_, B, pool, ties, seed):
    """y with every |a y + b| >= 1e-3; pooled: the two largest activations of a window >= 1e-3 apart, except the windows tied on purpose
    (ties: in a tenth of them the maximum's value is copied over its horizontal neighbour -- an exact positive tie)"""
    g = _gen(H, C_, B, seed)
    M = B * H * H
    a = torch.rand(G, 1, C_, generator=g) + 0.5
    b = torch.randn(G, 1, C_, generator=g) * 0.3
    y = _away_from_zero(torch.randn(G, M, C_, generator=g), a, b)
    if pool:
        def windows(t):      # [G, M, C] -> [G, B, H2, W2, C, 4], window-internal row-major order
            return t.view(G, B, H // 2, 2, H // 2, 2, C_).permute(0, 1, 2, 4, 6, 3, 5).reshape(G, B, H // 2, H // 2, C_, 4)

        def unwindows(w):
            return w.view(G, B, H // 2, H // 2, C_, 2, 2).permute(0, 1, 2, 5, 3, 6, 4).reshape(G, M, C_)

        a6, b6 = a.double().view(G, 1, 1, 1, C_, 1), b.double().view(G, 1, 1, 1, C_, 1)
        yw = windows(y).clone()
        act = torch.relu(a6 * yw.double() + b6)
        top2 = act.topk(2, -1).values
        first = R.pool_first_max(unwindows(act).view(G * B, H, H, C_)).view(G, B, H // 2, H // 2, C_, 1)
        close = (top2[..., :1] - top2[..., 1:]) < 4e-3
        lifted = ((top2[..., :1] + 1e-2 - b6) / a6).float()          # the first maximum of such a window, lifted clear of the others
        yw.scatter_(-1, first, torch.where(close, lifted, yw.gather(-1, first)))
        tied = torch.zeros_like(close)
        if ties:
            tied = torch.rand(close.shape, generator=g) < 0.1
            yw.scatter_(-1, first ^ 1, torch.where(tied, yw.gather(-1, first), yw.gather(-1, first ^ 1)))
        y = unwindows(yw).contiguous()
        v = torch.relu(a6 * windows(y).double() + b6).sort(-1, descending=True).values
        ok = torch.where(tied, (v[..., :1] == v[..., 1:2]) & (v[..., :1] > 0) & (v[..., :1] - v[..., 2:3] >= 1e-3), v[..., :1] - v[..., 1:2] >= 1e-3)
        assert ok.all()
        assert (a.double() * y.double() + b.double()).abs().min().item() >= 1e-3
    mean = torch.randn(G, C_, generator=g) * 0.1
    inv = torch.rand(G, C_, generator=g) + 0.5
    gamma = torch.rand(G, C_, generator=g) + 0.5
    dP = torch.randn(G, M // 4, C_, generator=g) if pool else None
    return y, a.view(G, C_).contiguous(), b.view(G, C_).contiguous(), mean, inv, gamma, dP, g


def _bn_bwd_run(H, C_, B, pool, slice_, ties=False):
    L, lib = _L()
    y, a, b, mean, inv, gamma, dP, g = _bn_bwd_inputs(H, C_, B, pool, ties, 8 + 2 * pool + slice_)
    M = B * H * H
    cs, off = (C_ + 32, 16) if slice_ else (C_, 0)
    dAw = torch.randn(G, M, cs, generator=g)
    dA = dAw[:, :, off:off + C_]
    yd, ad, bd, md, ivd, gmd, dAd = (t.cuda() for t in (y, a, b, mean, inv, gamma, dAw))
    dPd = dP.cuda() if pool else None
    nblk = lib.vv_bn_bwd_nblk(B, H, H, C_)
    part = torch.full((1, G * nblk * 2 * C_ + 64), SENT, device='cuda')          # dense [G][nblk][2][C], no group stride
    dz = torch.full((G, M * C_ + 64), SENT, device='cuda')
    dgm, dbt = torch.full((G, C_ + 8), SENT, device='cuda'), torch.full((G, C_ + 8), SENT, device='cuda')
    scr = torch.zeros(G, 2 * C_, device='cuda')
    bp = L.BnBwdParams(G, B, H, H, C_, 0, yd.data_ptr(), yd.stride(0), ad.data_ptr(), bd.data_ptr(), md.data_ptr(), ivd.data_ptr(), C_,
                       L.view(dAd, cs, off, dAd.stride(0)), dPd.data_ptr() if pool else None, dPd.stride(0) if pool else 0,
                       dz.data_ptr(), dz.stride(0), part.data_ptr())
    L.check(lib.vv_bn_bwd_reduce(C.byref(bp), _st()), 'reduce')
    L.check(lib.vv_bn_bwd_apply(C.byref(bp), gmd.data_ptr(), C_, dgm.data_ptr(), dbt.data_ptr(), C_ + 8, scr.data_ptr(), _st()), 'apply')
    dev = (yd, ad, bd, md, ivd, gmd, dAd, dPd, dz, part)          # (kept alive: bp points into them)
    dz, dgm, dbt, part = dz.cpu(), dgm.cpu(), dbt.cpu(), part.cpu()
    for t, w in ((dz, 64), (part, 64), (dgm, 8), (dbt, 8)):
        assert torch.equal(t[:, -w:], torch.full((t.shape[0], w), SENT))
    op = 'bn_bwd_pool' if pool else 'bn_bwd'
    for gi in range(G):
        args = (y[gi].view(B, H, H, C_), a[gi], b[gi], mean[gi], inv[gi], gamma[gi], dA[gi].reshape(B, H, H, C_),
                dP[gi].view(B, H // 2, H // 2, C_) if pool else None)
        r64 = R.bn_relu_pool_backward(*_f64(*args))
        r32 = R.bn_relu_pool_backward(*args)
        _bar(op, 'dy', dz[gi, :-64].view(B, H, H, C_), r64[0], r32[0])
        _bar(op, 'dgamma', dgm[gi, :C_], r64[1], r32[1])
        _bar(op, 'dbeta', dbt[gi, :C_], r64[2], r32[2])
    return (L, lib, bp, dev), (y, a, b, mean, inv, gamma, dA)


@pytest.mark.parametrize('variant', ['plain', 'pool', 'plain_slice', 'pool_slice'])
@pytest.mark.parametrize('H,C_,B', [(32, 32, 3), (16, 64, 5), (8, 128, 9), (4, 256, 33), (4, 512, 3)])
def test_bn_backward(H, C_, B, variant):
    """vv_bn_bwd_reduce + vv_bn_bwd_apply on fp32 tensors: d gamma, d beta, dy; with and without the MaxPool2d(2) fan-in (dpool at half
    resolution), dA dense or a channel slice of a wider tensor"""
    _bn_bwd_run(H, C_, B, variant.startswith('pool'), variant.endswith('slice'))


def test_bn_backward_pool_exact_ties():
    """the first maximum of a window in row-major order takes the pooled gradient (at::max_pool2d): a tenth of the windows hold their
    positive maximum twice"""
    _bn_bwd_run(16, 64, 5, True, False, ties=True)


@pytest.mark.parametrize('H,C_,B,slice_', [(32, 32, 3, False), (16, 64, 5, True), (4, 512, 3, False)])
def test_bn_backward_sums_table(H, C_, B, slice_):
    """vv_bn_bwd_sums after vv_bn_bwd_reduce: rows a, b, mean, invstd are copies of the inputs; gk = gamma invstd, c1 = mean(dz),
    c2 = mean(dz xhat) against float64; d gamma / d beta as from vv_bn_bwd_apply"""
    (L, lib, bp, dev), (y, a, b, mean, inv, gamma, dA) = _bn_bwd_run(H, C_, B, False, slice_)
    TG = L.BNBWD_TAB_ROWS * C_ + 32
    tab = torch.full((G, TG), SENT, device='cuda')
    dgm, dbt = torch.zeros(G, C_, device='cuda'), torch.zeros(G, C_, device='cuda')
    L.check(lib.vv_bn_bwd_sums(C.byref(bp), dev[5].data_ptr(), C_, dgm.data_ptr(), dbt.data_ptr(), C_, tab.data_ptr(), TG, _st()), 'sums')
    tab = tab.cpu()
    assert torch.equal(tab[:, -32:], torch.full((G, 32), SENT))
    rows = tab[:, :-32].view(G, L.BNBWD_TAB_ROWS, C_)
    for k, src in enumerate((a, b, mean, inv)):
        assert torch.equal(rows[:, k], src)
    M = B * H * H
    for gi in range(G):
        args = (y[gi].view(B, H, H, C_), a[gi], b[gi], mean[gi], inv[gi], gamma[gi], dA[gi].reshape(B, H, H, C_))
        r64 = R.bn_relu_pool_backward(*_f64(*args))
        r32 = R.bn_relu_pool_backward(*args)
        _bar('bn_bwd_sums', 'gk', rows[gi, 4], gamma[gi].double() * inv[gi].double(), gamma[gi] * inv[gi])
        _bar('bn_bwd_sums', 'c1', rows[gi, 5], r64[2] / M, r32[2] / M)
        _bar('bn_bwd_sums', 'c2', rows[gi, 6], r64[1] / M, r32[1] / M)
        _bar('bn_bwd_sums', 'dgamma', dgm[gi], r64[1], r32[1])
        _bar('bn_bwd_sums', 'dbeta', dbt[gi], r64[2], r32[2])


# ================================================================================================ reductions and elementwise

@pytest.mark.parametrize('C_', [32, 64, 256])
@pytest.mark.parametrize('M', [1, 1023, 1024, 1025, 5000])
def test_bias_grad(M, C_):
    """db[c] = sum over pixels of dy[p][32 + c], dy a channel slice of a wider tensor; one block, the block edge, several blocks"""
    L, lib = _L()
    g = _gen(M, C_, 9)
    cs, coff = C_ + 64, 32
    dy = torch.randn(G, M, cs, generator=g) + 0.25
    dyd = dy.cuda()
    nblk = (M + 1023) // 1024
    scr = torch.full((G, nblk * C_ + 32), SENT, device='cuda')
    db = torch.full((G, C_ + 8), SENT, device='cuda')
    L.check(lib.vv_bias_grad(G, M, C_, dyd.data_ptr(), dyd.stride(0), cs, coff, scr.data_ptr(), db.data_ptr(), C_ + 8, _st()), 'bias_grad')
    db = db.cpu()
    assert torch.equal(db[:, C_:], torch.full((G, 8), SENT))
    for gi in range(G):
        sl = dy[gi, :, coff:coff + C_]
        _bar('bias_grad', (M, C_), db[gi, :C_], sl.double().sum(0), sl.sum(0))


@pytest.mark.parametrize('coff', [0, 32])
@pytest.mark.parametrize('n', [32, 40])
@pytest.mark.parametrize('ntiles', [1, 33, 130])
def test_bias_from_partials(ntiles, n, coff):
    """db[j] = sum over tiles of partial[tile][0][coff + j] (slot 1, the sums of squares, must not leak in)"""
    L, lib = _L()
    g = _gen(ntiles, n, coff, 10)
    C_ = 96
    part = torch.randn(G, ntiles, 2, C_, generator=g) + 0.5
    part[:, :, 1] += 100.0
    pd = torch.cat([part.reshape(G, -1), torch.full((G, 32), SENT)], 1).cuda()
    db = torch.full((G, n + 8), SENT, device='cuda')
    L.check(lib.vv_bias_from_partials(G, C_, ntiles, coff, n, pd.data_ptr(), pd.stride(0), db.data_ptr(), n + 8, _st()), 'bias_from_partials')
    db = db.cpu()
    assert torch.equal(db[:, n:], torch.full((G, 8), SENT))
    for gi in range(G):
        sl = part[gi, :, 0, coff:coff + n]
        _bar('bias_from_partials', (ntiles, n, coff), db[gi, :n], sl.double().sum(0), sl.sum(0))


def _bf16_buffer(t):
    """values of t (already bf16-representable) stored as bf16 at the start of an fp32-sized buffer per group"""
    buf = torch.zeros(t.shape[0], t[0].numel())
    buf.view(torch.bfloat16)[:, :t[0].numel()] = t.reshape(t.shape[0], -1).to(torch.bfloat16)
    return buf


@pytest.mark.parametrize('io16', [0, 1])
@pytest.mark.parametrize('B,H2', [(3, 16), (5, 2)])
@pytest.mark.parametrize('C_', [32, 256])
def test_pool_act(C_, B, H2, io16):
    """MaxPool2d(2)(relu(a y + b)): fp32 within one float ulp of the float64 value rounded to float; bf16 in / out: the bf16 rounding of
    the float result on bf16-rounded input"""
    L, lib = _L()
    g = _gen(C_, B, H2, 11)
    H = 2 * H2
    y = torch.randn(G, B, H, H, C_, generator=g)
    a = torch.rand(G, C_, generator=g) + 0.5
    b = torch.randn(G, C_, generator=g) * 0.3
    if io16:
        y = y.to(torch.bfloat16).float()
    n = B * H2 * H2 * C_
    yd = (_bf16_buffer(y) if io16 else y.reshape(G, -1)).cuda()
    out = torch.full((G, n + 32), SENT, device='cuda')
    ad, bd = a.cuda(), b.cuda()
    L.check(lib.vv_pool_act(G, B, H2, H2, C_, yd.data_ptr(), yd.stride(0), ad.data_ptr(), bd.data_ptr(), C_, out.data_ptr(), out.stride(0),
                            io16, _st()), 'pool_act')
    out = out.cpu()
    assert torch.equal(out[:, -32:], torch.full((G, 32), SENT))
    for gi in range(G):
        ref = R.pool_act(y[gi].double(), a[gi].double(), b[gi].double()).float()          # float64 value rounded to float
        if io16:
            got = out[gi].view(torch.bfloat16)[:n].view(B, H2, H2, C_)
            assert torch.equal(got, ref.to(torch.bfloat16))
            assert torch.equal(out[gi, n // 2:], torch.full((n + 32 - n // 2,), SENT))          # bf16 elements: half the floats
        else:
            got = out[gi, :n].view(B, H2, H2, C_)
            ulp = torch.from_numpy(np.spacing(ref.abs().numpy()))
            assert ((got - ref).abs() <= ulp).all(), ((got - ref).abs() / ulp).max().item()


@pytest.mark.parametrize('out16', [0, 1])
def test_cube_erase(out16):
    """frame erasure through chmap: Cc = 15 channels padded to CP = 16, three UNets with -1 entries in different places; exact"""
    L, lib = _L()
    g = _gen(12, out16)
    Gc, npix, Cc, CP = 3, 1000, 15, 16
    cube = torch.rand(npix, Cc, generator=g)
    if out16:
        cube = cube.to(torch.bfloat16).float()
    chmap = torch.tensor([[0, 1, 2, 3, 4, 5, -1, -1, -1, 9, 10, 11, 12, 13, 14, -1],
                          [-1, -1, -1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, -1],
                          [14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, -1, -1, -1, -1]], dtype=torch.int32)
    n = npix * CP
    out = torch.full((Gc, n + 32), SENT, device='cuda')
    cd, md = cube.cuda(), chmap.cuda()
    L.check(lib.vv_cube_erase(Gc, npix, Cc, CP, cd.data_ptr(), md.data_ptr(), out.data_ptr(), out.stride(0), out16, _st()), 'cube_erase')
    out = out.cpu()
    ref = R.cube_erase(cube, chmap.long())
    assert torch.equal(out[:, -32:], torch.full((Gc, 32), SENT))
    if out16:
        assert torch.equal(out.view(torch.bfloat16)[:, :n].view(Gc, npix, CP), ref.to(torch.bfloat16))
    else:
        assert torch.equal(out[:, :n].view(Gc, npix, CP), ref)


@pytest.mark.parametrize('use_idx', [False, True])
@pytest.mark.parametrize('T,Tf,which', [(5, 1, 'both'), (5, 5, 'both'), (5, 1, 'raw'), (5, 5, 'flow')])
def test_cube_gather(T, Tf, which, use_idx):
    """uint8 [N, T, HW, 3] -> float32(u8) / float32(255) as [B, HW, 3T]; flow [N, Tf, HW, 2] -> [B, HW, 2Tf]; idx = NULL or with a repeat"""
    L, lib = _L()
    rng = np.random.RandomState(T * 10 + Tf)
    N, B, HW = 4, 3, 1024
    raw = rng.randint(0, 256, (N, T, HW, 3)).astype(np.uint8)
    flow = rng.randn(N, Tf, HW, 2).astype(np.float32)
    idx = np.array([2, 0, 2], dtype=np.int64) if use_idx else None
    rd = torch.from_numpy(raw).cuda() if which != 'flow' else None
    fd = torch.from_numpy(flow).cuda() if which != 'raw' else None
    idd = torch.from_numpy(idx).cuda() if use_idx else None
    x = torch.full((B * HW * 3 * T + 32,), SENT, device='cuda')
    xof = torch.full((B * HW * 2 * Tf + 32,), SENT, device='cuda')
    L.check(lib.vv_cube_gather(B, T, Tf, HW, idd.data_ptr() if use_idx else None, rd.data_ptr() if rd is not None else None,
                               fd.data_ptr() if fd is not None else None, x.data_ptr(), xof.data_ptr(), _st()), 'cube_gather')
    x, xof = x.cpu().numpy(), xof.cpu().numpy()
    rx, rf = R.cube_gather(raw[:B] if idx is None else raw, flow[:B] if idx is None else flow, idx)
    sent = np.float32(SENT)
    assert np.array_equal(x[:-32].reshape(rx.shape), rx) if which != 'flow' else (x == sent).all()
    assert np.array_equal(xof[:-32].reshape(rf.shape), rf) if which != 'raw' else (xof == sent).all()
    assert (x[-32:] == sent).all() and (xof[-32:] == sent).all()


@pytest.mark.parametrize('C_', [2, 15])
def test_nchw_to_nhwc(C_):
    L, lib = _L()
    B, HW = 3, 1000
    src = torch.randn(B, C_, HW, generator=_gen(C_, 13))
    dst = torch.full((B * HW * C_ + 32,), SENT, device='cuda')
    sd = src.cuda()
    L.check(lib.vv_nchw_to_nhwc(B, C_, HW, sd.data_ptr(), dst.data_ptr(), _st()), 'nchw_to_nhwc')
    dst = dst.cpu()
    assert torch.equal(dst[:-32].view(B, HW, C_), R.nchw_to_nhwc(src)) and torch.equal(dst[-32:], torch.full((32,), SENT))


@pytest.mark.parametrize('oc', [2, 3])
def test_out4_layout_copies(oc):
    """vv_out4_to_nchw into channels [choff, choff + oc) of a wider NCHW tensor (neighbours untouched), vv_nchw_to_out4 back (channels
    >= oc zeroed); both exact"""
    L, lib = _L()
    g = _gen(oc, 14)
    B, HW, Ctot, choff = 3, 1000, 9, 4
    out4 = torch.randn(B, HW, 4, generator=g)
    dst0 = torch.randn(B, Ctot, HW, generator=g)
    o4d = out4.cuda()
    dst = torch.cat([dst0.reshape(-1), torch.full((32,), SENT)]).cuda()
    L.check(lib.vv_out4_to_nchw(B, HW, oc, o4d.data_ptr(), dst.data_ptr(), Ctot, choff, _st()), 'out4_to_nchw')
    back = torch.full((B * HW * 4 + 32,), SENT, device='cuda')
    L.check(lib.vv_nchw_to_out4(B, HW, oc, dst.data_ptr(), Ctot, choff, back.data_ptr(), _st()), 'nchw_to_out4')
    dst, back = dst.cpu(), back.cpu()
    ref = R.out4_to_nchw(out4, dst0, oc, choff)
    assert torch.equal(dst[:-32].view(B, Ctot, HW), ref) and torch.equal(dst[-32:], torch.full((32,), SENT))
    assert torch.equal(back[:-32].view(B, HW, 4), R.nchw_to_out4(ref, oc, choff)) and torch.equal(back[-32:], torch.full((32,), SENT))
    assert back[:-32].view(B, HW, 4)[:, :, oc:].abs().max().item() == 0.0


@pytest.mark.parametrize('n', [1, 64, 65])
def test_counter_add(n):
    L, lib = _L()
    c0 = torch.arange(n + 3, dtype=torch.int64) * (10 ** 10) + 5
    cd = c0.cuda()
    L.check(lib.vv_counter_add(cd.data_ptr(), n, 3, _st()), 'counter_add')
    L.check(lib.vv_counter_add(cd.data_ptr(), n, 2 ** 33, _st()), 'counter_add')
    ref = c0.clone()
    ref[:n] += 3 + 2 ** 33
    assert torch.equal(cd.cpu(), ref)


# ================================================================================================ Adam

LR, B1, B2, EPS, GSCALE = float(np.float32(1e-3)), 0.9, 0.999, float(np.float32(1e-7)), float(np.float32(0.37))
B1F, B2F = float(np.float32(B1)), float(np.float32(B2))          # what the float arguments of the kernels hold
ADAM_BOUNDS = {1: [0, 4104], 3: [0, 4, 1000, 4104], 8: [0, 4, 100, 1000, 1004, 2048, 3000, 4000, 4104]}


def _adam_state(Gc, U, seed):
    g = _gen(Gc, U, seed)
    p = torch.randn(Gc, U, generator=g)
    m = torch.randn(Gc, U, generator=g) * 0.1
    v = torch.rand(Gc, U, generator=g) * 0.01
    grads = [torch.randn(Gc, U, generator=g) * (0.1 if s != 1 else 3.0) for s in range(3)]
    return p, m, v, grads


def _adam_reference(p, m, v, grads, dtype):
    """three steps of the restatement; betas as the kernels hold them (floats for the moments, doubles for the bias corrections)"""
    p, m, v = p.to(dtype), m.to(dtype), v.to(dtype)
    for t, gr in enumerate(grads, 1):
        sc = R.adam_scalars(LR, B1, B2, t)
        if dtype == torch.float32:
            sc = tuple(float(np.float32(s)) for s in sc)
        p, m, v = R.adam_step(p, gr.to(dtype), m, v, t, LR, B1F, B2F, EPS, GSCALE, scalars=sc)
    return p, m, v


@pytest.mark.parametrize('nb', [1, 3, 8])
def test_adam_tick_and_bucketed(nb):
    """three consecutive steps of vv_adam_tick + vv_adam_bucketed over [G = 3][U = 4104] from non-zero m / v, gradients in bucket-major
    layout (uneven bounds, one bucket 4 wide), grad_scale 0.37, eps 1e-7: param, m, v against float64; t_dev reads 3; the step scalars
    within one float ulp of the float64 values after every tick"""
    L, lib = _L()
    Gc, U = 3, 4096 + 8
    bounds = ADAM_BOUNDS[nb]
    p, m, v, grads = _adam_state(Gc, U, 15)
    # (param / m / v are [G][U] with group stride U: dense, with a sentinel tail behind the last group)
    pd, md, vd = (torch.cat([t.reshape(-1), torch.full((8,), SENT)]).cuda() for t in (p, m, v))
    t_dev = torch.zeros(2, dtype=torch.int64, device='cuda')
    t_dev[1] = -7
    sc = torch.full((4,), SENT, device='cuda')
    barr = (C.c_int64 * (nb + 1))(*bounds)
    for t, gr in enumerate(grads, 1):
        # (a tail as long as the tensor: a wrong bucket offset then reads sentinels inside the buffer, and shows, instead of reading past it)
        gd = torch.cat([R.to_bucket_major(gr, bounds), torch.full((Gc * U,), SENT)]).cuda()
        L.check(lib.vv_adam_tick(t_dev.data_ptr(), LR, B1, B2, sc.data_ptr(), _st()), 'tick')
        L.check(lib.vv_adam_bucketed(Gc, U, nb, barr, pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), sc.data_ptr(), B1F, B2F,
                                     EPS, GSCALE, _st()), 'adam_bucketed')
        torch.cuda.synchronize()
        ref = np.array(R.adam_scalars(LR, B1, B2, t))
        got = sc.cpu().numpy()
        assert (np.abs(got[:2].astype(np.float64) - ref) <= np.spacing(ref.astype(np.float32))).all(), (t, got, ref)
        assert (got[2:] == np.float32(SENT)).all()
    assert t_dev.cpu().tolist() == [3, -7]
    r64 = _adam_reference(p, m, v, grads, F64)
    r32 = _adam_reference(p, m, v, grads, torch.float32)
    for what, x, a64, a32 in zip(('param', 'm', 'v'), (pd, md, vd), r64, r32):
        x = x.cpu()
        assert torch.equal(x[-8:], torch.full((8,), SENT))
        _bar('adam_bucketed', (nb, what), x[:-8].view(Gc, U), a64, a32)


def test_adam_unbucketed():
    """vv_adam with host-computed bias corrections, the same numbers"""
    L, lib = _L()
    Gc, U = 3, 4096 + 8
    p, m, v, grads = _adam_state(Gc, U, 15)
    pd, md, vd = (torch.cat([t.reshape(-1), torch.full((8,), SENT)]).cuda() for t in (p, m, v))
    for t, gr in enumerate(grads, 1):
        gd = gr.reshape(-1).cuda()
        L.check(lib.vv_adam(Gc * U, pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), LR, B1F, B2F, EPS, 1.0 - B1 ** t,
                            (1.0 - B2 ** t) ** 0.5, GSCALE, _st()), 'adam')
        torch.cuda.synchronize()
    r64 = _adam_reference(p, m, v, grads, F64)
    r32 = _adam_reference(p, m, v, grads, torch.float32)
    for what, x, a64, a32 in zip(('param', 'm', 'v'), (pd, md, vd), r64, r32):
        x = x.cpu()
        assert torch.equal(x[-8:], torch.full((8,), SENT))
        _bar('adam', what, x[:-8].view(Gc, U), a64, a32)


# ================================================================================================ refusals

def test_refused_calls_return_their_status_and_launch_nothing():
    """unsupported arguments come back as a status (VV_ERR_BAD_ARG = 1 for a bad argument value, VV_ERR_UNSUPPORTED = 3 for a shape the
    kernel has no form for) with valid device pointers, and every buffer keeps its contents"""
    L, lib = _L()
    BAD_ARG, UNSUPPORTED = 1, 3
    bufs = [torch.full((4096,), SENT, device='cuda') for _ in range(5)]
    ptr = [t.data_ptr() for t in bufs]
    ints = torch.zeros(64, dtype=torch.int32, device='cuda')
    st = _st()
    assert lib.vv_adam(4094, ptr[0], ptr[1], ptr[2], ptr[3], LR, B1F, B2F, EPS, 0.1, 0.03, 1.0, st) == BAD_ARG
    for bounds in ([0, 8, 4, 16], [0, 8, 8, 16], [0, 6, 12, 16], [4, 8, 12, 16], [0, 4, 8, 12]):          # unsorted, empty, not x4, ends
        barr = (C.c_int64 * 4)(*bounds)
        assert lib.vv_adam_bucketed(2, 16, 3, barr, ptr[0], ptr[1], ptr[2], ptr[3], ptr[4], B1F, B2F, EPS, 1.0, st) == BAD_ARG, bounds
    assert lib.vv_bias_grad(2, 64, 24, ptr[0], 1536, 24, 0, ptr[1], ptr[2], 24, st) == UNSUPPORTED
    assert lib.vv_cube_erase(2, 8, 17, 20, ptr[0], ints.data_ptr(), ptr[1], 160, 0, st) == BAD_ARG
    assert lib.vv_out4_to_nchw(2, 16, 5, ptr[0], ptr[1], 8, 0, st) == BAD_ARG
    torch.cuda.synchronize()
    for t in bufs:
        assert torch.equal(t.cpu(), torch.full((4096,), SENT))
