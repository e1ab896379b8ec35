"""Kernel-level parity of FlowNet2's fp32 conv stack through the C ABI: vv_conv2d_mfma (every instantiation launch2d can select,
direct and split-K), vv_conv2d_splitk_finish, vv_pack_conv2d, vv_conv3x3_n2 (every form of launch_n2, both sides of every threshold),
vv_deconv4x4_c2, vv_conv2d_wino and vv_upsample4 against the float64 restatements of tests/flownet2_ops_restatement.py (checked against
torch in float64 by tests/test_flownet2_ops_host.py).

Common to every case: the source sits at coff = 4 inside a wider pixel; its pad channels, the channels in front of coff and 64 floats
behind the tensor hold finite random numbers (the header asks only that pad channels be finite; a recycled activation buffer holds
stale values there).  The destination is a sentinel-filled buffer with cstride = Cout + 7 and coff = 3 and 64 floats of slack;
everything outside [coff, coff + Cout) keeps the sentinel bit for bit.  Every launch is repeated with all filler and slack redrawn: the
output must be bit-equal.  Two groups of data per case; weights ~ 1 / sqrt(K) and bias ~ 1, so the bias is of the order of the output.
No element is left out of any comparison.

Bars (docs/flownet2_ops_parity.md): every element within 2e-5 of the float64 reference's maximum; for the direct kernel, the n2 forms,
the two-channel deconv and vv_upsample4 also the float-summation rule err_hip <= max(8 err_ref32, 16 * 2^-23), err = max |x - ref64| /
max |ref64|, err_ref32 = the same operation evaluated by torch on the CPU in float32.  No shape here needed a second float32 reference
for its summation length: the longest sum (9 x 1026 products) sits at 0.011 of the rule.  The Winograd form is held to the fixed 2e-5;
its ratio is recorded for scale only.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import flownet2_ops_restatement as R
from _util import FLOOR, SENT, err as _err, gen as _gen, observe

pytestmark = pytest.mark.gpu

SLACK = 64
OK, BAD_ARG, UNSUPPORTED = 0, 1, 3


def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _bars(op, what, got, ref64, ref32, rule=True):
    """prints / records the figures, then asserts the fixed bar and (rule) the float-summation rule"""
    e_hip, e_32 = _err(got, ref64), _err(ref32, ref64)
    observe('flownet2_ops:' + op, err_hip=e_hip, err_ref32=e_32, ratio=e_hip / max(8 * e_32, FLOOR))
    assert e_hip <= 2e-5, (op, what, e_hip)
    if rule:
        assert e_hip <= max(8 * e_32, FLOOR), (op, what, e_hip, e_32)


class _Src:
    """x [B, H, W, C] as channels [coff, coff + C) of pixels cstride wide; draw() gives a fresh device buffer with the same x and all
    the filler (pad channels, channels in front of coff and behind the tensor's channels, slack) redrawn"""

    def __init__(self, x, cstride, coff, g, slack=SLACK):
        self.x, self.cs, self.coff, self.g, self.slack = x, cstride, coff, g, slack
        self.npix = x.numel() // x.shape[-1]
        assert coff + x.shape[-1] <= cstride and cstride % 4 == 0 and coff % 4 == 0

    def draw(self):
        buf = torch.randn(self.npix * self.cs + self.slack, generator=self.g)
        return R.view_fill(buf, self.x, self.cs, self.coff).cuda()


def _dst(M, Cout):
    ocs, ocoff = Cout + 7, 3
    return torch.full((M * ocs + SLACK,), SENT, device='cuda'), ocs, ocoff


def _dst_slice(out, M, ocs, ocoff, Cout):
    """the written slice [M, Cout]; everything else of the buffer must hold the sentinel bit for bit"""
    out = out.cpu()
    body = out[:M * ocs].view(M, ocs)
    keep = torch.ones(ocs, dtype=torch.bool)
    keep[ocoff:ocoff + Cout] = False
    rest = body[:, keep]
    assert torch.equal(rest, torch.full_like(rest, SENT)), 'channels beside the slice changed'
    assert torch.equal(out[M * ocs:], torch.full((out.numel() - M * ocs,), SENT)), 'slack behind the buffer changed'
    return body[:, ocoff:ocoff + Cout].clone()


def _launch2d_form(de, Rk, stride, W, Cout, CoutP, rowk):
    """the instantiation launch2d selects (vv_conv2d.hip), from LW, Cout and CoutP"""
    LW = W if de else R.conv_out_size(W, Rk, stride)
    narrow = LW <= 16 and not rowk
    wide = CoutP % 64 == 0 and Cout > 32
    can16 = (de or (Rk == 3 and stride == 1)) and not rowk
    if narrow and wide:
        return 'tw16'
    if wide:
        return 'nr2'
    if can16 and Cout <= 16 and CoutP == 32:
        return 'n16'
    return 'nr1'


def _conv_refs(de, x, w, bias, stride, slope):
    """(ref64, ref32) of one conv / deconv layer on x [B, H, W, Cin] float32: the float64 restatement and torch's float32 evaluation"""
    b64 = None if bias is None else bias.double()
    xn = x.permute(0, 3, 1, 2)
    if de:
        ref64 = R.deconv_nhwc(x.double(), w.double(), b64, slope)
        r32 = F.leaky_relu(F.conv_transpose2d(xn, w, bias, stride=2, padding=1), slope).permute(0, 2, 3, 1)
    else:
        Rk = w.shape[-1]
        ref64 = R.conv_nhwc(x.double(), w.double(), b64, stride, slope)
        r32 = F.leaky_relu(F.conv2d(xn, w, bias, stride=stride, padding=(Rk - 1) // 2), slope).permute(0, 2, 3, 1)
    return ref64, r32


# ================================================================================================ vv_conv2d_mfma

def _draw_layer(g, de, Rk, Cin, Cout, has_bias):
    taps = 16 if de else Rk * Rk
    shape = (Cin, Cout, 4, 4) if de else (Cout, Cin, Rk, Rk)
    w = torch.randn(*shape, generator=g) / (taps * Cin / (4 if de else 1)) ** 0.5
    bias = torch.randn(Cout, generator=g) if has_bias else None
    return w, bias


def _conv2d_case(op, de, Rk, stride, B, H, W, Cin, CinP, Cout, CoutP, form, pad0=0, slope=0.1, has_bias=True, rowk_cs=0):
    L, lib = _L()
    assert _launch2d_form(de, Rk, stride, W, Cout, CoutP, bool(rowk_cs)) == form
    OH, OW = (2 * H, 2 * W) if de else (R.conv_out_size(H, Rk, stride), R.conv_out_size(W, Rk, stride))
    M = B * OH * OW
    for gi in range(2):
        g = _gen(Rk, stride, B, H, W, Cin, Cout, pad0, gi)
        x = torch.randn(B, H, W, Cin, generator=g)
        w, bias = _draw_layer(g, de, Rk, Cin, Cout, has_bias)
        ref64, r32 = _conv_refs(de, x, w, bias, stride, slope)
        ref64, r32 = ref64.reshape(M, Cout), r32.reshape(M, Cout)
        if rowk_cs:
            src = _Src(x, rowk_cs, 0, g)
            panel = R.pack_panel(R.rowk_weight(w, rowk_cs, CinP), CinP, CoutP, False)
            kind, pCin = 2, CinP
        else:
            src = _Src(x, 4 + R.ceil_to(Cin, 4) + 4, 4, g)
            panel = R.pack_panel(w, CinP, CoutP, de)
            kind, pCin = (1 if de else 0), Cin
        panel_d = panel.cuda()
        bias_d = None if bias is None else bias.cuda()
        ks = pad0 if pad0 > 1 else 1
        outs = []
        for rep in range(2):
            buf = src.draw()
            sv = L.View(buf.data_ptr(), 0, src.cs, src.coff)
            if ks == 1:
                out, ocs, ocoff = _dst(M, Cout)
                p = L.Conv2dParams(kind, 4 if de else Rk, 2 if de else stride, B, H, W, pCin, CinP, Cout, CoutP, sv, panel_d.data_ptr(),
                                   None if bias_d is None else bias_d.data_ptr(), slope, pad0, L.View(out.data_ptr(), 0, ocs, ocoff))
                L.check(lib.vv_conv2d_mfma(C.byref(p), _st()), op)
                _sync()
                outs.append(_dst_slice(out, M, ocs, ocoff, Cout))
                continue
            # split-K: raw partial sums into a workspace [ks][M][CoutP]; five more rows and the slack behind them must stay
            ws = torch.full(((ks * M + 5) * CoutP + SLACK,), SENT, device='cuda')
            p = L.Conv2dParams(kind, 4 if de else Rk, 2 if de else stride, B, H, W, pCin, CinP, Cout, CoutP, sv, panel_d.data_ptr(),
                               None, 1.0, pad0, L.View(ws.data_ptr(), 0, CoutP, 0))
            L.check(lib.vv_conv2d_mfma(C.byref(p), _st()), op)
            out, ocs, ocoff = _dst(M, Cout)
            L.check(lib.vv_conv2d_splitk_finish(ws.data_ptr(), ks, M, Cout, CoutP, None if bias_d is None else bias_d.data_ptr(), slope,
                                                out.data_ptr(), ocs, ocoff, _st()), op + ' finish')
            _sync()
            wsc = ws.cpu()
            assert torch.equal(wsc[ks * M * CoutP:], torch.full((5 * CoutP + SLACK,), SENT)), 'workspace rows behind ksplit * M changed'
            outs.append((wsc[:ks * M * CoutP].clone(), _dst_slice(out, M, ocs, ocoff, Cout)))
        if ks == 1:
            assert torch.equal(outs[0], outs[1]), 'the output depends on filler or slack'
            _bars(op, (gi,), outs[0], ref64, r32)
            continue
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), 'the output depends on filler or slack'
        wsc, fin = outs[0]
        slabs = wsc.view(ks, M, CoutP)
        nwritten = 16 if form == 'n16' else CoutP          # the 16-wide form stores its 16 columns, the others the whole padded row
        if nwritten > Cout:
            assert float(slabs[:, :, Cout:nwritten].abs().max()) == 0                               # zero weights: exactly 0
        assert torch.equal(slabs[:, :, nwritten:], torch.full_like(slabs[:, :, nwritten:], SENT))
        nchunk = CinP // (16 if (de or stride == 1) else 8)
        for k in range(ks):
            if nchunk * k // ks == nchunk * (k + 1) // ks:      # a slab with no chunk comes out all zeros
                assert float(slabs[k, :, :nwritten].abs().max()) == 0, k
        total = slabs[:, :, :Cout].double().sum(0)
        if bias is not None:
            total = total + bias.double()
        _bars(op + '_slabs', (gi,), R.act(total, slope), ref64, r32)
        assert torch.equal(fin, R.splitk_finish_f32(wsc, ks, M, Cout, CoutP, bias, slope)), 'finish is not the fixed-order float32 sum'
        _bars(op + '_finished', (gi,), fin, ref64, r32)


GEOMS = [('1x1', False, 1, 1), ('3x3', False, 3, 1), ('3x3s2', False, 3, 2), ('5x5s2', False, 5, 2), ('7x7s2', False, 7, 2),
         ('deconv', True, 4, 2)]


def _in_size(de, stride, extent, odd):
    """an input size whose tile-space extent is ``extent``: the size itself (stride 1, deconv) or, for stride 2 with padding
    (R - 1) // 2, OH = (H - 1) // 2 + 1, one odd and one even input size"""
    if de or stride == 1:
        return extent
    return (2 * extent[0] - 1, 2 * extent[1] - 1) if odd else (2 * extent[0], 2 * extent[1])


DIRECT = []
for _i, (_name, _de, _R, _s) in enumerate(GEOMS):
    # NR = 1 (32-wide) and NR = 2 (64-wide, the second N block masked from lane 8); stride 2: odd input for one, even for the other
    DIRECT.append((_name + '-nr1', _de, _R, _s, (11, 37), True, 24, 32, 'nr1'))
    DIRECT.append((_name + '-nr2', _de, _R, _s, (11, 37), False, 40, 64, 'nr2'))
    DIRECT.append((_name + '-tw16', _de, _R, _s, (9, 16), _i % 2 == 0, 64, 64, 'tw16'))
    if _name in ('3x3', 'deconv'):
        DIRECT.append((_name + '-n16-13', _de, _R, _s, (11, 37), True, 13, 32, 'n16'))
        DIRECT.append((_name + '-n16-16', _de, _R, _s, (11, 37), True, 16, 32, 'n16'))
        DIRECT.append((_name + '-17', _de, _R, _s, (11, 37), True, 17, 32, 'nr1'))      # just above the N16 gate


@pytest.mark.parametrize('name,de,Rk,stride,extent,odd,Cout,CoutP,form', DIRECT, ids=[d[0] for d in DIRECT])
def test_conv2d_mfma_direct(name, de, Rk, stride, extent, odd, Cout, CoutP, form):
    """batch 3 (the workgroup total is no multiple of 8), Cin = 19 (CinP = 32), two ragged tiles each way"""
    H, W = _in_size(de, stride, extent, odd)
    _conv2d_case('direct_' + form, de, Rk, stride, 3, H, W, 19, 32, Cout, CoutP, form)


def test_conv2d_mfma_direct_no_bias_no_activation():
    _conv2d_case('direct_nr1', False, 3, 1, 3, 11, 37, 19, 32, 24, 32, 'nr1', slope=1.0, has_bias=False)


@pytest.mark.parametrize('Rk,stride,cs,Cin,CinP,size', [(7, 2, 4, 3, 32, (21, 73)), (7, 2, 4, 3, 32, (22, 74)), (3, 1, 8, 6, 24, (11, 37))])
@pytest.mark.parametrize('Cout,CoutP,form', [(24, 32, 'nr1'), (64, 64, 'nr2')])
def test_conv2d_mfma_row_k(Rk, stride, cs, Cin, CinP, size, Cout, CoutP, form):
    """kind 2: src.coff = 0 as the ABI requires, the pad channels of the 4- / 8-float pixels hold garbage"""
    _conv2d_case('rowk_' + form, False, Rk, stride, 3, size[0], size[1], Cin, CinP, Cout, CoutP, form, rowk_cs=cs)


# (id, de, R, stride, H, W, Cin, CinP, Cout, CoutP, form, pad0)
SPLITK = [('3x3-k%d' % k, False, 3, 1, 11, 37, 75, 80, 24, 32, 'nr1', k) for k in (2, 3, 5, 6)] + [
    ('3x3s2-k4', False, 3, 2, 21, 74, 43, 48, 24, 32, 'nr1', 4), ('1x1-k2', False, 1, 1, 11, 37, 19, 32, 40, 64, 'nr2', 2),
    ('deconv-k3', True, 4, 2, 11, 37, 43, 48, 24, 32, 'nr1', 3), ('n16-k2', False, 3, 1, 11, 37, 19, 32, 13, 32, 'n16', 2),
    ('tw16-k3', False, 3, 1, 9, 16, 43, 48, 64, 64, 'tw16', 3)]


@pytest.mark.parametrize('name,de,Rk,stride,H,W,Cin,CinP,Cout,CoutP,form,pad0', SPLITK, ids=[s[0] for s in SPLITK])
def test_conv2d_mfma_split_k_and_finish(name, de, Rk, stride, H, W, Cin, CinP, Cout, CoutP, form, pad0):
    """pad0 set directly: the float64 sum of the slabs and the finished output meet the bars, vv_conv2d_splitk_finish is bit-equal to
    the float32 fixed-order sum of the downloaded workspace, a slab without a chunk is all zeros, rows behind ksplit * M stay"""
    _conv2d_case('splitk_' + form, de, Rk, stride, 3, H, W, Cin, CinP, Cout, CoutP, form, pad0=pad0)


def test_conv2d_mfma_refused_calls_write_nothing():
    L, lib = _L()
    B, H, W, Cin = 1, 8, 32, 16
    src = torch.randn(B * H * W * 32 + SLACK, device='cuda')
    panel = torch.randn(49 * 32 * 64, device='cuda')
    out = torch.full((B * 4 * H * W * 40 + SLACK,), SENT, device='cuda')

    def call(want, kind=0, Rk=3, stride=1, Cin=Cin, CinP=16, CoutP=32, cs=32, coff=0, pad0=0):
        p = L.Conv2dParams(kind, Rk, stride, B, H, W, Cin, CinP, 24, CoutP, L.View(src.data_ptr(), 0, cs, coff), panel.data_ptr(), None,
                           0.1, pad0, L.View(out.data_ptr(), 0, 40, 4))
        st = lib.vv_conv2d_mfma(C.byref(p), _st())
        assert (st & 0xff) == want, (st, want, kind, Rk, stride, Cin, CinP, CoutP, cs, coff, pad0)

    call(BAD_ARG, kind=0, CinP=24)                  # CinP % 16, conv
    call(BAD_ARG, kind=1, Rk=4, stride=2, CinP=24)  # CinP % 16, deconv
    call(BAD_ARG, CoutP=48)                         # CoutP % 32
    call(BAD_ARG, cs=30)                            # src.cstride % 4
    call(BAD_ARG, coff=2)                           # src.coff % 4
    rk = dict(kind=2, Rk=7, stride=2, Cin=32, CinP=32, cs=4)
    call(BAD_ARG, **dict(rk, coff=4))               # row-K with coff != 0
    call(BAD_ARG, **dict(rk, pad0=2))               # row-K with split-K
    call(BAD_ARG, **dict(rk, Cin=3))                # row-K with Cin != CinP
    call(UNSUPPORTED, **dict(rk, cs=8))             # row-K geometries: only 7 / 2 / 4 / 32 and 3 / 1 / 8 / 24
    call(UNSUPPORTED, **dict(rk, Rk=5))
    call(UNSUPPORTED, kind=2, Rk=3, stride=1, Cin=24, CinP=24, cs=4)
    call(UNSUPPORTED, Rk=5, stride=1)
    call(UNSUPPORTED, Rk=3, stride=3)
    call(BAD_ARG, kind=3)
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_pack_conv2d

PACK = [(1, 19, 32, 24, 32, 0), (9, 19, 32, 40, 64, 0), (16, 43, 48, 13, 32, 1), (16, 16, 16, 32, 32, 1), (25, 3, 8, 33, 64, 0),
        (49, 12, 16, 64, 64, 0), (7, 32, 32, 24, 32, 0),          # taps = R: the row-K panel
        (9, 500, 512, 1000, 1024, 0)]                               # above 16384 * 256 elements: the grid-stride loop runs


@pytest.mark.parametrize('taps,K,KP,N,NP,tr', PACK)
def test_pack_conv2d_bit_equal(taps, K, KP, N, NP, tr):
    L, lib = _L()
    g = _gen(taps, K, KP, N, NP, tr)
    w = torch.randn(*((K, N) if tr else (N, K)), taps, generator=g)
    assert (taps * KP * NP > 16384 * 256) == (KP == 512)
    out = torch.full((taps * KP * NP + SLACK,), SENT, device='cuda')
    L.check(lib.vv_pack_conv2d(w.cuda().data_ptr(), out.data_ptr(), taps, K, KP, N, NP, tr, _st()), 'pack')
    _sync()
    out = out.cpu()
    assert torch.equal(out[-SLACK:], torch.full((SLACK,), SENT))
    assert torch.equal(out[:-SLACK], R.pack_panel(w, KP, NP, tr))


def test_pack_conv2d_refused():
    L, lib = _L()
    w = torch.randn(32 * 32 * 9, device='cuda')
    out = torch.full((9 * 64 * 64,), SENT, device='cuda')
    assert lib.vv_pack_conv2d(w.data_ptr(), out.data_ptr(), 9, 19, 20, 24, 32, 0, _st()) == BAD_ARG      # KP % 8
    assert lib.vv_pack_conv2d(w.data_ptr(), out.data_ptr(), 9, 19, 24, 24, 48, 0, _st()) == BAD_ARG      # NP % 32
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_conv3x3_n2

def _n2_form(npix, Cin):
    """the form launch_n2 selects for the fp32 entry (vv_conv2d.hip)"""
    if npix >= 20000 and Cin <= 32:
        return 'tile16' if Cin <= 16 else 'tile32'
    if npix >= 100000:
        return '8x32'
    if npix >= 20000:
        return 'split8'
    if Cin >= 320:
        return 'tap16' if npix >= 4096 else ('tap32' if npix >= 1024 else 'tap64')
    return 'split32' if npix >= 4096 else 'split64'


N2 = [('tile16', 1, 101, 199, 2), ('tile16', 1, 101, 199, 16), ('tile32', 1, 101, 199, 17), ('tile32', 1, 101, 199, 32),
      ('8x32', 1, 251, 401, 34), ('8x32', 1, 251, 401, 70),
      ('split8', 3, 83, 81, 128), ('split8', 3, 83, 81, 130), ('split8', 3, 83, 81, 194),      # C4 = 32, 33, 49: the 4x-unrolled loop
      ('split32', 1, 64, 64, 33), ('split32', 1, 64, 64, 130), ('split32', 1, 64, 64, 318),
      ('split64', 1, 63, 65, 130), ('split64', 3, 7, 9, 130),
      ('tap16', 1, 64, 65, 322), ('tap32', 1, 32, 32, 386), ('tap64', 1, 31, 33, 320), ('tap64', 3, 4, 6, 1026)]


@pytest.mark.parametrize('form,B,H,W,Cin', N2, ids=['%s-%dx%dx%d-%d' % n for n in N2])
def test_conv3x3_n2_every_form(form, B, H, W, Cin):
    """every form of launch_n2, at both sides of every threshold; the ABI has no source offset, so the pointer itself is moved to
    channel 4 of the wider pixel; where Cin % 4 != 0 the pad channels hold garbage"""
    L, lib = _L()
    npix = B * H * W
    assert _n2_form(npix, Cin) == form
    C4P = R.ceil_to(Cin, 32) // 4
    for gi in range(2):
        g = _gen(B, H, W, Cin, gi)
        x = torch.randn(B, H, W, Cin, generator=g)
        w = torch.randn(2, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        bias = torch.randn(2, generator=g)
        slope = 1.0 if gi == 0 else 0.1                      # predict_flow has no activation; the second group takes the other branch
        ref64, r32 = _conv_refs(False, x, w, bias, 1, slope)
        ref64, r32 = ref64.reshape(npix, 2), r32.reshape(npix, 2)
        src = _Src(x, 4 + R.ceil_to(Cin, 4) + 4, 4, g)
        wq, bd = R.n2_weight(w, C4P).cuda(), bias.cuda()
        outs = []
        for rep in range(2):
            buf = src.draw()
            out, ocs, ocoff = _dst(npix, 2)
            L.check(lib.vv_conv3x3_n2(buf.data_ptr() + 4 * src.coff, src.cs, B, H, W, Cin, wq.data_ptr(), C4P, bd.data_ptr(), slope,
                                      out.data_ptr(), ocs, ocoff, _st()), 'n2')
            _sync()
            outs.append(_dst_slice(out, npix, ocs, ocoff, 2))
        assert torch.equal(outs[0], outs[1]), 'the output depends on filler or slack'
        _bars('n2_' + form, (gi,), outs[0], ref64, r32)


def test_conv3x3_n2_refused():
    L, lib = _L()
    src = torch.randn(4 * 6 * 40 + SLACK, device='cuda')
    wq = torch.randn(9 * 8 * 8, device='cuda')
    out = torch.full((4 * 6 * 9 + SLACK,), SENT, device='cuda')
    # C4P * 4 < ceil32(Cin): 33 channels need 64 panel channels
    assert lib.vv_conv3x3_n2(src.data_ptr(), 40, 1, 4, 6, 33, wq.data_ptr(), 8, None, 1.0, out.data_ptr(), 9, 3, _st()) == BAD_ARG
    assert lib.vv_conv3x3_n2(src.data_ptr(), 38, 1, 4, 6, 32, wq.data_ptr(), 8, None, 1.0, out.data_ptr(), 9, 3, _st()) == BAD_ARG
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_deconv4x4_c2

@pytest.mark.parametrize('has_bias', [True, False])
@pytest.mark.parametrize('H,W', [(4, 6), (11, 37)])
def test_deconv4x4_c2(H, W, has_bias):
    L, lib = _L()
    B = 3
    M = B * 4 * H * W
    for gi in range(2):
        g = _gen(H, W, has_bias, gi)
        x = torch.randn(B, H, W, 2, generator=g)
        w = torch.randn(2, 2, 4, 4, generator=g) / 8 ** 0.5
        bias = torch.randn(2, generator=g) if has_bias else None
        slope = 1.0 if gi == 0 else 0.1
        ref64, r32 = _conv_refs(True, x, w, bias, 2, slope)
        src = _Src(x, 12, 4, g)
        wd, bd = w.cuda(), None if bias is None else bias.cuda()
        outs = []
        for rep in range(2):
            buf = src.draw()
            out, ocs, ocoff = _dst(M, 2)
            L.check(lib.vv_deconv4x4_c2(buf.data_ptr() + 4 * src.coff, src.cs, B, H, W, wd.data_ptr(), None if bd is None else bd.data_ptr(),
                                        slope, out.data_ptr(), ocs, ocoff, _st()), 'c2')
            _sync()
            outs.append(_dst_slice(out, M, ocs, ocoff, 2))
        assert torch.equal(outs[0], outs[1]), 'the output depends on filler or slack'
        got = outs[0].view(B, 2 * H, 2 * W, 2)
        for py in range(2):
            for px in range(2):           # the four output parities, each against its own maximum
                _bars('deconv_c2', (gi, py, px), got[:, py::2, px::2], ref64[:, py::2, px::2], r32[:, py::2, px::2])


# ================================================================================================ vv_conv2d_wino

def _wino_panel(L, lib, w, K, KP, N):
    wd = w.contiguous().cuda()
    panel = torch.empty(16 * KP * N, device='cuda')
    tab = torch.frombuffer(bytearray(bytes((L.PackEntry * 1)(L.PackEntry(0, 0, 0, K, KP, N)))), dtype=torch.uint8).cuda()
    L.check(lib.vv_pack_wino(tab.data_ptr(), 1, 1, wd.data_ptr(), wd.numel(), panel.data_ptr(), panel.numel(), KP * N, _st()), 'pack_wino')
    return panel


# K = 473: CinP = 480 channels read from coff = 4 of 480-float pixels run 4 floats past every pixel, at the last pixel past the tensor,
# where src_elems must turn the reads into zeros; H % 4 == 2; one block wide; B = 1 and B = 3
@pytest.mark.parametrize('B,H,W,Cin,Cout,cs', [(3, 6, 32, 473, 64, 480), (1, 6, 32, 473, 32, 480), (1, 8, 64, 40, 32, 48), (3, 4, 32, 19, 64, 28)])
def test_conv2d_wino(B, H, W, Cin, Cout, cs):
    L, lib = _L()
    M, CinP = B * H * W, R.ceil_to(Cin, 8)
    for gi in range(2):
        g = _gen(B, H, W, Cin, Cout, gi)
        x = torch.randn(B, H, W, Cin, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
        bias = torch.randn(Cout, generator=g)
        slope = 0.1 if gi == 0 else 1.0
        ref64, r32 = _conv_refs(False, x, w, bias, 1, slope)
        ref64, r32 = ref64.reshape(M, Cout), r32.reshape(M, Cout)
        src = _Src(x, cs, 4, g)
        panel, bd = _wino_panel(L, lib, w, Cin, CinP, Cout), bias.cuda()
        outs = []
        for rep in range(2):
            buf = src.draw()
            out, ocs, ocoff = _dst(M, Cout)
            # src_elems stops in front of the slack: whatever the slack holds, reads past the tensor must come back as zeros
            L.check(lib.vv_conv2d_wino(buf.data_ptr(), cs, 4, M * cs, panel.data_ptr(), bd.data_ptr(), slope, out.data_ptr(), ocs, ocoff,
                                       B, H, W, CinP, Cout, _st()), 'wino')
            _sync()
            outs.append(_dst_slice(out, M, ocs, ocoff, Cout))
        assert torch.equal(outs[0], outs[1]), 'the output depends on filler or slack'
        _bars('wino', (gi,), outs[0], ref64, r32, rule=False)


def test_conv2d_wino_refused():
    L, lib = _L()
    src = torch.randn(8 * 64 * 16 + SLACK, device='cuda')
    panel = torch.randn(16 * 8 * 64, device='cuda')
    out = torch.full((8 * 64 * 71 + SLACK,), SENT, device='cuda')

    def call(H=8, W=64, Cout=32, coff=4):
        return lib.vv_conv2d_wino(src.data_ptr(), 16, coff, 8 * 64 * 16, panel.data_ptr(), None, 0.1, out.data_ptr(), 71, 3, 1, H, W, 8, Cout, _st())

    assert call(H=7) == UNSUPPORTED and call(W=48) == UNSUPPORTED and call(Cout=48) == UNSUPPORTED and call(coff=2) == UNSUPPORTED
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_upsample4

@pytest.mark.parametrize('H,W', [(9, 13), (1, 7), (5, 1)])
@pytest.mark.parametrize('BC', [1, 6])
def test_upsample4(BC, H, W):
    """all three modes; a single row / column is where mode 2 guards a division; nearest is bit-equal to src * scale in float32"""
    L, lib = _L()
    n = BC * 16 * H * W
    for gi in range(2):
        g = _gen(BC, H, W, gi)
        x = torch.randn(BC, H, W, generator=g)
        scale = 20.0 if gi == 0 else 0.05
        for mode in (0, 1, 2):
            outs = []
            for rep in range(2):
                xd = torch.cat([x.reshape(-1), torch.randn(SLACK, generator=g)]).cuda()
                out = torch.full((n + SLACK,), SENT, device='cuda')
                L.check(lib.vv_upsample4(xd.data_ptr(), out.data_ptr(), BC, H, W, mode, scale, _st()), 'upsample4')
                _sync()
                out = out.cpu()
                assert torch.equal(out[n:], torch.full((SLACK,), SENT))
                outs.append(out[:n].view(BC, 4 * H, 4 * W).clone())
            assert torch.equal(outs[0], outs[1])
            if mode == 0:
                assert torch.equal(outs[0], R.upsample4(x, 0, torch.tensor(scale)))
                continue
            kw = {'align_corners': mode == 2}
            r32 = F.interpolate(x[None], scale_factor=4, mode='bilinear', **kw)[0] * scale
            _bars('upsample4_mode%d' % mode, (gi,), outs[0], R.upsample4(x.double(), mode, scale), r32)


# ================================================================================================ the 2 GiB guard

def test_conv2d_mfma_refuses_a_source_its_loader_cannot_address():
    """The staging loads of vv_conv2d_mfma form 32-bit BYTE offsets against a 2^31 - 1 byte descriptor: a source of 2^31 bytes or more
    must be refused (VV_ERR_UNSUPPORTED), not read as zeros from element 2^29 on.  A 3x3 stride-2 launch on a zero-filled source of just
    over 2 GiB (cstride 64, H * W just over 2^23) with data in its last 16 rows only; both buffers are allocated at their true full size,
    so a launch stays in bounds whatever the guard does."""
    L, lib = _L()
    B, H, W, cs, Cin, Cout = 1, 2049, 4096, 64, 56, 8
    assert H * W > 2 ** 23 and B * H * W * cs * 4 >= 2 ** 31 and B * H * W * cs < 2 ** 31
    g = _gen(H, W, cs)
    src = torch.zeros(B * H * W * cs + SLACK, device='cuda')
    src[(H - 16) * W * cs:H * W * cs] = torch.randn(16 * W * cs, generator=g).cuda()
    w, bias = _draw_layer(g, False, 3, Cin, Cout, True)
    panel, bd = R.pack_panel(w, 64, 32, False).cuda(), bias.cuda()
    OH, OW = R.conv_out_size(H, 3, 2), R.conv_out_size(W, 3, 2)
    out, ocs, ocoff = _dst(B * OH * OW, Cout)
    p = L.Conv2dParams(0, 3, 2, B, H, W, Cin, 64, Cout, 32, L.View(src.data_ptr(), 0, cs, 4), panel.data_ptr(), bd.data_ptr(), 0.1, 0,
                       L.View(out.data_ptr(), 0, ocs, ocoff))
    st = lib.vv_conv2d_mfma(C.byref(p), _st())
    _sync()
    assert st == UNSUPPORTED, st
    assert bool((out == SENT).all())
