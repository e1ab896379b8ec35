"""Kernel-level parity of FlowNet2's fp16 conv stack through the C ABI: vv_conv2d_f16 (every form launch_f16 can select on every
geometry, direct, row-K and split-K), vv_conv2d_splitk_finish_f16, vv_pack_conv2d_f16, vv_conv3x3_n2_f16 (every form of
launch_n2<vv_h>, both sides of every threshold), vv_deconv4x4_c2_f16 and vv_out8_to_nchw_f16 against the float64 restatements of
tests/flownet2_f16_ops_restatement.py on the exact fp16 operand values (docs/flownet2_ops_parity.md, "Kernel-level parity of the fp16
conv stack").  tests/test_flownet2_f16_ops_host.py imports the case tables and the checks of this module and runs torch's float32
evaluation of every case through them on the CPU: every bar and cap below is met by plain float32 arithmetic.

Every case: the source sits at coff = 8 inside pixels of ceil8(Cin) + 16 halves (the pointer itself is moved for the two-channel heads,
whose ABI has no offset; row-K has coff = 0, cstride = 8 as the ABI requires); pad channels, the channels in front of and behind the
slice and 64 halves behind the buffer hold finite random fp16 numbers.  The destination is a sentinel-filled buffer with coff = 3,
cstride = Cout + 7 and 64 halves of slack; everything outside [coff, coff + Cout) keeps the sentinel bit for bit.  Every launch is
repeated with all filler and slack redrawn and gives the same bits.  The tests upload the restatement's panel.  Every test asserts the
form its case selects.

Group E (exact): integer sources in [-3, 3], filters in [-2, 2], per-channel integer biases in [-6000, 6000]; every partial sum in any
order is an integer below 2^24, so the output is bit-equal to act_out_f16(pre64) and split-K slabs are bit-equal to the float64 partial
sums.  Asserted on the reference of every case with a bias: >= 25 % of the outputs need the first rounding, >= 10 % are exact ties,
>= 20 % are negative, and (slope 0.1) some value has rn(0.1f rn(pre)) != rn(0.1f pre).  The seed of a case is the first of its own
sequence whose reference meets these conditions (two-channel heads have two biases; most draws miss).  Cases with bias = NULL cannot
reach 2048 with these operands (|sum| <= taps * Cin * 6, typically a few hundred) and carry no such condition.  Two more exact groups
on one direct geometry and one n2 form: 'sub' (sources integers * 2^-24, filters multiples of 0.5, bias 0: every output subnormal,
ties on the 2^-24 grid) and 'ovf' (biases of +-65520 on some channels: outputs on both sides of the overflow edge, +-inf past it).

Group R (random): N(0, 1) sources, N / sqrt(K) filters, N biases, all rounded to fp16 (one case keeps an unrounded fp32 bias).
fp32 quantities (the float64 sum of split-K slabs against pre64 without bias): err_hip <= max(8 err_ref32, 16 * 2^-23).  fp16 outputs:
with e = max(8 err_ref32, 16 * 2^-23) * max |pre64| an element is bit-equal to act_out_f16(pre64) (+0 and -0 one value) unless
act_out_f16(pre64 - e) != act_out_f16(pre64 + e); then it is excused and must lie between those two.  That e made torch's own
float32 evaluation miss the 25 % cap on the long sums (26 - 36 % excused at K = 1377 and up: torch's float32 error grows with K, and e
with it), so the width is tightened element by element, never widened: e_i = min(e, 8 * 2^-24 * (sum |x| |w| + |bias|)_i), the a-priori
scale of float32 accumulation round-off of that element, as vv_correlation_nhwc_f16 is held to.  It is calibrated against torch's
float32 evaluation on the CPU (the host test asserts that evaluation inside it on every case), not against the kernels.  Caps:
excused <= 25 %, differing <= 1 % (<= 2 elements below 200 outputs).  The finish is bit-equal to splitk_finish_f16 of the downloaded
workspace in both groups.  Measured figures: docs/flownet2_ops_parity.md.
"""
import collections
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

import flownet2_f16_ops_restatement as R
from _util import FLOOR, SENT, err as _err, gen as _gen, observe

SLACK = 64
OK, BAD_ARG, UNSUPPORTED = 0, 1, 3
FAM = 'flownet2_f16_ops:'
GROUPS = ('E', 'R', 'sub', 'ovf')
I16 = torch.int16


# ================================================================================================ data, references, checks (no GPU)

def _ulp16(a):
    """fp16 spacing at |a| (float64): 2^(floor(log2 |a|) - 10), 2^-24 below 2^-14"""
    _, ex = torch.frexp(a.abs().clamp_min(2.0 ** -14))
    return torch.pow(2.0, (ex - 11).double())


def e_stats(pre, slope):
    """shares of outputs that need the first rounding, are exact ties, are negative; and whether skipping the first rounding shows"""
    r = R.rn_f16(pre)
    q = pre.abs() / (_ulp16(pre) / 2)
    ties = (q == q.floor()) & (q.floor() % 2 == 1)
    s = torch.tensor(float(slope), dtype=torch.float32).double()
    skipped = torch.where(pre > 0, r, R.rn_f16(pre * s))              # integers below 2^24 times a 24-bit slope: exact in float64
    shows = bool((skipped != R.act_out_f16(pre, slope)).any())
    return float((r.double() != pre).double().mean()), float(ties.double().mean()), float((pre < 0).double().mean()), shows


def _draw(group, g, de, Rk, Cin, Cout, B, H, W, has_bias, raw_bias):
    wshape = (Cin, Cout, 4, 4) if de else (Cout, Cin, Rk, Rk)
    if group == 'R':
        K = (16 if de else Rk * Rk) * Cin / (4 if de else 1)
        x = torch.randn(B, H, W, Cin, generator=g).half()
        w = (torch.randn(*wshape, generator=g) / K ** 0.5).half()
        bias = torch.randn(Cout, generator=g)
        if raw_bias:
            assert not torch.equal(bias.half().float(), bias)         # a bias fp16 cannot hold: the kernel adds it unrounded
        else:
            bias = bias.half().float()
        return x, w, (bias if has_bias else None)
    xi = torch.randint(-3, 4, (B, H, W, Cin), generator=g).double()
    if group == 'sub':
        return (xi * 2.0 ** -24).half(), (torch.randint(-4, 5, wshape, generator=g).double() * 0.5).half(), torch.zeros(Cout)
    w = torch.randint(-2, 3, wshape, generator=g).half()
    bias = torch.randint(-6000, 6001, (Cout,), generator=g).float()
    if group == 'ovf':
        bias[0::3] = 65520.0
        bias[1::3] = -65520.0
    return xi.half(), w, (bias if has_bias else None)


def _refs(de, Rk, stride, x, w, bias, slope):
    pre_nb = R.pre64(de, x, w, None, stride)
    Cout = pre_nb.shape[-1]
    pre_nb = pre_nb.reshape(-1, Cout)
    pre = pre_nb if bias is None else pre_nb + bias.double()
    xn, wf = x.float().permute(0, 3, 1, 2), w.float()
    if de:
        f32 = lambda b: F.conv_transpose2d(xn, wf, b, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Cout)
    else:
        f32 = lambda b: F.conv2d(xn, wf, b, stride=stride, padding=(Rk - 1) // 2).permute(0, 2, 3, 1).reshape(-1, Cout)
    D = dict(x=x, w=w, bias=bias, slope=slope, pre_nb=pre_nb, pre=pre, ref=R.act_out_f16(pre, slope), r32_nb=f32(None), r32=f32(bias))
    D['e32'] = _err(D['r32'], pre)
    # the element-wise width of group R (see check_out): 8 * 2^-24 * (sum |x| |w| + |bias|)
    absum = R.pre64(de, x.abs(), w.abs(), None, stride).reshape(-1, Cout)
    D['width'] = 8 * 2.0 ** -24 * (absum if bias is None else absum + bias.double().abs())
    return D


@functools.lru_cache(maxsize=2)
def make(group, key, de, Rk, stride, B, H, W, Cin, Cout, slope, has_bias=True, raw_bias=False):
    """operands and references of one group of one case; group E with a bias: the first seed whose reference meets the conditions"""
    assert (16 if de else Rk * Rk) * R.ceil_to(Cin, 32) * 6 + 65600 < 2 ** 24      # covers 6000 and the overflow biases
    conditioned = group == 'E' and has_bias
    for si in range(200):
        g = _gen(*[int(k) for k in key], GROUPS.index(group), si)
        D = _refs(de, Rk, stride, *_draw(group, g, de, Rk, Cin, Cout, B, H, W, has_bias, raw_bias), slope)
        if not conditioned:
            break
        rs, ts, ns, shows = e_stats(D['pre'], slope)
        if rs >= 0.25 and ts >= 0.10 and ns >= 0.20 and (shows or slope == 1.0):
            break
    if conditioned:
        rs, ts, ns, shows = e_stats(D['pre'], slope)
        assert rs >= 0.25 and ts >= 0.10 and ns >= 0.20, (key, rs, ts, ns)
        assert shows or slope == 1.0, key
    if group == 'sub':
        rs, ts, ns, shows = e_stats(D['pre'], slope)
        assert float(D['pre'].abs().max()) < 2.0 ** -14 and rs > 0.1 and ts > 0.1 and ns > 0.2, (key, rs, ts, ns)
    if group == 'ovf':
        ref, big = D['ref'], D['pre'].abs() > 65000
        assert bool(torch.isinf(ref[big]).any()) and bool(torch.isfinite(ref[big]).any()) and bool((ref == float('-inf')).any())
        assert bool((D['pre'][torch.isinf(ref)].abs() >= 65520).all())
    return D


def check_out(op, what, got, pre, ref, e32, slope, group, rec=True, width=None):
    """group E / sub / ovf: every bit; group R: the interval rule and its caps.  Figures are printed before anything is asserted."""
    assert got.dtype == torch.float16 and got.shape == ref.shape, (op, what)
    n = ref.numel()
    if group != 'R':
        same = int((got.view(I16) == ref.view(I16)).sum())
        print('E', op, what, group, 'bit-equal %d of %d' % (same, n))
        if rec:
            observe(FAM + op + ':E', n=n, bit_equal=same)
        assert same == n, (op, what, group, same, n)
        return
    e = max(8 * e32, FLOOR) * float(pre.abs().max())
    if width is not None:
        e = torch.clamp(width, max=e)                 # never wider than the rule's e; see the module docstring
    lo, hi = R.act_out_f16(pre - e, slope), R.act_out_f16(pre + e, slope)
    excused, differ = lo != hi, got != ref
    g = got.double()
    inside = (g >= lo.double()) & (g <= hi.double())
    n_exc, n_diff = int(excused.sum()), int(differ.sum())
    n_bad = int((differ & ~excused).sum()) + int((excused & ~inside).sum())
    print('R', op, what, 'n %d excused %.4f differing %.5f (%d) unexcused or outside %d' % (n, n_exc / n, n_diff / n, n_diff, n_bad))
    if rec:
        observe(FAM + op + ':R', n=n, excused=n_exc / n, differing=n_diff / n, n_differing=n_diff, err_ref32=e32)
    assert n_bad == 0, (op, what, n_bad)
    assert n_exc <= 0.25 * n, (op, what, n_exc, n)
    assert n_diff <= (2 if n < 200 else 0.01 * n), (op, what, n_diff, n)


def check_sum(op, what, total64, pre_nb, r32_nb, group, rec=True):
    """an fp32 quantity against the float64 value: exact in the exact groups, the float-summation rule in group R"""
    if group != 'R':
        assert torch.equal(total64, pre_nb), (op, what, group)
        return
    e_hip, e_32 = _err(total64, pre_nb), _err(r32_nb, pre_nb)
    print('R', op, what, 'err_hip %.3e err_ref32 %.3e' % (e_hip, e_32))
    if rec:
        observe(FAM + op + ':sum', err_hip=e_hip, err_ref32=e_32, ratio=e_hip / max(8 * e_32, FLOOR))
    assert e_hip <= max(8 * e_32, FLOOR), (op, what, e_hip, e_32)


# ------------------------------------------------------------------------------------------------ vv_conv2d_f16: case tables
Case = collections.namedtuple('Case', 'name de Rk stride H W Cin CinP Cout CoutP form pad0 slope has_bias raw_bias rowk groups')


def _case(name, de, Rk, stride, size, Cin, CinP, Cout, CoutP, form, pad0=0, slope=0.1, has_bias=True, raw_bias=False, rowk=False,
          groups=('E', 'R')):
    return Case(name, de, Rk, stride, size[0], size[1], Cin, CinP, Cout, CoutP, form, pad0, slope, has_bias, raw_bias, rowk, groups)


def _in_size(de, stride, extent, odd):
    """an input size whose tile-space extent is ``extent``: stride 2 has OH = (H - 1) // 2 + 1, one odd and one even input size"""
    if de or stride == 1:
        return extent
    return (2 * extent[0] - 1, 2 * extent[1] - 1) if odd else (2 * extent[0], 2 * extent[1])


GEOMS = [('1x1', False, 1, 1), ('3x3', False, 3, 1), ('3x3s2', False, 3, 2), ('5x5s2', False, 5, 2), ('7x7s2', False, 7, 2),
         ('deconv', True, 4, 2)]
DIRECT = []
for _i, (_n, _de, _R, _s) in enumerate(GEOMS):
    for _j, (_Cin, _CinP) in enumerate(((19, 32), (75, 96))):       # one chunk of 32 (two of 16 at stride 2) / the pipelined loop
        _t = '%s-c%d-' % (_n, _Cin)
        _odd = (_i + _j) % 2 == 0
        DIRECT += [_case(_t + 'nr1', _de, _R, _s, _in_size(_de, _s, (11, 37), _odd), _Cin, _CinP, 24, 32, 'nr1'),
                   _case(_t + 'nr2', _de, _R, _s, _in_size(_de, _s, (11, 37), not _odd), _Cin, _CinP, 40, 64, 'nr2'),
                   _case(_t + 'tw16nr2', _de, _R, _s, _in_size(_de, _s, (9, 16), _odd), _Cin, _CinP, 64, 64, 'tw16_nr2'),
                   _case(_t + 'tw16nr1', _de, _R, _s, _in_size(_de, _s, (11, 13), not _odd), _Cin, _CinP, 24, 32, 'tw16_nr1')]
    if _n in ('1x1', '3x3', 'deconv'):
        DIRECT += [_case(_n + '-c19-n16-13', _de, _R, _s, (11, 37), 19, 32, 13, 32, 'n16'),
                   _case(_n + '-c19-n16-16', _de, _R, _s, (11, 37), 19, 32, 16, 32, 'n16'),
                   _case(_n + '-c75-n16-13', _de, _R, _s, (11, 37), 75, 96, 13, 32, 'n16'),
                   _case(_n + '-c19-17', _de, _R, _s, (11, 37), 19, 32, 17, 32, 'nr1')]          # just above the N16 gate
DIRECT += [_case('3x3s2-c19-cout13', False, 3, 2, (21, 73), 19, 32, 13, 32, 'nr1'),             # stride 2 has no 16-wide form
           _case('3x3-c19-narrow-cout13', False, 3, 1, (11, 13), 19, 32, 13, 32, 'tw16_nr1'),    # narrow wins over N16
           _case('3x3-c19-nobias-noact', False, 3, 1, (11, 37), 19, 32, 24, 32, 'nr1', slope=1.0, has_bias=False),
           _case('3x3-c19-rawbias', False, 3, 1, (11, 37), 19, 32, 24, 32, 'nr1', raw_bias=True, groups=('R',)),
           _case('3x3-c19-sub-ovf', False, 3, 1, (11, 37), 19, 32, 24, 32, 'nr1', groups=('sub', 'ovf'))]

ROWK = []
for _Rk, _s, _Cin, _CinP, _sizes in ((7, 2, 3, 64, ((21, 73), (22, 74), (21, 31))), (3, 1, 6, 32, ((11, 37), (11, 13)))):
    for _sz in _sizes:                                                # the last size of each has LW <= 16: row-K stays on 32-wide tiles
        ROWK += [_case('rowk%d-%dx%d-nr1' % ((_Rk,) + _sz), False, _Rk, _s, _sz, _Cin, _CinP, 24, 32, 'nr1', rowk=True),
                 _case('rowk%d-%dx%d-nr2' % ((_Rk,) + _sz), False, _Rk, _s, _sz, _Cin, _CinP, 64, 64, 'nr2', rowk=True)]

SPLITK = [_case('3x3-k%d' % k, False, 3, 1, (11, 37), 153, 160, 24, 32, 'nr1', pad0=k) for k in (2, 3, 5, 6)] + [
    _case('3x3s2-k4', False, 3, 2, (21, 74), 91, 96, 24, 32, 'nr1', pad0=4),
    _case('1x1-nr2-k2', False, 1, 1, (11, 37), 75, 96, 40, 64, 'nr2', pad0=2),
    _case('deconv-k3', True, 4, 2, (11, 37), 91, 96, 24, 32, 'nr1', pad0=3),
    _case('n16-k2', False, 3, 1, (11, 37), 75, 96, 13, 32, 'n16', pad0=2),
    _case('tw16-k3', False, 3, 1, (9, 16), 91, 96, 64, 64, 'tw16_nr2', pad0=3)]
B_CONV = 3


def conv_form(c):
    return R.expected_form_f16(c.de, c.Rk, c.stride, c.W, c.Cout, c.CoutP, c.rowk)


def conv_geometry(c):
    OH, OW = (2 * c.H, 2 * c.W) if c.de else (R.conv_out_size(c.H, c.Rk, c.stride), R.conv_out_size(c.W, c.Rk, c.stride))
    return OH, OW, B_CONV * OH * OW


def conv_data(c, group):
    key = (c.de, c.Rk, c.stride, c.H, c.W, c.Cin, c.Cout, c.pad0, c.has_bias, c.rowk)
    return make(group, key, c.de, c.Rk, c.stride, B_CONV, c.H, c.W, c.Cin, c.Cout, c.slope, c.has_bias, c.raw_bias)


def conv_panel(c, D):
    if c.rowk:
        assert R.ROWK_KP[(c.Rk, c.stride)] == c.CinP
        return R.pack_panel_f16(R.rowk_weight_f16(D['w'].float()), c.CinP, c.CoutP, False)
    return R.pack_panel_f16(D['w'].float(), c.CinP, c.CoutP, c.de)


def slab_ranges(c):
    """the input channels of each split: whole chunks of CK, chunk k * nchunk / ksplit up to (k + 1) * nchunk / ksplit"""
    CK = R.CK_F16['deconv' if c.de else (c.Rk, c.stride)]
    nchunk = c.CinP // CK
    return [(nchunk * k // c.pad0 * CK, min(nchunk * (k + 1) // c.pad0 * CK, c.Cin)) for k in range(c.pad0)]


def slab_refs(c, D, dtype):
    """[ksplit][M][Cout] partial sums without bias: float64 of the restatement, or float32 by torch (the host's evaluation)"""
    M = conv_geometry(c)[2]
    out = torch.zeros(c.pad0, M, c.Cout, dtype=dtype)
    for k, (lo, hi) in enumerate(slab_ranges(c)):
        if lo >= hi:
            continue
        x, w = D['x'][..., lo:hi], (D['w'][lo:hi] if c.de else D['w'][:, lo:hi])
        if dtype == torch.float64:
            out[k] = R.pre64(c.de, x.contiguous(), w.contiguous(), None, c.stride).reshape(M, c.Cout)
        elif c.de:
            out[k] = F.conv_transpose2d(x.float().permute(0, 3, 1, 2), w.float(), None, stride=2, padding=1).permute(0, 2, 3, 1).reshape(M, c.Cout)
        else:
            out[k] = F.conv2d(x.float().permute(0, 3, 1, 2), w.float(), None, stride=c.stride,
                              padding=(c.Rk - 1) // 2).permute(0, 2, 3, 1).reshape(M, c.Cout)
    return out


def ws_columns(c):
    return 16 if c.form == 'n16' else c.CoutP          # the 16-wide form stores its 16 columns, the others the whole padded row


def conv_eval32(c, D):
    """what torch's float32 arithmetic gives for the case, in the shape of the kernel's results"""
    if c.pad0 <= 1:
        return R.act_out_f16(D['r32'].double(), c.slope)
    M = conv_geometry(c)[2]
    ws = torch.full((c.pad0, M, c.CoutP), SENT)
    ws[:, :, :ws_columns(c)] = 0
    ws[:, :, :c.Cout] = slab_refs(c, D, torch.float32)
    return ws.reshape(-1), R.splitk_finish_f16(ws.reshape(-1), c.pad0, M, c.Cout, c.CoutP, D['bias'], c.slope)


def conv_check(c, group, D, res, rec=True):
    op = ('rowk_' if c.rowk else 'splitk_' if c.pad0 > 1 else 'direct_') + c.form
    if c.pad0 <= 1:
        check_out(op, c.name, res, D['pre'], D['ref'], D['e32'], c.slope, group, rec, D['width'])
        return
    ws, fin = res
    M, ks = conv_geometry(c)[2], c.pad0
    slabs = ws[:ks * M * c.CoutP].view(ks, M, c.CoutP)
    nw = ws_columns(c)
    if nw > c.Cout:
        assert float(slabs[:, :, c.Cout:nw].abs().max()) == 0, 'pad columns of a slab are not 0'
    assert torch.equal(slabs[:, :, nw:], torch.full_like(slabs[:, :, nw:], SENT)), 'columns the form does not store changed'
    for k, (lo, hi) in enumerate(slab_ranges(c)):
        if lo >= hi:
            assert float(slabs[k, :, :nw].abs().max()) == 0, ('a slab without a chunk is not all zeros', k)
    if group != 'R':
        assert torch.equal(slabs[:, :, :c.Cout].double(), slab_refs(c, D, torch.float64)), 'slabs are not the exact partial sums'
    check_sum(op + '_slabs', c.name, slabs[:, :, :c.Cout].double().sum(0), D['pre_nb'], D['r32_nb'], group, rec)
    want = R.splitk_finish_f16(ws, ks, M, c.Cout, c.CoutP, D['bias'], c.slope)
    assert torch.equal(fin.view(I16), want.view(I16)), 'finish is not the fixed-order float32 sum, rounded as act_out_f16'
    check_out(op + '_finished', c.name, fin, D['pre'], D['ref'], D['e32'], c.slope, group, rec, D['width'])


def finish_case():
    """a workspace on which the ORDER of the float32 sum shows in the fp16 result on many elements (on a conv's own slabs it flips a
    handful, or none on a small case): slab 1 cancels slab 0 (~ 4096 N) up to an N(0, 1) rest, so whatever is added to slab 0 first
    is rounded to float32's spacing at 4096, half an fp16 step at 1"""
    ks, M, Cout, CoutP = 3, 257, 24, 32
    g = _gen(ks, M, Cout, CoutP)
    ws = torch.randn(ks, M, CoutP, generator=g)
    ws[0] *= 4096
    ws[1] = torch.randn(M, CoutP, generator=g) - ws[0]
    return ws.reshape(-1).contiguous(), ks, M, Cout, CoutP, torch.randn(Cout, generator=g), 0.1


# ------------------------------------------------------------------------------------------------ two-channel heads: case tables
N2 = [('tile16', 1, 101, 199, 2), ('tile16', 1, 101, 199, 16), ('tile32', 1, 101, 199, 17), ('tile32', 1, 101, 199, 32),
      ('split8', 1, 251, 401, 34),                                   # npix >= 100000, Cin > 32: fp16 has no 8 x 32 form
      ('split8', 3, 83, 81, 128), ('split8', 3, 83, 81, 130), ('split8', 3, 83, 81, 194),      # C4 = 32, 33, 49: the 4x-unrolled loop
      ('split32', 1, 64, 64, 33), ('split32', 1, 64, 64, 130), ('split32', 1, 64, 64, 318),
      ('split64', 1, 63, 65, 130), ('split64', 3, 7, 9, 130), ('split64', 1, 1, 37, 33), ('split64', 1, 29, 1, 40),
      ('tap16', 1, 64, 65, 322), ('tap32', 1, 32, 32, 386), ('tap64', 1, 31, 33, 320), ('tap64', 3, 4, 6, 1026)]
N2_EXTRA = ('split64', 3, 7, 9, 130)                                 # also runs the 'sub' and 'ovf' groups
N2_SLOPE = {'E': 0.1, 'R': 1.0, 'sub': 0.1, 'ovf': 0.1}            # predict_flow has no activation; the exact groups run the second rounding


def n2_groups(n):
    return ('E', 'R', 'sub', 'ovf') if n == N2_EXTRA else ('E', 'R')


def n2_data(n, group):
    _, B, H, W, Cin = n
    return make(group, (9, B, H, W, Cin), False, 3, 1, B, H, W, Cin, 2, N2_SLOPE[group])


C2 = [(4, 6, True), (4, 6, False), (11, 37, True), (11, 37, False)]


def c2_data(c, group):
    H, W, has_bias = c
    return make(group, (16, H, W, has_bias), True, 4, 2, B_CONV, H, W, 2, 2, N2_SLOPE[group], has_bias)


def c2_check(c, group, D, got, rec=True):
    """each output parity on its own (its own max |pre64| in the interval's width)"""
    H, W, _ = c
    v = lambda t: t.view(B_CONV, 2 * H, 2 * W, 2)
    for py in range(2):
        for px in range(2):
            s = lambda t: v(t)[:, py::2, px::2].reshape(-1, 2)
            e32 = _err(s(D['r32']), s(D['pre']))
            check_out('deconv_c2', (c, py, px), s(got).contiguous(), s(D['pre']), s(D['ref']).contiguous(), e32, D['slope'], group, rec, s(D['width']))


# ================================================================================================ launches (GPU)

def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


class _Src:
    """x [B, H, W, C] fp16 as channels [coff, coff + C) of pixels cstride halves wide; draw() gives a fresh device buffer with the same x
    and all the filler (pad channels, channels in front of coff and behind the slice, slack) redrawn"""

    def __init__(self, x, cstride, coff, g):
        self.x, self.cs, self.coff, self.g = x, cstride, coff, g
        self.npix = x.numel() // x.shape[-1]
        assert coff + R.ceil_to(x.shape[-1], 8) <= cstride and cstride % 8 == 0 and coff % 8 == 0

    def draw(self):
        buf = torch.randn(self.npix * self.cs + SLACK, generator=self.g).half()
        assert bool(torch.isfinite(buf).all())
        return R.view_fill(buf, self.x, self.cs, self.coff).cuda()


def _dst(M, Cout):
    ocs, ocoff = Cout + 7, 3
    return torch.full((M * ocs + SLACK,), SENT, dtype=torch.float16, device='cuda'), ocs, ocoff


def _dst_slice(out, M, ocs, ocoff, Cout):
    """the written slice [M, Cout]; everything else of the buffer must hold the sentinel bit for bit"""
    out = out.cpu()
    body = out[:M * ocs].view(M, ocs)
    keep = torch.ones(ocs, dtype=torch.bool)
    keep[ocoff:ocoff + Cout] = False
    rest = body[:, keep]
    assert torch.equal(rest.view(I16), torch.full_like(rest, SENT).view(I16)), 'channels beside the slice changed'
    tail = out[M * ocs:]
    assert torch.equal(tail.view(I16), torch.full_like(tail, SENT).view(I16)), 'slack behind the buffer changed'
    return body[:, ocoff:ocoff + Cout].clone()


def _same_bits(a, b):
    return torch.equal(a.view(I16), b.view(I16)) if a.dtype == torch.float16 else torch.equal(a, b)


def _conv_launch(c, group):
    L, lib = _L()
    assert conv_form(c) == c.form
    D = conv_data(c, group)
    OH, OW, M = conv_geometry(c)
    g = _gen(c.H, c.W, c.Cin, c.Cout, c.pad0, GROUPS.index(group), 77)
    if c.rowk:
        src, kind, pCin = _Src(D['x'], 8, 0, g), 2, c.CinP
    else:
        src, kind, pCin = _Src(D['x'], R.ceil_to(c.Cin, 8) + 16, 8, g), (1 if c.de else 0), c.Cin
    panel_d = conv_panel(c, D).cuda()
    bias_d = None if D['bias'] is None else D['bias'].cuda()
    bp = None if bias_d is None else bias_d.data_ptr()
    ks = c.pad0 if c.pad0 > 1 else 1
    Rk, stride = (4, 2) if c.de else (c.Rk, c.stride)
    outs = []
    for rep in range(2):
        buf = src.draw()
        sv = L.View(buf.data_ptr(), 0, src.cs, src.coff)
        out, ocs, ocoff = _dst(M, c.Cout)
        if ks == 1:
            p = L.Conv2dParams(kind, Rk, stride, B_CONV, c.H, c.W, pCin, c.CinP, c.Cout, c.CoutP, sv, panel_d.data_ptr(), bp, c.slope, c.pad0,
                               L.View(out.data_ptr(), 0, ocs, ocoff))
            L.check(lib.vv_conv2d_f16(C.byref(p), _st()), c.name)
            _sync()
            outs.append(_dst_slice(out, M, ocs, ocoff, c.Cout))
            continue
        # split-K: raw fp32 partial sums into a workspace [ks][M][CoutP]; five more rows and the slack behind them must stay
        ws = torch.full(((ks * M + 5) * c.CoutP + SLACK,), SENT, device='cuda')
        p = L.Conv2dParams(kind, Rk, stride, B_CONV, c.H, c.W, pCin, c.CinP, c.Cout, c.CoutP, sv, panel_d.data_ptr(), None, 1.0, c.pad0,
                           L.View(ws.data_ptr(), 0, c.CoutP, 0))
        L.check(lib.vv_conv2d_f16(C.byref(p), _st()), c.name)
        L.check(lib.vv_conv2d_splitk_finish_f16(ws.data_ptr(), ks, M, c.Cout, c.CoutP, bp, c.slope, out.data_ptr(), ocs, ocoff, _st()),
                c.name + ' finish')
        _sync()
        wsc = ws.cpu()
        assert torch.equal(wsc[ks * M * c.CoutP:], torch.full((5 * c.CoutP + SLACK,), SENT)), 'workspace rows behind ksplit * M changed'
        outs.append((wsc[:ks * M * c.CoutP].clone(), _dst_slice(out, M, ocs, ocoff, c.Cout)))
    if ks == 1:
        assert _same_bits(outs[0], outs[1]), 'the output depends on filler or slack'
    else:
        assert torch.equal(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1]), 'the output depends on filler or slack'
    conv_check(c, group, D, outs[0])


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.gpu
@pytest.mark.parametrize('c', DIRECT, ids=_ids(DIRECT))
def test_conv2d_f16_direct(c):
    """batch 3, two ragged tiles each way; the workgroup total is mostly no multiple of 8"""
    for group in c.groups:
        _conv_launch(c, group)


@pytest.mark.gpu
@pytest.mark.parametrize('c', ROWK, ids=_ids(ROWK))
def test_conv2d_f16_row_k(c):
    """kind 2: 8-half pixels at coff = 0, channels [Cin, 8) of every pixel hold garbage"""
    for group in c.groups:
        _conv_launch(c, group)


@pytest.mark.gpu
@pytest.mark.parametrize('c', SPLITK, ids=_ids(SPLITK))
def test_conv2d_f16_split_k_and_finish(c):
    """pad0 set directly: slabs (exact in group E, their float64 sum under the float-summation rule in group R), pad columns, a slab
    without a chunk, the rows behind ksplit * M, and vv_conv2d_splitk_finish_f16 bit-equal to the restatement of the workspace"""
    for group in c.groups:
        _conv_launch(c, group)


@pytest.mark.gpu
def test_conv2d_f16_refused_calls_write_nothing():
    L, lib = _L()
    B, H, W = 1, 8, 32
    src = torch.randn(B * H * W * 64 + SLACK, device='cuda').half()
    panel = torch.randn(49 * 64 * 64, device='cuda').half()
    out = torch.full((B * 4 * H * W * 64 + SLACK,), SENT, dtype=torch.float16, device='cuda')
    ws = torch.full((4 * B * 4 * H * W * 64 + SLACK,), SENT, device='cuda')

    def call(want, kind=0, Rk=3, stride=1, Cin=16, CinP=32, CoutP=32, cs=32, coff=0, pad0=0, sp=True, wp=True, op=True):
        dst = ws if pad0 > 1 else out
        p = L.Conv2dParams(kind, Rk, stride, B, H, W, Cin, CinP, 24, CoutP, L.View(src.data_ptr() if sp else None, 0, cs, coff),
                           panel.data_ptr() if wp else None, None, 0.1, pad0, L.View(dst.data_ptr() if op else None, 0, 40, 3))
        st = lib.vv_conv2d_f16(C.byref(p), _st())
        assert (st & 0xff) == want, (st, want, kind, Rk, stride, Cin, CinP, CoutP, cs, coff, pad0, sp, wp, op)

    assert lib.vv_conv2d_f16(None, _st()) == BAD_ARG
    call(BAD_ARG, sp=False)
    call(BAD_ARG, wp=False)
    call(BAD_ARG, op=False)
    call(BAD_ARG, CoutP=48)                                  # CoutP % 32
    call(BAD_ARG, cs=36)                                     # src.cstride % 8
    call(BAD_ARG, coff=4)                                    # src.coff % 8
    call(BAD_ARG, Cin=40)                                    # Cin > CinP
    call(BAD_ARG, CinP=48, cs=64)                            # CinP % 32, conv
    call(BAD_ARG, kind=1, Rk=4, stride=2, CinP=48, cs=64)    # CinP % 32, deconv
    call(BAD_ARG, coff=24)                                   # coff + ceil8(Cin) > cstride
    call(BAD_ARG, Cin=13, cs=16, coff=8)                     # the same through the rounding up of Cin: 8 + 16 > 16
    call(BAD_ARG, kind=1, Rk=3, stride=2)                    # kind 1 with R != 4
    call(BAD_ARG, kind=3)
    call(UNSUPPORTED, Rk=5, stride=1)
    rk = dict(kind=2, Rk=7, stride=2, Cin=64, CinP=64, cs=8)
    call(BAD_ARG, **dict(rk, coff=8))                        # row-K with coff != 0
    call(BAD_ARG, **dict(rk, pad0=2))                        # row-K with split-K
    call(BAD_ARG, **dict(rk, Cin=3))                         # row-K with Cin != CinP
    call(BAD_ARG, **dict(rk, cs=16))                         # row-K with cstride != 8
    call(UNSUPPORTED, **dict(rk, Cin=32, CinP=32))           # row-K with a wrong CinP: 7x7 s2 needs 64 ...
    call(UNSUPPORTED, kind=2, Rk=3, stride=1, Cin=64, CinP=64, cs=8)      # ... and 3x3 s1 needs 32
    assert lib.vv_conv2d_splitk_finish_f16(ws.data_ptr(), 0, 64, 24, 32, None, 0.1, out.data_ptr(), 40, 3, _st()) == BAD_ARG
    assert lib.vv_conv2d_splitk_finish_f16(None, 2, 64, 24, 32, None, 0.1, out.data_ptr(), 40, 3, _st()) == BAD_ARG
    _sync()
    assert bool((out == SENT).all()) and bool((ws == SENT).all())


@pytest.mark.gpu
def test_splitk_finish_f16_order_of_the_sum():
    """vv_conv2d_splitk_finish_f16 on its own, on a workspace where another order of the sum changes a third of the fp16 results"""
    L, lib = _L()
    ws, ks, M, Cout, CoutP, bias, slope = finish_case()
    out, ocs, ocoff = _dst(M, Cout)
    wsd = torch.cat([ws, torch.full((SLACK,), SENT)]).cuda()
    L.check(lib.vv_conv2d_splitk_finish_f16(wsd.data_ptr(), ks, M, Cout, CoutP, bias.cuda().data_ptr(), slope, out.data_ptr(), ocs, ocoff,
                                            _st()), 'finish')
    _sync()
    got, want = _dst_slice(out, M, ocs, ocoff, Cout), R.splitk_finish_f16(ws, ks, M, Cout, CoutP, bias, slope)
    same = int((got.view(I16) == want.view(I16)).sum())
    observe(FAM + 'finish:E', n=want.numel(), bit_equal=same)
    assert same == want.numel()


# ================================================================================================ vv_pack_conv2d_f16

PACK =[(1, 19, 32, 24, 32, 0), (9, 19, 32, 40, 64, 0), (16, 43, 48, 13, 32, 1), (16, 16, 16, 32, 32, 1), (25, 3, 16, 33, 64, 0),
        (49, 12, 16, 64, 64, 0), (7, 56, 64, 24, 32, 0),          # taps = R: the row-K panel
        (9, 500, 512, 1000, 1024, 0)]                               # above 16384 * 256 elements: the grid-stride loop runs
# exact ties (to even, both directions), subnormals and their ties, the overflow edge
PACK_EDGES = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2049.0, -2051.0, 3 * 2.0 ** -24, 2.0 ** -25, -3 * 2.0 ** -25, 5 * 2.0 ** -25,
              2.0 ** -14 - 2.0 ** -25, 65519.0, 65520.0, -70000.0, 65504.0, 1e-9]


def pack_weight(taps, K, KP, N, NP, tr):
    g = _gen(taps, K, KP, N, NP, tr)
    w = torch.randn(*((K, N) if tr else (N, K)), taps, generator=g)
    w.view(-1)[:len(PACK_EDGES)] = torch.tensor(PACK_EDGES)
    assert all(float(torch.tensor(v)) == v for v in PACK_EDGES[:-1])          # float32 holds every edge value exactly
    return w


@pytest.mark.gpu
@pytest.mark.parametrize('taps,K,KP,N,NP,tr', PACK)
def test_pack_conv2d_f16_bit_equal(taps, K, KP, N, NP, tr):
    L, lib = _L()
    w = pack_weight(taps, K, KP, N, NP, tr)
    assert (taps * KP * NP > 16384 * 256) == (KP == 512)
    out = torch.full((taps * KP * NP + SLACK,), SENT, dtype=torch.float16, device='cuda')
    L.check(lib.vv_pack_conv2d_f16(w.cuda().data_ptr(), out.data_ptr(), taps, K, KP, N, NP, tr, _st()), 'pack')
    _sync()
    out = out.cpu()
    assert torch.equal(out[-SLACK:], torch.full((SLACK,), SENT, dtype=torch.float16))
    want = R.pack_panel_f16(w, KP, NP, tr)
    same = int((out[:-SLACK].view(I16) == want.view(I16)).sum())
    observe(FAM + 'pack:E', n=want.numel(), bit_equal=same)
    assert same == want.numel()


@pytest.mark.gpu
def test_pack_conv2d_f16_refused():
    L, lib = _L()
    w = torch.randn(32 * 32 * 9, device='cuda')
    out = torch.full((9 * 64 * 64,), SENT, dtype=torch.float16, device='cuda')
    assert lib.vv_pack_conv2d_f16(w.data_ptr(), out.data_ptr(), 9, 19, 24, 24, 32, 0, _st()) == BAD_ARG      # KP % 16
    assert lib.vv_pack_conv2d_f16(w.data_ptr(), out.data_ptr(), 9, 19, 32, 24, 48, 0, _st()) == BAD_ARG      # NP % 32
    assert lib.vv_pack_conv2d_f16(None, out.data_ptr(), 9, 19, 32, 24, 32, 0, _st()) == BAD_ARG
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_conv3x3_n2_f16

@pytest.mark.gpu
@pytest.mark.parametrize('n', N2, ids=['%s-%dx%dx%d-%d' % n for n in N2])
def test_conv3x3_n2_f16_every_form(n):
    """every form of launch_n2<vv_h>, at both sides of every threshold; the pointer itself is moved to channel 8 of the wider pixel"""
    L, lib = _L()
    form, B, H, W, Cin = n
    npix = B * H * W
    assert R.n2_form_f16(npix, Cin) == form
    C4P = R.ceil_to(Cin, 32) // 4
    for group in n2_groups(n):
        D = n2_data(n, group)
        g = _gen(B, H, W, Cin, GROUPS.index(group), 78)
        src = _Src(D['x'], R.ceil_to(Cin, 8) + 16, 8, g)
        wq, bd = R.n2_weight(D['w'].float(), C4P).cuda(), D['bias'].cuda()
        outs = []
        for rep in range(2):
            buf = src.draw()
            out, ocs, ocoff = _dst(npix, 2)
            L.check(lib.vv_conv3x3_n2_f16(buf.data_ptr() + 2 * src.coff, src.cs, B, H, W, Cin, wq.data_ptr(), C4P, bd.data_ptr(), D['slope'],
                                          out.data_ptr(), ocs, ocoff, _st()), 'n2_f16')
            _sync()
            outs.append(_dst_slice(out, npix, ocs, ocoff, 2))
        assert _same_bits(outs[0], outs[1]), 'the output depends on filler or slack'
        check_out('n2_' + form, n, outs[0], D['pre'], D['ref'], D['e32'], D['slope'], group, width=D['width'])


@pytest.mark.gpu
def test_conv3x3_n2_f16_refused():
    L, lib = _L()
    src = torch.randn(4 * 6 * 40 + SLACK, device='cuda').half()
    wq = torch.randn(9 * 8 * 8, device='cuda')
    out = torch.full((4 * 6 * 9 + SLACK,), SENT, dtype=torch.float16, device='cuda')

    def call(cs=40, Cin=32, sp=True, wp=True, op=True):
        return lib.vv_conv3x3_n2_f16(src.data_ptr() if sp else None, cs, 1, 4, 6, Cin, wq.data_ptr() if wp else None, 8, None, 1.0,
                                     out.data_ptr() if op else None, 9, 3, _st())

    assert call(Cin=33) == BAD_ARG           # C4P * 4 < ceil32(Cin): 33 channels need 64 panel channels
    assert call(cs=38) == BAD_ARG
    assert call(cs=36) == BAD_ARG            # a multiple of 4 halves, not of 8: the header's rule for fp16 strides
    assert call(sp=False) == BAD_ARG and call(wp=False) == BAD_ARG and call(op=False) == BAD_ARG
    assert lib.vv_deconv4x4_c2_f16(None, 8, 1, 4, 6, wq.data_ptr(), None, 1.0, out.data_ptr(), 9, 3, _st()) == BAD_ARG
    _sync()
    assert bool((out == SENT).all())


# ================================================================================================ vv_deconv4x4_c2_f16

@pytest.mark.gpu
@pytest.mark.parametrize('c', C2, ids=['%dx%d-bias%d' % c for c in C2])
def test_deconv4x4_c2_f16(c):
    L, lib = _L()
    H, W, has_bias = c
    M = B_CONV * 4 * H * W
    for group in ('E', 'R'):
        D = c2_data(c, group)
        g = _gen(H, W, has_bias, GROUPS.index(group), 79)
        src = _Src(D['x'], 24, 8, g)
        wd, bd = D['w'].float().contiguous().cuda(), None if D['bias'] is None else D['bias'].cuda()
        outs = []
        for rep in range(2):
            buf = src.draw()
            out, ocs, ocoff = _dst(M, 2)
            L.check(lib.vv_deconv4x4_c2_f16(buf.data_ptr() + 2 * src.coff, src.cs, B_CONV, H, W, wd.data_ptr(),
                                            None if bd is None else bd.data_ptr(), D['slope'], out.data_ptr(), ocs, ocoff, _st()), 'c2_f16')
            _sync()
            outs.append(_dst_slice(out, M, ocs, ocoff, 2))
        assert _same_bits(outs[0], outs[1]), 'the output depends on filler or slack'
        c2_check(c, group, D, outs[0])


# ================================================================================================ vv_out8_to_nchw_f16

OUT8_EDGES = [float('inf'), float('-inf'), 2.0 ** -24, -3 * 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 65504.0, -0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize('dst_f16', [1, 0])
@pytest.mark.parametrize('B,HW,oc,Ctot,choff', [(3, 35, 1, 5, 2), (2, 273, 2, 4, 1), (1, 9, 3, 7, 4), (3, 35, 4, 6, 1), (2, 15, 2, 2, 0)])
def test_out8_to_nchw_f16(B, HW, oc, Ctot, choff, dst_f16):
    L, lib = _L()
    assert HW % 2 == 1 and choff + oc <= Ctot
    g = _gen(B, HW, oc, Ctot, choff)
    src = torch.randn(B * HW * 8 + SLACK, generator=g).half()
    src[:len(OUT8_EDGES) * 8:8] = torch.tensor(OUT8_EDGES).half()           # channel 0 of the first pixels
    dt = torch.float16 if dst_f16 else torch.float32
    dst0 = torch.full((B * Ctot * HW + SLACK,), SENT, dtype=dt)
    dst = dst0.cuda()
    L.check(lib.vv_out8_to_nchw_f16(B, HW, oc, src.cuda().data_ptr(), dst.data_ptr(), dst_f16, Ctot, choff, _st()), 'out8')
    _sync()
    got = dst.cpu()
    want = torch.cat([R.out8_to_nchw(src[:B * HW * 8], B, HW, oc, dst0[:B * Ctot * HW], Ctot, choff), dst0[B * Ctot * HW:]])
    bits = torch.int16 if dst_f16 else torch.int32
    same = int((got.view(bits) == want.view(bits)).sum())
    observe(FAM + 'out8:E', n=want.numel(), bit_equal=same)
    assert same == want.numel()


@pytest.mark.gpu
def test_out8_to_nchw_f16_refused():
    L, lib = _L()
    src = torch.randn(35 * 8, device='cuda').half()
    dst = torch.full((6 * 35,), SENT, dtype=torch.float16, device='cuda')
    assert lib.vv_out8_to_nchw_f16(1, 35, 5, src.data_ptr(), dst.data_ptr(), 1, 6, 0, _st()) == BAD_ARG          # oc > 4
    assert lib.vv_out8_to_nchw_f16(1, 35, 2, None, dst.data_ptr(), 1, 6, 0, _st()) == BAD_ARG
    _sync()
    assert bool((dst == SENT).all())
