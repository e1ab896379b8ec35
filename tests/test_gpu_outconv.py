"""Kernel-level parity of the 1x1 output conv family (vv_outconv_fwd, vv_outconv_bwd, vv_outconv_fwdbwd, vv_outconv_bwd_reduce: four
channels per lane for fp32 y, eight per lane for bf16 y, C = 32 and C = 64 each) and of vv_fold_bn, through the C ABI, against the
float64 restatements of tests/train_ops_restatement.py (checked against torch autograd by tests/test_train_ops_host.py).  Method and
bars are those of tests/test_gpu_train_ops.py: `_bar` (err_hip <= max(8 err_ref32, 16 * 2^-23) with err_ref32 the SAME restatement in
float32 on the same inputs), bit-equality where the arithmetic is the same, sentinels behind and beside every output, no element left
out.  The figures are recorded under observe('outconv:...') and tabulated in docs/train_ops_parity.md.

One case: G = 3 groups of different data, oc = (3, 2, 3), tgt_src = (0, 1, 0), tgt_coff = (6, 2, 0) into tgt0 [B, HW, 15] and
tgt1 [B, HW, 4], a gscale per group.  The C ABI has ONE `w` and ONE `bias` pointer for all groups (group g at + g * param_gstride), so
the bias sits at the same offset in every block: a block holds max(oc) * C floats of filter rows (rows [0, oc) the group's filter, the
rows behind them finite random filler), then the oc biases, then 4 * C + 4 - oc floats of finite random filler.  The backward kernels
read four filter rows whatever oc is (d(out) is 0 in the rows >= oc), so what lies there must not matter: a second run with all the
filler redrawn leaves the same bits.  param_gstride, ab_gstride, y_gstride and dA_gstride all differ from the dense sizes.

Shapes: HW = 1024 (the bank's), 200 (no multiple of a trip of 64 / 128 / 256 pixels: the last trip is ragged inside the unroll),
40 (below one trip: pixel groups without a pixel); B = 1, 3, 8 -> 3, 9, 24 work items against the (B G + 7) / 8 * 8 grid.

bf16 family (y holds bf16 elements): the inputs are the bf16 rounding of the fp32 y, nudged again so that no |a y + b| of the ROUNDED
values is below 1e-3; the restatement runs on the rounded values.  dA stored as bf16: |dA - ref64| <= 2^-8 |ref64| + FLOOR max|ref64|
elementwise (bf16 keeps 8 significant bits: a nearest-even rounding of x is within 2^-8 |x|, reached just above a power of two; the
fp32 error in front of it, which can tip a value to the neighbouring bf16, adds (1 + 2^-8) times itself and is of the order of
2^-23 max|ref64|), and the BatchNorm-backward sums are those of the STORED values."""
import ctypes as C_
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import train_ops_restatement as R
from _util import FLOOR, SENT, away_from_zero as _away_from_zero, bar, err as _err, gen as _gen, observe

pytestmark = pytest.mark.gpu

G = 3
OCS = (3, 2, 3)
OCS_ODD = (1, 4, 2)          # accepted by the kernels, never used by the bank
TSRC = (0, 1, 0)
GSCALE = (0.7, 0.013, 2.5)
SLACK = 64
CASES = ([(C, HW, 3, OCS) for C in (32, 64) for HW in (1024, 200, 40)] + [(C, 200, B, OCS) for C in (32, 64) for B in (1, 8)] +
         [(C, 200, 3, OCS_ODD) for C in (32, 64)])
BAD_ARG, UNSUPPORTED = 1, 3


def _bar(op, what, got, ref64, ref32):
    bar(op, what, got, ref64, ref32, family='outconv')


def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _tcoff(ocs):
    return (6, 2, 0) if ocs == OCS else (6, 0, 0)          # (a 4-channel group reads all four channels of tgt1)


def _filler(prm, ocs, C, g):
    """redraw every float of the parameter blocks that is neither a filter row < oc nor a bias < oc"""
    boff = max(ocs) * C
    new = torch.randn(prm.shape, generator=g)
    for gi, oc in enumerate(ocs):
        new[gi, :oc * C] = prm[gi, :oc * C]
        new[gi, boff:boff + oc] = prm[gi, boff:boff + oc]
    return new


@functools.lru_cache(maxsize=2)
def _case(C, HW, B, ocs):
    """the CPU inputs of one case (float32), shared by the families"""
    g = _gen(C, HW, B, ocs[1])
    c = NS(C=C, HW=HW, B=B, ocs=ocs, boff=max(ocs) * C, tcoff=_tcoff(ocs))
    c.pgs = c.boff + 4 + 4 * C                                  # a multiple of 4 floats: the kernels load filter rows as float4
    c.abs_ = C + 4
    c.a = torch.rand(G, c.abs_, generator=g) + 0.5
    c.b = torch.randn(G, c.abs_, generator=g) * 0.3
    c.mean = torch.randn(G, c.abs_, generator=g) * 0.1
    c.invstd = torch.rand(G, c.abs_, generator=g) + 0.5
    c.y = _away_from_zero(torch.randn(G, B * HW, C, generator=g), c.a[:, None, :C], c.b[:, None, :C])
    yb = _away_from_zero(c.y.bfloat16().float(), c.a[:, None, :C], c.b[:, None, :C], margin=4e-3).bfloat16()
    assert (c.a[:, None, :C].double() * yb.double() + c.b[:, None, :C].double()).abs().min().item() >= 1e-3
    c.y16 = yb
    prm = torch.zeros(G, c.pgs)
    for gi, oc in enumerate(ocs):
        prm[gi, :oc * C] = torch.randn(oc * C, generator=g) * 0.2
        prm[gi, c.boff:c.boff + oc] = torch.randn(oc, generator=g)
    c.prm = _filler(prm, ocs, C, g)
    c.prm2 = _filler(prm, ocs, C, g)
    assert not torch.equal(c.prm, c.prm2)
    c.tgt0 = torch.rand(B, HW, 15, generator=g)
    c.tgt1 = torch.randn(B, HW, 4, generator=g)
    c.gscale = torch.tensor(GSCALE)
    return c


def _group(c, gi, y16, dt):
    """the arguments of the restatements for group gi in dtype dt"""
    oc = c.ocs[gi]
    y = (c.y16.float() if y16 else c.y)[gi].view(c.B, c.HW, c.C)
    tgt = (c.tgt0, c.tgt1)[TSRC[gi]][..., c.tcoff[gi]:c.tcoff[gi] + oc]
    w, bias = c.prm[gi, :oc * c.C].view(oc, c.C), c.prm[gi, c.boff:c.boff + oc]
    return NS(oc=oc, y=y.to(dt), a=c.a[gi, :c.C].to(dt), b=c.b[gi, :c.C].to(dt), w=w.to(dt), bias=bias.to(dt), tgt=tgt.to(dt),
              gscale=c.gscale[gi].to(dt), mean=c.mean[gi, :c.C].to(dt), invstd=c.invstd[gi, :c.C].to(dt))


def _bwd(q, dout4, dA_stored=None):
    return R.outconv_backward(dout4, q.y, q.a, q.b, q.w, q.mean, q.invstd, dA_stored)


def _partial(r):
    """the [B, 4 C + 4] rows vv_outconv_bwd leaves per cube from outconv_backward's result"""
    return torch.cat([r[1].reshape(r[1].shape[0], -1), r[2]], 1)


@functools.lru_cache(maxsize=2)
def _refs(C, HW, B, ocs, y16):
    """per group and precision: forward; backward fed the float rounding of the float64 d(out); the chain forward -> backward"""
    c = _case(C, HW, B, ocs)
    out = []
    for gi in range(G):
        q64, q32 = _group(c, gi, y16, torch.float64), _group(c, gi, y16, torch.float32)
        f64 = R.outconv_forward(q64.y, q64.a, q64.b, q64.w, q64.bias, q64.oc, q64.tgt, q64.gscale)
        f32 = R.outconv_forward(q32.y, q32.a, q32.b, q32.w, q32.bias, q32.oc, q32.tgt, q32.gscale)
        din = f64[2].float()
        out.append(NS(q64=q64, q32=q32, f64=f64, f32=f32, din=din, b64=_bwd(q64, din.double()), b32=_bwd(q32, din),
                      c64=_bwd(q64, f64[2]), c32=_bwd(q32, f32[2])))
    return out


class _Dev:
    """device buffers of one case / family; every output is filled with the sentinel and has slack behind it"""

    def __init__(self, c, y16, da16, prm=None):
        self.c, self.y16, self.da16 = c, y16, da16
        n = c.B * c.HW
        self.n = n
        ysrc = c.y16 if y16 else c.y
        ybuf = torch.zeros(G, n * c.C + SLACK, dtype=ysrc.dtype)
        ybuf[:, :n * c.C] = ysrc.reshape(G, -1)
        self.y = ybuf.cuda()
        self.y_gs = self.y.stride(0) // (2 if y16 else 1)
        self.a, self.b, self.mean, self.invstd = (t.cuda() for t in (c.a, c.b, c.mean, c.invstd))
        self.prm = (c.prm if prm is None else prm).cuda()
        self.tgt0, self.tgt1, self.gscale = c.tgt0.cuda(), c.tgt1.cuda(), c.gscale.cuda()
        self.oc = torch.tensor(c.ocs, dtype=torch.int32).cuda()
        self.tsrc = torch.tensor(TSRC, dtype=torch.int32).cuda()
        self.tcoff = torch.tensor(c.tcoff, dtype=torch.int32).cuda()
        self.nout = 4 * c.C + 4

    def full(self, *shape, dtype=torch.float32):
        return torch.full(shape, SENT, dtype=dtype, device='cuda')

    def params(self, L, out4, score, gscale, dout4):
        c, p = self.c, lambda t: None if t is None else t.data_ptr()
        return L.OutconvParams(G, c.B, c.HW, c.C, self.y.data_ptr(), self.y_gs, self.a.data_ptr(), self.b.data_ptr(), c.abs_,
                               self.prm.data_ptr(), self.prm.data_ptr() + 4 * c.boff, c.pgs, self.oc.data_ptr(),
                               self.tgt0.data_ptr(), 15, 1 if self.y16 else 0, self.tgt1.data_ptr(), 4, 0, self.tsrc.data_ptr(),
                               self.tcoff.data_ptr(), p(out4), p(score), p(gscale), p(dout4))

    def fwd_bufs(self):
        return self.full(G * self.n * 4 + SLACK), self.full(G * self.n * 4 + SLACK), self.full(G * self.c.B + 16)

    def bwd_bufs(self):
        c = self.c
        dA = self.full(G, self.n * c.C + 2 * SLACK, dtype=torch.bfloat16 if self.da16 else torch.float32)
        return dA, self.full(G * c.B * self.nout + SLACK), self.full(G * c.B * 2 * c.C + SLACK)

    def dA_gs(self, dA):
        return dA.stride(0) // (2 if self.da16 else 1)

    def flags(self):
        return (1 if self.da16 else 0) | (2 if self.y16 else 0)

    def fwd(self, L, lib, nulls=False):
        out4, dout4, score = self.fwd_bufs()
        p = self.params(L, None if nulls else out4, score, None if nulls else self.gscale, None if nulls else dout4)
        L.check(lib.vv_outconv_fwd(C_.byref(p), _st()), 'outconv_fwd')
        return out4.cpu(), dout4.cpu(), score.cpu()

    def bwd(self, L, lib, dout4_dev, bn=True):
        c = self.c
        dA, part, bnp = self.bwd_bufs()
        L.check(lib.vv_outconv_bwd(G, c.B, c.HW, c.C, dout4_dev.data_ptr(), self.y.data_ptr(), self.y_gs, self.a.data_ptr(),
                                   self.b.data_ptr(), c.abs_, self.prm.data_ptr(), c.pgs, dA.data_ptr(), self.dA_gs(dA), part.data_ptr(),
                                   self.mean.data_ptr(), self.invstd.data_ptr(), bnp.data_ptr() if bn else None, self.flags(), _st()),
                'outconv_bwd')
        return dA.cpu(), part.cpu(), bnp.cpu()

    def fwdbwd(self, L, lib):
        out4, dout4, score = self.fwd_bufs()
        dA, part, bnp = self.bwd_bufs()
        p = self.params(L, out4, score, self.gscale, dout4)
        L.check(lib.vv_outconv_fwdbwd(C_.byref(p), dA.data_ptr(), self.dA_gs(dA), part.data_ptr(), self.mean.data_ptr(),
                                      self.invstd.data_ptr(), bnp.data_ptr(), self.flags(), _st()), 'outconv_fwdbwd')
        return (out4.cpu(), dout4.cpu(), score.cpu()), (dA.cpu(), part.cpu(), bnp.cpu())


def _sent(t):
    return torch.equal(t, torch.full_like(t, SENT))


def _split_fwd(c, out4, dout4, score):
    n = c.B * c.HW
    assert _sent(out4[G * n * 4:]) and _sent(dout4[G * n * 4:]) and _sent(score[G * c.B:])
    return out4[:G * n * 4].view(G, c.B, c.HW, 4), dout4[:G * n * 4].view(G, c.B, c.HW, 4), score[:G * c.B].view(G, c.B)


def _split_bwd(c, dA, part, bnp, bn=True):
    n, nout = c.B * c.HW, 4 * c.C + 4
    assert _sent(dA[:, n * c.C:]) and _sent(part[G * c.B * nout:])          # beside (between the groups) and behind
    assert _sent(bnp[G * c.B * 2 * c.C:] if bn else bnp)
    return dA[:, :n * c.C].view(G, c.B, c.HW, c.C), part[:G * c.B * nout].view(G, c.B, nout), bnp[:G * c.B * 2 * c.C].view(G, c.B, 2, c.C)


def _check_dA(op, da16, got, ref64, ref32):
    if not da16:
        return _bar(op, 'dA', got, ref64, ref32)
    dev = (got.double() - ref64).abs()
    allow = 2.0 ** -8 * ref64.abs() + FLOOR * ref64.abs().max()
    observe('outconv:' + op + '_bf16', worst_over_allowed=(dev / allow).max().item(), err_hip=_err(got, ref64))
    assert bool((dev <= allow).all()), (op, (dev / allow).max().item())


def _check_bnpart(op, r, bnp, dA_stored):
    """the sums against the restatement evaluated on what the kernel stored (float, or the float value of the stored bf16)"""
    s64 = _bwd(r.q64, r.din.double(), dA_stored.double())
    s32 = _bwd(r.q32, r.din, dA_stored.float())
    _bar(op, 'sum g', bnp[:, 0], s64[5], s32[5])
    _bar(op, 'sum g xhat', bnp[:, 1], s64[6], s32[6])


@pytest.mark.parametrize('family', ['fp32', 'bf16', 'bf16_dA16'])
@pytest.mark.parametrize('C,HW,B,ocs', CASES)
def test_output_conv_kernels_against_float64(C, HW, B, ocs, family):
    """one case through all four entry points (module docstring); family: fp32 y (four channels per lane), bf16 y (eight per lane)
    with dA stored as float or as bf16"""
    L, lib = _L()
    y16, da16 = family != 'fp32', family == 'bf16_dA16'
    fam = '8' if y16 else '4'
    c, refs = _case(C, HW, B, ocs), _refs(C, HW, B, ocs, y16)
    d = _Dev(c, y16, da16)

    # ---- vv_outconv_fwd: out4, dout4, score; channels >= oc exactly 0; the same score bits without the optional outputs
    raw_fwd = d.fwd(L, lib)
    out4, dout4, score = _split_fwd(c, *raw_fwd)
    for gi, r in enumerate(refs):
        _bar('fwd%s_out' % fam, gi, out4[gi], r.f64[0], r.f32[0])
        _bar('fwd%s_dout' % fam, gi, dout4[gi], r.f64[2], r.f32[2])
        _bar('fwd%s_score' % fam, gi, score[gi], r.f64[1], r.f32[1])
        if r.q64.oc < 4:
            assert out4[gi, ..., r.q64.oc:].abs().max().item() == 0.0 and dout4[gi, ..., r.q64.oc:].abs().max().item() == 0.0
    o4n, d4n, score_n = d.fwd(L, lib, nulls=True)
    assert _sent(o4n) and _sent(d4n) and torch.equal(score_n, raw_fwd[2])

    # ---- vv_outconv_bwd fed the float rounding of the float64 d(out) (zeros at channels >= oc)
    din = torch.full((G * c.B * c.HW * 4 + SLACK,), SENT)
    din[:G * c.B * c.HW * 4] = torch.stack([r.din for r in refs]).reshape(-1)
    din = din.cuda()
    raw_bwd = d.bwd(L, lib, din)
    dA, part, bnp = _split_bwd(c, *raw_bwd)
    for gi, r in enumerate(refs):
        _check_dA('bwd%s_dA' % fam, da16, dA[gi].float(), r.b64[0], r.b32[0])
        _bar('bwd%s_partial' % fam, gi, part[gi], _partial(r.b64), _partial(r.b32))
        if r.q64.oc < 4:
            assert part[gi, :, r.q64.oc * C:4 * C].abs().max().item() == 0.0 and part[gi, :, 4 * C + r.q64.oc:].abs().max().item() == 0.0
        _check_bnpart('bwd%s_bnpart' % fam, r, bnp[gi], dA[gi])
    nb = d.bwd(L, lib, din, bn=False)
    _split_bwd(c, *nb, bn=False)
    assert torch.equal(nb[0], raw_bwd[0]) and torch.equal(nb[1], raw_bwd[1])
    other = _Dev(c, y16, da16, prm=c.prm2).bwd(L, lib, din)          # the rows >= oc the kernel reads must not matter
    assert all(torch.equal(x, y) for x, y in zip(other, raw_bwd))

    # ---- vv_outconv_bwd_reduce on that partial: rows / entries >= oc keep the sentinel
    gs = 4 * C + 4 + 8
    grads = d.full(G * gs + SLACK)
    pdev = raw_bwd[1].cuda()
    L.check(lib.vv_outconv_bwd_reduce(G, C, c.B, pdev.data_ptr(), d.oc.data_ptr(), grads.data_ptr(), grads.data_ptr() + 4 * 4 * C, gs,
                                      _st()), 'outconv_bwd_reduce')
    grads = grads.cpu()
    assert _sent(grads[G * gs:])
    grads = grads[:G * gs].view(G, gs)
    for gi, r in enumerate(refs):
        oc = r.q64.oc
        _bar('reduce%s_dW' % fam, gi, grads[gi, :oc * C], r.b64[3][:oc].reshape(-1), r.b32[3][:oc].reshape(-1))
        _bar('reduce%s_db' % fam, gi, grads[gi, 4 * C:4 * C + oc], r.b64[4][:oc], r.b32[4][:oc])
        assert _sent(grads[gi, oc * C:4 * C]) and _sent(grads[gi, 4 * C + oc:])

    # ---- vv_outconv_fwdbwd: the bits of vv_outconv_fwd followed by vv_outconv_bwd on the d(out) it wrote, and the float64 chain
    kd = raw_fwd[1].cuda()
    two = d.bwd(L, lib, kd)
    f_fwd, f_bwd = d.fwdbwd(L, lib)
    assert all(torch.equal(x, y) for x, y in zip(f_fwd, raw_fwd)), 'out4 / dout4 / score'
    assert torch.equal(f_bwd[0], two[0]), 'dA'
    assert torch.equal(f_bwd[1], two[1]), 'partial'
    assert torch.equal(f_bwd[2], two[2]), 'bnpart'
    dA, part, bnp = _split_bwd(c, *f_bwd)
    for gi, r in enumerate(refs):
        _check_dA('fwdbwd%s_dA' % fam, da16, dA[gi].float(), r.c64[0], r.c32[0])
        _bar('fwdbwd%s_partial' % fam, gi, part[gi], _partial(r.c64), _partial(r.c32))
        s64 = _bwd(r.q64, r.f64[2], dA[gi].double())
        s32 = _bwd(r.q32, r.f32[2], dA[gi].float())
        _bar('fwdbwd%s_bnpart' % fam, 'sum g', bnp[gi, :, 0], s64[5], s32[5])
        _bar('fwdbwd%s_bnpart' % fam, 'sum g xhat', bnp[gi, :, 1], s64[6], s32[6])


def _ulp32(x64):
    """one float ulp at the float rounding of x (float64 array)"""
    return np.spacing(np.abs(x64.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize('C,nblk', [(32, n) for n in (1, 6, 7, 8, 13, 14, 15, 300)] + [(64, n) for n in (1, 2, 3, 4, 6, 7, 300)])
def test_output_conv_reduce_is_a_fixed_order_float64_sum(C, nblk):
    """vv_outconv_bwd_reduce on synthetic partials at mean 50 / std 1 (7 partial-sum lanes at C = 32, 3 at C = 64, two accumulators
    per lane striding by twice that): every written output within one float ulp of the float64 sum rounded to float -- which a
    sequential float32 accumulation of the nblk = 300 input misses (asserted on the CPU), so the bar tells the two apart."""
    L, lib = _L()
    nout, gs = 4 * C + 4, 4 * C + 4 + 8
    part = (50.0 + torch.randn(G, nblk, nout, generator=_gen(C, nblk, 9))).float()
    ref = part.double().sum(1).numpy()                                   # [G, nout]
    tol = _ulp32(ref)
    if nblk == 300:
        seq = np.cumsum(part.numpy(), axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        assert (np.abs(seq - ref.astype(np.float32)) > tol).any(), 'the input is too easy: raise the offset'
    pdev = torch.full((G * nblk * nout + SLACK,), SENT)
    pdev[:G * nblk * nout] = part.reshape(-1)
    pdev = pdev.cuda()
    oc = torch.tensor(OCS, dtype=torch.int32).cuda()
    grads = torch.full((G * gs + SLACK,), SENT, device='cuda')
    L.check(lib.vv_outconv_bwd_reduce(G, C, nblk, pdev.data_ptr(), oc.data_ptr(), grads.data_ptr(), grads.data_ptr() + 4 * 4 * C, gs,
                                      _st()), 'outconv_bwd_reduce')
    grads = grads.cpu()
    assert _sent(grads[G * gs:])
    grads = grads[:G * gs].view(G, gs)
    worst = 0.0
    for gi, n in enumerate(OCS):
        for lo, hi in ((0, n * C), (4 * C, 4 * C + n)):
            dev = np.abs(grads[gi, lo:hi].double().numpy() - ref[gi, lo:hi].astype(np.float32)) / tol[gi, lo:hi]
            worst = max(worst, dev.max())
        assert _sent(grads[gi, n * C:4 * C]) and _sent(grads[gi, 4 * C + n:])
    observe('outconv:reduce_fp64', ulps=worst)
    assert worst <= 1.0, worst


def test_output_conv_refusals_leave_the_outputs_untouched():
    """host-side early returns: the status, and not one sentinel changed; every pointer and size of every call is valid"""
    L, lib = _L()
    c = _case(64, 40, 1, OCS)          # buffers of a 64-channel case: larger than anything a 48-channel launch would touch
    d = _Dev(c, False, False)
    d16 = _Dev(c, True, False)
    out4, dout4, score = d.fwd_bufs()
    dA, part, bnp = d.bwd_bufs()
    grads = d.full(G * (4 * 64 + 4) + SLACK)
    din = torch.zeros(G * c.B * c.HW * 4, device='cuda')
    gs = d.dA_gs(dA)
    ptr = lambda t: t.data_ptr()

    def call_fwdbwd(dev, p, flags, mean=True, bn=True):
        return lib.vv_outconv_fwdbwd(C_.byref(p), ptr(dA), gs, ptr(part), ptr(dev.mean) if mean else None, ptr(dev.invstd),
                                     ptr(bnp) if bn else None, flags, _st())

    def call_bwd(C, mean=True):
        return lib.vv_outconv_bwd(G, c.B, c.HW, C, ptr(din), ptr(d.y), d.y_gs, ptr(d.a), ptr(d.b), c.abs_, ptr(d.prm), c.pgs, ptr(dA), gs,
                                  ptr(part), ptr(d.mean) if mean else None, ptr(d.invstd), ptr(bnp), 0, _st())

    p48 = d.params(L, out4, score, d.gscale, dout4)
    p48.C = 48
    assert lib.vv_outconv_fwd(C_.byref(p48), _st()) == UNSUPPORTED
    assert call_fwdbwd(d, p48, 0) == UNSUPPORTED
    p48b = d16.params(L, out4, score, d16.gscale, dout4)
    p48b.C = 48
    assert lib.vv_outconv_fwd(C_.byref(p48b), _st()) == UNSUPPORTED          # the eight-per-lane family
    assert call_fwdbwd(d16, p48b, 2) == UNSUPPORTED
    assert call_bwd(48) == UNSUPPORTED
    assert lib.vv_outconv_bwd_reduce(G, 48, c.B, ptr(part), ptr(d.oc), ptr(grads), ptr(grads) + 4 * 4 * 48, 4 * 48 + 4, _st()) == UNSUPPORTED
    # flags bit 1 != pad0 bit 0, both ways
    assert call_fwdbwd(d, d.params(L, out4, score, d.gscale, dout4), 2) == BAD_ARG
    assert call_fwdbwd(d16, d16.params(L, out4, score, d16.gscale, dout4), 0) == BAD_ARG
    # no gscale
    assert call_fwdbwd(d, d.params(L, out4, score, None, dout4), 0) == BAD_ARG
    # bnpart without mean
    assert call_fwdbwd(d, d.params(L, out4, score, d.gscale, dout4), 0, mean=False) == BAD_ARG
    assert call_bwd(64, mean=False) == BAD_ARG
    torch.cuda.synchronize()
    for t in (out4, dout4, score, dA, part, bnp, grads):
        assert _sent(t.cpu())


# ================================================================================================ vv_fold_bn

def test_fold_bn_against_float64():
    """G = 2, a parameter block of five conv + BatchNorm entries of which the table names three: (cout, row) = (32, 15 * 9),
    (64, 32 * 9) and (512, 256 * 9) -- 1.18 M filter elements, more than the 64 x 256 threads of the launch's first grid-stride step.
    running_var down to 1e-6, so eps decides a.  Folded filter within 2^-23 |ref64| elementwise: a is formed in double and rounded to
    float (relative error u / (1 + u), u = 2^-24), the product rounds once more, and (1 + u / (1 + u))^2 - 1 < 2 u.  Folded bias within
    one float ulp of the float64 value (formed in double, rounded once).  The restatement takes eps as the float the C ABI passes."""
    L, lib = _L()
    g = _gen(5, 1, 2)
    GG = 2
    shapes = [(32, 15 * 9), (32, 32 * 9), (64, 32 * 9), (16, 9), (512, 256 * 9)]
    named = (0, 2, 4)
    offs, off, boff = [], 0, 0
    for cout, row in shapes:
        e = NS(cout=cout, row=row, w=off, b=off + cout * row, g=off + cout * row + cout, beta=off + cout * row + 2 * cout, rm=boff, rv=boff + cout)
        off += cout * row + 3 * cout
        boff += 2 * cout
        offs.append(e)
    U, UB = off, boff
    pgs, fgs, bgs = U + 12, U + 20, UB + 4
    params = torch.randn(GG, pgs, generator=g) * 0.1
    bufs = torch.randn(GG, bgs, generator=g)
    for e in offs:
        params[:, e.g:e.g + e.cout] = torch.rand(GG, e.cout, generator=g) + 0.5
        params[:, e.b:e.b + e.cout] = torch.randn(GG, e.cout, generator=g)
        params[:, e.beta:e.beta + e.cout] = torch.randn(GG, e.cout, generator=g)
        rv = 10.0 ** (-6 * torch.rand(GG, e.cout, generator=g))
        rv[:, ::5] = 1e-6
        bufs[:, e.rv:e.rv + e.cout] = rv
    eps = float(np.float32(1e-5))
    ents = (L.FoldEntry * len(named))(*[L.FoldEntry(offs[i].w, offs[i].b, offs[i].g, offs[i].beta, offs[i].rm, offs[i].rv, offs[i].cout,
                                                     offs[i].row) for i in named])
    tab = torch.frombuffer(bytearray(bytes(ents)), dtype=torch.uint8).cuda()
    pd, bd = params.cuda(), bufs.cuda()
    folded = torch.full((GG, fgs), SENT, device='cuda')
    L.check(lib.vv_fold_bn(tab.data_ptr(), len(named), GG, pd.data_ptr(), pgs, bd.data_ptr(), bgs, eps, folded.data_ptr(), fgs, _st()), 'fold_bn')
    folded = folded.cpu()
    untouched = torch.ones(fgs, dtype=torch.bool)
    worst_w = worst_b = 0.0
    for i in named:
        e = offs[i]
        untouched[e.w:e.w + e.cout * e.row] = False
        untouched[e.b:e.b + e.cout] = False
        for gi in range(GG):
            P, Bf = params[gi].double(), bufs[gi].double()
            wf, bf = R.fold_bn(P[e.w:e.w + e.cout * e.row].view(e.cout, e.row), P[e.b:e.b + e.cout], P[e.g:e.g + e.cout],
                               P[e.beta:e.beta + e.cout], Bf[e.rm:e.rm + e.cout], Bf[e.rv:e.rv + e.cout], eps)
            dw = (folded[gi, e.w:e.w + e.cout * e.row].double() - wf.reshape(-1)).abs()
            worst_w = max(worst_w, (dw / wf.reshape(-1).abs().clamp_min(1e-300)).max().item() / 2.0 ** -23)
            assert bool((dw <= 2.0 ** -23 * wf.reshape(-1).abs()).all()), (i, gi)
            db = (folded[gi, e.b:e.b + e.cout].double() - bf).abs().numpy() / _ulp32(bf.numpy())
            worst_b = max(worst_b, db.max())
            assert db.max() <= 1.0, (i, gi, db.max())
    observe('outconv:fold_bn', weight_err_over_bar=worst_w, bias_ulps=worst_b)
    assert _sent(folded[:, untouched])          # the entries the table does not name, gamma / beta, the slack
