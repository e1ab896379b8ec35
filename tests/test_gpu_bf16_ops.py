"""The bf16 convolution kernels (vv_conv_mfma with VV_CONV_BF16: conv_mfma_kernel<.., BF>, conv_gemm16p_kernel, conv_ring16_kernel;
vv_wgrad_bf16 + vv_wgrad_reduce) against the float64 restatement of their EXACT bf16 operands (tests/bf16_ops_restatement.py), through
the C ABI.  Bars, cases and measurements: docs/bf16_ops_parity.md.

Every case runs with two groups of data: E (small integers: every product and partial sum is exact, so a kernel whose indexing is right
is BIT-EQUAL to the reference and the output rounding meets exact ties) and R (random: float-summation rule for fp32 outputs, the
bound and the interval rule for bf16 outputs).  Sources sit at coff = 8 inside wider pixels with random filler around them, the
destination is sentinel-filled, every launch is repeated with all filler redrawn and must give the same bits, and each case asserts
the launch form its shape selects."""
import ctypes as C

import pytest
import torch

import bf16_ops_restatement as R
from _util import SENT, bar, gen, observe

pytestmark = pytest.mark.gpu
FAM = 'bf16_ops'
KIND = {'conv3': 0, 'dgrad3': 0, 'convT_fwd': 1, 'convT_dgrad': 2}
PACK_MODE = {'conv3': 0, 'dgrad3': 1, 'convT_fwd': 2, 'convT_dgrad': 3}


def _L():
    from vec_vad_amd import _lib as L
    return L, L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack(L, lib, w, mode, K, N):
    """w [G, ...] in the nn layout of `mode` -> bf16 panels [G][9 K N / 2 floats]"""
    G = w.shape[0]
    w = w.contiguous().cuda()
    ent = (L.PackEntry * 1)(L.PackEntry(0, 0, mode | L.PACK_BF16, K, K, N))
    tab = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).cuda()
    out = torch.zeros(G, 9 * K * N, device='cuda')
    L.check(lib.vv_pack_weights(tab.data_ptr(), 1, G, w.data_ptr(), w[0].numel(), out.data_ptr(), out.stride(0), 9 * K * N, _stream()), 'pack')
    return out


def _src_buf(L, x, coff, pad, bf16, g):
    """x [Gs, B, C, H, W] -> NHWC channels [coff, coff + C) of pixels with cstride = C + pad; pad channels and 64 elements behind the
    buffer hold finite random numbers.  bf16: 2-byte elements, gstride still in floats.  Gs == 1: shared by all UNets (gstride 0)."""
    Gs, B, Cc, H, W = x.shape
    M, cs = B * H * W, Cc + pad
    n = M * cs + 64
    buf = torch.randn(Gs, n, generator=g)
    buf[:, :M * cs].view(Gs, M, cs)[:, :, coff:coff + Cc] = x.permute(0, 1, 3, 4, 2).reshape(Gs, M, Cc)
    dev = (buf.bfloat16() if bf16 else buf).cuda()
    gs = 0 if Gs == 1 else (n // 2 if bf16 else n)
    return dev, L.View(dev.data_ptr(), gs, cs, coff)


def _rows(t, g, pad=16):
    """[G, C] parameter rows with `pad` random floats behind every row: (device tensor, group stride)"""
    buf = torch.randn(t.shape[0], t.shape[1] + pad, generator=g)
    buf[:, :t.shape[1]] = t
    return buf.cuda(), t.shape[1] + pad


class _Out:
    """sentinel-filled destination: channels [coff, coff + C) of pixels with cstride = C + pad, 64 elements of slack"""

    def __init__(self, L, G, M, Cc, bf16, coff=8, pad=24, buf=None):
        self.G, self.M, self.C, self.cs, self.coff, self.bf16 = G, M, Cc, Cc + pad, coff, bf16
        n = M * self.cs + 64
        self.buf = torch.full((G, n), SENT, dtype=torch.bfloat16 if bf16 else torch.float32, device='cuda') if buf is None else buf
        self.view = L.View(self.buf.data_ptr(), n // 2 if bf16 else n, self.cs, coff)

    def get(self):
        """[G, M, C] float32 on the CPU (the stored values), after checking that everything else kept the sentinel bit for bit"""
        px = self.buf[:, :self.M * self.cs].view(self.G, self.M, self.cs)
        got = px[:, :, self.coff:self.coff + self.C].float().cpu()
        rest = self.buf.clone()
        rest[:, :self.M * self.cs].view(self.G, self.M, self.cs)[:, :, self.coff:self.coff + self.C] = SENT
        assert bool((rest == SENT).all()), 'written outside the promised channels'
        return got


def _setup_conv(L, lib, c, d, pk, rep):
    """parameter block + buffers of one launch of a case; all filler drawn from a generator seeded by `rep`"""
    g = gen(rep, 991, len(c.name))
    flags = R.conv_flags(c)
    src16 = c.src != 'f32'
    Hs, Ho = R.src_hw(c), R.out_hw(c)
    keep = []
    s0, v0 = _src_buf(L, d.x0, 8, 16, src16, g)
    keep.append(s0)
    v1 = L.NULL_VIEW
    if d.x1 is not None:
        s1, v1 = _src_buf(L, d.x1, 16, 32, src16, g)
        keep.append(s1)
    a = b = bias = None
    abg = bg = 0
    if d.a is not None:
        (a, abg), (b, _) = _rows(d.a, g), _rows(d.b, g)
    if d.bias is not None:
        bias, bg = _rows(d.bias, g, 8)
    M = c.B * Ho * Ho
    nt = lib.vv_conv_ntiles2(c.B, c.H, c.H, KIND[c.kind], flags)
    if c.split:
        cs = max(c.split, c.N - c.split) + 24              # the two views share the pixel and group strides
        both = torch.full((2, c.G, M * cs + 64), SENT, dtype=torch.bfloat16, device='cuda')
        outs = [_Out(L, c.G, M, c.split, True, pad=cs - c.split, buf=both[0]),
                _Out(L, c.G, M, c.N - c.split, True, pad=cs - (c.N - c.split), buf=both[1])]
        keep.append(both)
    else:
        outs = [_Out(L, c.G, M, c.N, c.out16)]
    rows = nt if not c.bnf else lib.vv_conv_ntiles(c.B, c.H, c.H)
    sbuf = torch.full((c.G * rows * 2 * c.N + 4 * c.N,), SENT, device='cuda') if (c.stats or c.bnf) else None
    cp = L.ConvParams(KIND[c.kind], R.MODES[c.mode], c.G, c.B, c.H, c.H, c.K, c.K, c.N, v0, a.data_ptr() if a is not None else None,
                      b.data_ptr() if b is not None else None, abg, v1, c.csplit, flags, None, pk.data_ptr(), pk.stride(0),
                      bias.data_ptr() if bias is not None else None, bg, outs[0].view, sbuf.data_ptr() if c.stats else None)
    if c.split:
        cp.out1, cp.osplit = outs[1].view, c.split
    if c.bnf:
        z, zv = _src_buf(L, d.z, 0, 0, True, g)            # [G][B H W][Cout], pixel stride Cout, bf16 elements
        bn = [_rows(t, g) for t in d.bn]
        keep += [z] + [t for t, _ in bn]
        cp.bn_z, cp.bn_z_gstride = z.data_ptr(), zv.gstride
        cp.bn_a, cp.bn_b, cp.bn_mean, cp.bn_invstd = (t.data_ptr() for t, _ in bn)
        cp.bn_gstride, cp.bn_partial = bn[0][1], sbuf.data_ptr()
    keep += [a, b, bias]
    return cp, outs, sbuf, rows, keep


def _run_conv(L, lib, c, d, pk, rep):
    cp, outs, sbuf, rows, keep = _setup_conv(L, lib, c, d, pk, rep)
    L.check(lib.vv_conv_mfma(C.byref(cp), _stream()), c.name)
    torch.cuda.synchronize()
    Ho = R.out_hw(c)
    got = torch.cat([o.get() for o in outs], 2).view(c.G, c.B, Ho, Ho, c.N).permute(0, 1, 4, 2, 3).contiguous()
    st = None
    if sbuf is not None:
        n = c.G * rows * 2 * c.N
        assert bool((sbuf[n:] == SENT).all()), 'rows behind the tiles of the launch were written'
        st = sbuf[:n].view(c.G, rows, 2, c.N).cpu()
    del keep
    return got, st


def _max_run(c, ncu):
    """tiles a workgroup of conv_gemm16p_kernel can fold into one stats row (bf16_ops_restatement.walk_info); every other kernel writes
    one row per tile"""
    f = c.form.split(':')
    if f[0] != 'p':
        return 1
    NI = {16: 1, 8: 4, 4: 16}[c.H]
    return R.walk_info(c.G, c.N // int(f[1][2:]), (c.B + NI - 1) // NI, ncu)[0]


def _check_conv(c, group):
    L, lib = _L()
    ncu = lib.vv_num_cus()
    # the dispatch condition this case is meant to reach, restated from the C++ in bf16_ops_restatement.expected_form (with the line
    # numbers it was read from)
    assert R.expected_form(c, ncu) == c.form, (R.expected_form(c, ncu), c.form)
    d, ref64, ref32, pre64 = R.conv_refs(c, group)
    assert R.conv_exact(c, d) == 0.0                     # a x + b exact in float64: the operand is reproduced exactly
    pk = _pack(L, lib, d.w, PACK_MODE[c.kind], c.K, c.N)
    got, st = _run_conv(L, lib, c, d, pk, 0)
    got2, st2 = _run_conv(L, lib, c, d, pk, 1)           # all filler and slack redrawn: the same bits
    assert torch.equal(got.view(torch.int32), got2.view(torch.int32))
    if st is not None:
        assert torch.equal(st.view(torch.int32), st2.view(torch.int32))
    del got2, st2
    got64 = got.double()
    op = '%s:%s' % (c.name, group)
    want = R.rn_bf16(ref64) if c.out16 else ref64
    if group == 'E':
        assert R.exact_bound(c, d) < 2 ** 24
        neq = int((got64 != want).sum())
        rounded, ties = R.tie_shares(ref64) if c.out16 else (0.0, 0.0)
        observe(FAM + ':' + op, bit_equal=got64.numel() - neq, elements=got64.numel(), rounded=rounded, ties=ties)
        assert neq == 0, (op, neq, (got64 - want).abs().max().item())
        if c.out16:
            assert rounded >= 0.25 and ties >= 0.01, (rounded, ties)
    elif c.out16:
        r = R.bf16_out_check(got64, ref64, ref32, pre64)
        observe(FAM + ':' + op, err_hip=r.err_hip, err_ref32=r.err_ref32, excused=r.excused, differing=r.differing)
        assert r.bound_ok, (op, 'bound', vars(r))
        assert r.inside, (op, 'interval', vars(r))
        assert r.excused <= R.EXCUSED_CAP and r.differing <= R.DIFFER_CAP, (op, vars(r))
    else:
        bar(op, 'out', got, ref64, ref32, family=FAM)
    if c.stats:
        tot = st.double().sum(1)                           # rows summed over the tiles in float64: [G, 2, N]
        s64, q64 = got64.sum((1, 3, 4)), (got64 * got64).sum((1, 3, 4))
        exact = group == 'E' and 2 * _max_run(c, ncu) * 256 * got64.abs().max().item() < 2 ** 24
        if exact:                                          # every per-workgroup sum of (half-)integers stays below 2^24: exact
            assert torch.equal(tot[:, 0], s64), (op, (tot[:, 0] - s64).abs().max().item())
        else:
            bar(op + ':stats_sum', 'sum', tot[:, 0], s64, got.sum((1, 3, 4)), family=FAM)
        bar(op + ':stats_sq', 'sum of squares', tot[:, 1], q64, (got * got).sum((1, 3, 4)), family=FAM)
    if c.bnf:
        tot = st.double().sum(1)
        for dt, acc in ((torch.float64, []), (torch.float32, [])):
            for gi in range(c.G):
                acc.append(torch.stack(R.bn_partial_ref(got[gi], d.z[gi], *[t[gi] for t in d.bn], dtype=dt)))
            if dt == torch.float64:
                b64 = torch.stack(acc)
            else:
                b32 = torch.stack(acc)
        bar(op + ':bn_sum_dz', 'sum dz', tot[:, 0], b64[:, 0], b32[:, 0], family=FAM)
        bar(op + ':bn_sum_dz_xhat', 'sum dz xhat', tot[:, 1], b64[:, 1], b32[:, 1], family=FAM)


@pytest.mark.parametrize('group', ['E', 'R'])
@pytest.mark.parametrize('name', [c.name for c in R.GEMM16P])
def test_bf16_gemm16p_matches_float64_of_exact_operands(name, group):
    """conv_gemm16p_kernel: every N-tile width, chunk size, resident / streamed filter on the three levels it serves, all three input
    modes, ragged batches, and per level one launch with more units than workgroups (G NN NT > ncu, not a multiple of 8), so that
    workgroups walk several tiles and carry their column sums across them: across a UNet boundary with stats, with out1 / osplit (N
    tile inside a half, and spanning both halves) and with VV_CONV_RELU (`:walk`), and across an N-tile boundary with three N tiles
    (`:walk:nn`; with out1 the N tile cannot change inside a workgroup, see docs/bf16_ops_parity.md)"""
    _check_conv(R.CONV_BY_NAME[name], group)


@pytest.mark.parametrize('group', ['E', 'R'])
@pytest.mark.parametrize('name', [c.name for c in R.RING])
def test_bf16_ring_and_its_twin_match_float64_of_exact_operands(name, group):
    """conv_ring16_kernel and, with VV_CONV_NO_RING, conv_mfma_kernel<8, 32, 1, 1, VV_CONV3, 16, true, 2 | 3> on the same inputs: each
    against the reference, not only against each other -- output, stats, the fused BatchNorm-backward sums (against bn_partial_ref on
    the dA the launch stored) and VV_CONV_RELU"""
    _check_conv(R.CONV_BY_NAME[name], group)


@pytest.mark.parametrize('group', ['E', 'R'])
@pytest.mark.parametrize('name', [c.name for c in R.MFMA])
def test_bf16_conv_mfma_matches_float64_of_exact_operands(name, group):
    """conv_mfma_kernel<.., BF = true>: VV_CONV3 forward and data gradient with fp32 tensors (S16 = 0), VV_CONV_SRC_BF16 (1) and all-bf16
    tensors under VV_CONV_NO_GEMM16 (2) on all four levels, fp32 and bf16 output; VV_CONVT_FWD and VV_CONVT_DGRAD on 16 / 8 / 4; the
    `wide` forms"""
    _check_conv(R.CONV_BY_NAME[name], group)


# ------------------------------------------------------------------------------------------------------ weight gradient
def _run_wgrad(L, lib, c, d, rep):
    g = gen(rep, 577, len(c.name))
    kind = L.CONV3 if c.kind == 'conv3' else L.CONVT_FWD
    flags = (L.WGRAD_X_BF16 | L.WGRAD_DY_BF16) if c.ring else 0
    nt, nblk, kw = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.vv_wgrad_bf16_plan(kind | (flags << 8), c.B, c.H, c.H, c.CinP, c.Cout, C.byref(nt), C.byref(nblk), C.byref(kw)) == 1
    ks = {1: 1, 'mid': min(max(2, nt.value // 2), nt.value), 'all': nt.value}[c.ks]
    s0, v0 = _src_buf(L, d.x0, 8, 16, c.ring, g)
    v1 = L.NULL_VIEW
    if d.x1 is not None:
        s1, v1 = _src_buf(L, d.x1, 16, 32, c.ring, g)
    dyb, vdy = _src_buf(L, d.dy, 8, 16, c.ring, g)         # dy at coff != 0
    a = b = None
    abg = 0
    if d.a is not None:
        (a, abg), (b, _) = _rows(d.a, g), _rows(d.b, g)
    nci, nco = (c.CinP + 31) // 32, c.Cout // 32
    n = nci * nco * ks * kw.value * 9 * 1024
    part = torch.full((c.G, n + 9 * 1024), SENT, device='cuda')      # one slab more than the plan names, per UNet
    ng = c.Cout * c.Cin * 9
    grad = torch.full((c.G, ng + 64), SENT, device='cuda')
    wp = L.WgradParams(kind, R.MODES[c.mode], c.G, c.B, c.H, c.H, c.Cin, c.CinP, c.Cout, ks, v0, a.data_ptr() if a is not None else None,
                       b.data_ptr() if b is not None else None, abg, v1, c.csplit, flags, None, vdy, part.data_ptr(), part.stride(0))
    L.check(lib.vv_wgrad_bf16(C.byref(wp), _stream()), c.name)
    L.check(lib.vv_wgrad_reduce(kind, c.G, c.Cin, c.CinP, c.Cout, ks * kw.value, part.data_ptr(), part.stride(0), grad.data_ptr(),
                                grad.stride(0), _stream()), 'reduce')
    torch.cuda.synchronize()
    assert bool((part[:, n:] == SENT).all()), 'a slab the plan does not name was written'
    assert bool((grad[:, ng:] == SENT).all())
    shape = (c.G, c.Cout, c.Cin, 3, 3) if c.kind == 'conv3' else (c.G, c.Cin, c.Cout, 3, 3)
    return grad[:, :ng].cpu().view(shape), ks, nt.value


@pytest.mark.parametrize('group', ['E', 'R'])
@pytest.mark.parametrize('name', [c.name for c in R.WGRAD_CASES])
def test_bf16_weight_gradient_matches_float64_of_exact_operands(name, group):
    """vv_wgrad_bf16 + vv_wgrad_reduce: the tile form (fp32 tensors, launch_b), the ring form (bf16 tensors, launch_r) and the
    transposed form (launch_t) in every block shape, ksplit 1 / a middle value / ntiles, zero-padded input channels, ragged batches,
    ACT / CAT / PLAIN inputs, dy at coff != 0.  Group E: the reduced gradient is bit-equal; group R: every entry within the
    float-summation rule."""
    L, lib = _L()
    c = R.WGRAD_BY_NAME[name]
    assert R.wgrad_form(c) == c.form                         # the launch form, restated from the C++ (wgrad_form's docstring)
    d, ref64, ref32 = R.wgrad_refs(c, group)
    assert R.wgrad_exact(c, d) == 0.0
    if group == 'E':      # the partial-sum bound on this test's own inputs: every partial sum is a multiple of 0.5 below 2^23
        assert R.wgrad_exact_bound(c, d) < 2 ** 24
    got, ks, nt = _run_wgrad(L, lib, c, d, 0)
    got2, _, _ = _run_wgrad(L, lib, c, d, 1)
    assert torch.equal(got.view(torch.int32), got2.view(torch.int32))
    assert 1 <= ks <= nt and (c.ks != 'mid' or nt < 3 or 1 < ks < nt)
    op = '%s:%s' % (c.name, group)
    if group == 'E':
        neq = int((got.double() != ref64).sum())
        observe(FAM + ':' + op, bit_equal=got.numel() - neq, elements=got.numel())
        assert neq == 0, (op, neq, (got.double() - ref64).abs().max().item())
    else:
        bar(op, 'dW', got, ref64, ref32, family=FAM)


# ---------------------------------------------------------------------------------------------------------- refused calls
BAD_ARG, UNSUPPORTED = 1, 3


def _refuse(c, status, mutate):
    """the launch of an otherwise valid case with one field changed is refused with `status`, and nothing is written"""
    L, lib = _L()
    d = R.conv_data(c, 'E')
    pk = _pack(L, lib, d.w, PACK_MODE[c.kind], c.K, c.N)
    cp, outs, sbuf, rows, keep = _setup_conv(L, lib, c, d, pk, 0)
    extra = mutate(L, cp, outs)
    assert lib.vv_conv_mfma(C.byref(cp), _stream()) == status
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o.buf == SENT).all())
    if sbuf is not None:
        assert bool((sbuf == SENT).all())
    del keep, extra


def _set(**kw):
    def m(L, cp, outs):
        for k, v in kw.items():
            setattr(cp, k, v)
    return m


def _coff(which, coff):
    def m(L, cp, outs):
        v = getattr(cp, which)
        setattr(cp, which, L.View(v.ptr, v.gstride, v.cstride, coff))
    return m


def _stride(which, cs):
    def m(L, cp, outs):
        v = getattr(cp, which)
        setattr(cp, which, L.View(v.ptr, v.gstride, cs, v.coff))
    return m


_F32 = R.conv_case('ref_f32', 'conv3', 16, 2, 32, 32, 'act', src='f32', out16=False, stats=True)
_F32T = R.conv_case('ref_f32t', 'convT_fwd', 8, 2, 32, 32, 'plain', src='f32', out16=False)
_SRC = R.conv_case('ref_src', 'dgrad3', 16, 2, 32, 32, 'plain', src='src16', out16=False)
_ALL = R.conv_case('ref_all', 'conv3', 16, 2, 32, 64, 'plain', stats=True)
_BNF = R.conv_case('ref_bnf', 'dgrad3', 32, 2, 16, 32, 'plain', bnf=True)
_BNF64 = R.conv_case('ref_bnf64', 'dgrad3', 32, 2, 16, 64, 'plain', bnf=True)
_BNF16 = R.conv_case('ref_bnf16', 'dgrad3', 16, 2, 16, 32, 'plain', bnf=True)
_SPL = R.conv_case('ref_spl', 'dgrad3', 16, 2, 32, 64, 'plain', split=32)
_SPL96 = R.conv_case('ref_spl96', 'dgrad3', 16, 2, 32, 96, 'plain', split=32)
_SPL192 = R.conv_case('ref_spl192', 'dgrad3', 16, 2, 32, 192, 'plain', split=96)
_O16 = R.conv_case('ref_o16', 'dgrad3', 16, 2, 32, 64, 'plain', src='src16', out16=True, extra=R.CONV_NO_GEMM16)
_O16T = R.conv_case('ref_o16t', 'convT_dgrad', 8, 2, 32, 32, 'plain', src='src16', out16=True)
_O16R = R.conv_case('ref_o16r', 'conv3', 32, 2, 48, 32, 'plain')
_SPLF = R.conv_case('ref_splf', 'dgrad3', 32, 2, 32, 64, 'plain', split=32)


def _fp32_out_with_out1(L, cp, outs):
    cp.pad0 &= ~L.CONV_OUT_BF16


def _stats_on(L, cp, outs):
    t = torch.full((4096,), SENT, device='cuda')
    cp.stats = t.data_ptr()
    return t


@pytest.mark.parametrize('what,case,status,mutate', [
    ('OUT_BF16 without BF16', _F32, BAD_ARG, _set(pad0=R.CONV_OUT_BF16)),
    ('SRC_BF16 with ACT', _F32, BAD_ARG, _set(pad0=R.CONV_BF16 | R.CONV_SRC_BF16)),
    ('SRC_BF16 with CONVT_FWD', _F32T, BAD_ARG, _set(pad0=R.CONV_BF16 | R.CONV_SRC_BF16)),
    ('SRC_BF16 with odd coff', _SRC, BAD_ARG, _coff('src0', 7)),
    ('ALLSRC_BF16 with POOL', _ALL, BAD_ARG, _set(in_mode=2)),
    ('ALLSRC_BF16 with CUBE', _ALL, BAD_ARG, _set(in_mode=4)),
    ('bn_partial with stats', _BNF, UNSUPPORTED, _stats_on),
    ('bn_partial with Cout % 64 == 0', _BNF64, UNSUPPORTED, _set()),
    ('bn_partial below 32x32', _BNF16, UNSUPPORTED, _set()),
    ('out1 with fp32 output', _SPLF, UNSUPPORTED, _fp32_out_with_out1),
    ('out1 with osplit % 32 != 0', _SPL, BAD_ARG, _set(osplit=16)),
    ('out1 with another pixel stride', _SPL, BAD_ARG, _stride('out1', 64)),
    ('out1 with Cout != 2 osplit on the GEMM-shaped kernel', _SPL96, UNSUPPORTED, _set()),
    ('out1 with a non-power-of-two osplit on the GEMM-shaped kernel', _SPL192, UNSUPPORTED, _set()),
    ('bf16 tile output with out.coff % 8 != 0 (conv_mfma_kernel, VV_CONV3)', _O16, BAD_ARG, _coff('out', 4)),
    ('bf16 tile output with out.cstride % 8 != 0 (conv_mfma_kernel, VV_CONVT_DGRAD)', _O16T, BAD_ARG, _stride('out', 60)),
    ('bf16 tile output with out.coff % 8 != 0 at 32x32', _O16R, BAD_ARG, _coff('out', 12)),
    ('misaligned src0.coff on vv_conv_gemm16', _ALL, BAD_ARG, _coff('src0', 4)),
    ('misaligned out.cstride on vv_conv_gemm16', _ALL, BAD_ARG, _stride('out', 92)),
], ids=lambda v: v.replace(' ', '_') if isinstance(v, str) else None)
def test_bf16_conv_refused_calls(what, case, status, mutate):
    """the calls the bf16 flags refuse (vv_conv_mfma's argument checks in vv_conv.hip, vv_conv_gemm16's in vv_conv_bf16.hip): the status,
    and nothing written"""
    _refuse(case, status, mutate)


def test_bf16_wgrad_refused_calls():
    """VV_WGRAD_X_BF16 without VV_WGRAD_DY_BF16; ksplit > ntiles (vv_wgrad_bf16.hip:924, launch_b / launch_r / launch_t)"""
    L, lib = _L()
    for ring, kindname, H in ((False, 'conv3', 16), (True, 'conv3', 16), (False, 'convT', 8)):
        c = R.wgrad_case('ref_w', kindname, H, 2, 32, 32, 32, 1, 'plain', ring=ring)
        d = R.wgrad_data(c, 'E')
        g = gen(5)
        kind = L.CONV3 if kindname == 'conv3' else L.CONVT_FWD
        flags = (L.WGRAD_X_BF16 | L.WGRAD_DY_BF16) if ring else 0
        nt = C.c_int32()
        assert lib.vv_wgrad_bf16_plan(kind | (flags << 8), c.B, c.H, c.H, c.CinP, c.Cout, C.byref(nt), None, None) == 1
        s0, v0 = _src_buf(L, d.x0, 8, 16, ring, g)
        dyb, vdy = _src_buf(L, d.dy, 8, 16, ring, g)
        part = torch.full((c.G, (nt.value + 2) * 9 * 1024), SENT, device='cuda')
        for ks, fl, status in ((nt.value + 1, flags, BAD_ARG), (1, L.WGRAD_X_BF16, UNSUPPORTED)):
            wp = L.WgradParams(kind, L.IN_PLAIN, c.G, c.B, c.H, c.H, c.Cin, c.CinP, c.Cout, ks, v0, None, None, 0, L.NULL_VIEW, c.CinP, fl,
                               None, vdy, part.data_ptr(), part.stride(0))
            assert lib.vv_wgrad_bf16(C.byref(wp), _stream()) == status, (ring, kindname, ks, fl)
            torch.cuda.synchronize()
            assert bool((part == SENT).all())
