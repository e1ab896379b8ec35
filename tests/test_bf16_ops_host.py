"""Host checks (no GPU) of tests/bf16_ops_restatement.py, the reference tests/test_gpu_bf16_ops.py holds the bf16 convolution kernels
to: the restatement against torch autograd in float64, rn_bf16 around ties, the exactness of the float64 a x + b (TwoSum), and the
float32 evaluation of the GPU tests' own inputs, which has to sit inside the bars the kernels are held to (docs/bf16_ops_parity.md)."""
import pytest
import torch

import bf16_ops_restatement as R
from _util import gen


def _rne_bits(f32):
    """nearest-even float32 -> bf16 in integer arithmetic (finite values), independent of torch's conversion"""
    b = f32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(torch.float32)


def test_rn_bf16_neighbours_of_ties():
    """fp32 values that sit exactly half way between two bf16 numbers (even and odd lower neighbour, both signs, across a power of two,
    small and large exponents) and their +-1-ulp neighbours: rn_bf16 rounds the tie to even, the neighbours to their side -- a
    truncating or half-away conversion differs on every one of these triples"""
    ties = [1.00390625, 1.01171875, -1.00390625, -1.01171875, 1.99609375, 3.9921875, 255.5, 257.0, 259.0, 4088.0,
            2.0 ** -7 * 1.00390625, 2.0 ** -20 * 1.01171875, 2.0 ** 20 * 1.99609375, -2.0 ** 10 * 1.50390625, 1.50390625, 1.51171875]
    t = torch.tensor(ties, dtype=torch.float32)
    assert bool(((t.view(torch.int32) & 0xFFFF) == 0x8000).all())                    # every one IS a tie
    inf = torch.tensor(float('inf'))
    trip = torch.stack([torch.nextafter(t, -inf), t, torch.nextafter(t, inf)])
    got = R.rn_bf16(trip)
    assert torch.equal(got, _rne_bits(trip))
    lo = (t.view(torch.int32) & ~0xFFFF).view(torch.float32)                        # truncation = the neighbour towards zero
    hi = ((t.view(torch.int32) & ~0xFFFF) + 0x10000).view(torch.float32)            # the neighbour away from zero
    even_is_lo = ((t.view(torch.int32) >> 16) & 1) == 0
    assert torch.equal(got[1], torch.where(even_is_lo, lo, hi))
    below, above = got[0], got[2]                                                    # in magnitude: one ulp towards / away from zero
    neg = t < 0
    assert torch.equal(torch.where(neg, above, below), lo) and torch.equal(torch.where(neg, below, above), hi)
    assert bool((~even_is_lo).any()) and bool(even_is_lo.any())
    # float64 input is rounded to float32 first: a value a hair above the tie in float64 collapses onto it, as in the kernels
    d = t.double() * (1 + 2.0 ** -40)
    assert torch.equal(R.rn_bf16(d).float(), got[1])


def test_twosum_tells_exact_from_inexact():
    """200 000 draws, a in [0.5, 1.5), b ~ 0.2 N(0,1): bf16-valued x keeps a x + b exact in float64 (32-bit product), full fp32 x with
    24-bit a does not always, a and b on the 2^-12 grid do -- so fp32 sources get 12-bit a / b"""
    g = gen(200000)
    x = torch.randn(200000, generator=g)
    a = torch.rand(200000, generator=g) + 0.5
    b = torch.randn(200000, generator=g) * 0.2
    assert R.twosum_residual(a, R.rn_bf16(x), b).abs().max().item() == 0.0
    assert int((R.twosum_residual(a, x, b) != 0).sum()) > 0
    assert R.twosum_residual(R._grid12(a), x, R._grid12(b)).abs().max().item() == 0.0
    # and the exact value rounded once is what float64 -> float32 gives: compare with the fused form in exact rational arithmetic
    from fractions import Fraction
    xs, as_, bs = R.rn_bf16(x[:200]), a[:200], b[:200]
    once = (as_.double() * xs.double() + bs.double()).float()
    for i in range(200):
        exact = Fraction(float(as_[i])) * Fraction(float(xs[i])) + Fraction(float(bs[i]))
        assert Fraction(float((as_[i].double() * xs[i].double() + bs[i].double()))) == exact
        assert float(once[i]) == float(torch.tensor(float(exact), dtype=torch.float64).float())


def test_restatement_matches_autograd_float64():
    """conv3 / conv3_dgrad / wgrad3 against autograd of nn.Conv2d(k3, p1), convT_fwd / convT_dgrad / wgradT against autograd of
    nn.ConvTranspose2d(k3, s2, p1, op1), float64, on the operands the restatement itself produced"""
    g = gen(3, 1, 4)
    B, K, N, H = 3, 16, 32, 8
    x = torch.randn(B, K, H, H, generator=g)
    a, b = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2
    op = R.operand(R.rn_bf16(x), a, b, 'act')
    assert torch.equal(op, R.rn_bf16(op)) and op.dtype == torch.float64 and bool((op >= 0).all())
    cat = R.operand(R.rn_bf16(x[:, :8]), a[:8], b[:8], 'cat', R.rn_bf16(x[:, 8:]))
    assert torch.equal(cat[:, :8], op[:, :8]) and torch.equal(cat[:, 8:], R.rn_bf16(x[:, 8:]).double())
    w = torch.randn(N, K, 3, 3, generator=g) * 0.1
    bias = torch.randn(N, generator=g)
    conv = torch.nn.Conv2d(K, N, 3, padding=1).double()
    with torch.no_grad():
        conv.weight.copy_(R.rn_bf16(w).double())
        conv.bias.copy_(bias.double())
    xin = op.clone().requires_grad_(True)
    y = conv(xin)
    dy = R.rn_bf16(torch.randn(B, N, H, H, generator=g)).double()
    y.backward(dy)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.conv3(op, w, bias), y.detach(), **tol)
    torch.testing.assert_close(R.conv3(op, w, bias, relu=True), torch.relu(y.detach()), **tol)
    torch.testing.assert_close(R.conv3_dgrad(dy, w), xin.grad, **tol)
    torch.testing.assert_close(R.wgrad3(op, dy), conv.weight.grad, **tol)
    wt = torch.randn(K, N, 3, 3, generator=g) * 0.1
    ct = torch.nn.ConvTranspose2d(K, N, 3, stride=2, padding=1, output_padding=1).double()
    with torch.no_grad():
        ct.weight.copy_(R.rn_bf16(wt).double())
        ct.bias.copy_(bias.double())
    xin = op.clone().requires_grad_(True)
    y = ct(xin)
    dy2 = R.rn_bf16(torch.randn(B, N, 2 * H, 2 * H, generator=g)).double()
    y.backward(dy2)
    torch.testing.assert_close(R.convT_fwd(op, wt, bias), y.detach(), **tol)
    torch.testing.assert_close(R.convT_dgrad(dy2, wt), xin.grad, **tol)
    torch.testing.assert_close(R.wgradT(op, dy2), ct.weight.grad, **tol)
    # bn_partial_ref against autograd of BatchNorm's normalisation: dz = dA [a z + b > 0]; sum dz = d/d(shift), sum dz xhat = d/d(scale)
    z = torch.randn(B, N, H, H, generator=g).double()
    mean, invstd = torch.randn(N, generator=g).double() * 0.1, torch.rand(N, generator=g).double() + 0.5
    ba, bb = torch.rand(N, generator=g).double() + 0.5, torch.randn(N, generator=g).double() * 0.2
    gam = (ba / invstd).requires_grad_(True)
    bet = (bb + ba * mean).requires_grad_(True)      # gam xhat + bet == a z + b
    xhat = (z - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
    torch.relu(gam.view(1, -1, 1, 1) * xhat + bet.view(1, -1, 1, 1)).backward(dy)
    s1, s2 = R.bn_partial_ref(dy, z, ba, bb, mean, invstd)
    torch.testing.assert_close(s1, bet.grad, rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(s2, gam.grad, rtol=1e-9, atol=1e-9)


_DATA_CASES = [c for c in R.CONV_CASES if getattr(c, 'data_of', c.name) == c.name]      # (the VV_CONV_NO_RING twins share their data)


@pytest.mark.parametrize('group', ['E', 'R'])
@pytest.mark.parametrize('name', [c.name for c in _DATA_CASES])
def test_float32_restatement_inside_conv_bars(name, group):
    """the float32 evaluation of every convolution case of the GPU test, on the same inputs: a x + b exact (TwoSum residual 0); group E
    -- the bound below 2^24, float32 bit-equal to float64, the shares of rounded values and ties; group R -- the bf16-output bound and
    interval rule with the excused and differing caps"""
    c = R.CONV_BY_NAME[name]
    d, ref64, ref32, pre64 = R.conv_refs(c, group)
    assert R.conv_exact(c, d) == 0.0
    if group == 'E':
        assert R.exact_bound(c, d) < 2 ** 24
        assert torch.equal(ref32.double(), ref64)
        if c.out16:
            rounded, ties = R.tie_shares(ref64)
            assert rounded >= 0.25 and ties >= 0.01, (rounded, ties)
        return
    if c.out16:
        r = R.bf16_out_check(R.rn_bf16(ref32), ref64, ref32, pre64)
        assert r.ok, vars(r)
        assert r.excused <= R.EXCUSED_CAP and r.differing <= R.DIFFER_CAP, vars(r)
    else:
        e, e32 = R.eabs(ref32, ref64)
        assert e32 < 2.0 ** -20, e32                       # float32 summation of these sizes: a few 2^-24 of the maximum


@pytest.mark.parametrize('group', ['E', 'R'])
@pytest.mark.parametrize('name', [c.name for c in R.WGRAD_CASES])
def test_float32_restatement_inside_wgrad_bars(name, group):
    c = R.WGRAD_BY_NAME[name]
    assert R.wgrad_form(c) == c.form
    d, ref64, ref32 = R.wgrad_refs(c, group)
    assert R.wgrad_exact(c, d) == 0.0
    if group == 'E':
        # every partial sum is a multiple of 0.5 below 2^23: pixels * max|act| * max|dy|
        npx = c.B * (2 * c.H if c.kind == 'convT' else c.H) ** 2
        assert npx * 8 * 3 * 2 < 2 ** 24
        assert R.wgrad_exact_bound(c, d) <= npx * 8 * 3 * 2
        assert torch.equal(ref32.double(), ref64)
    else:
        assert R.eabs(ref32, ref64)[1] < 2.0 ** -18


def test_walk_cases_cross_what_they_claim():
    """the unit lists of the persistent workgroups (walk_info) at 256 CUs: every `:walk` case has a workgroup whose consecutive units
    belong to two UNets, every `:walk:nn` case also one whose consecutive units are two N tiles; with out1 the N tile cannot change
    inside a workgroup (NN is 1 or 2 and divides the stride of 32)"""
    seen = 0
    for c in R.GEMM16P:
        f = c.form.split(':')
        NI = {16: 1, 8: 4, 4: 16}[c.H]
        run, cross_g, cross_nn = R.walk_info(c.G, c.N // int(f[1][2:]), (c.B + NI - 1) // NI, 256)
        assert cross_g == ('walk' in f) and cross_nn == ('nn' in f), (c.name, run, cross_g, cross_nn)
        assert (run > 1) == ('walk' in f and 'nn' not in f)      # (NN = 3: a workgroup's two units are two N tiles, each a run of one)
        assert not (c.split and cross_nn)
        seen += 'nn' in f
    assert seen == 3
    # UnitStep's carry arithmetic against the plain decomposition of u
    for NN, NT, du in ((3, 45, 32), (2, 45, 32), (1, 90, 32), (3, 7, 5)):
        u = 1
        nn, pt, g = u % NN, (u // NN) % NT, u // (NN * NT)
        for _ in range(20):
            u += du
            nn += du % NN
            c1 = nn >= NN
            nn -= NN if c1 else 0
            pt += (du // NN) % NT + c1
            c2 = pt >= NT
            pt -= NT if c2 else 0
            g += (du // NN) // NT + c2
            assert (nn, pt, g) == (u % NN, (u // NN) % NT, u // (NN * NT))


def test_case_tables_name_every_form():
    """the forms the issue lists, each reached by a case whose dispatch condition the GPU test asserts (256 CUs: the MI355X)"""
    forms = {c.form for c in R.CONV_CASES}
    for c in R.CONV_CASES:
        assert R.expected_form(c, 256) == c.form, (c.name, R.expected_form(c, 256), c.form)
    for H in (16, 8, 4):
        lv = {c.form for c in R.GEMM16P if c.H == H}
        assert {f.split(':')[1] for f in lv} == {'TN128', 'TN64', 'TN32'}
        # a walk across a UNet boundary, and one whose workgroups also switch to another N tile
        assert any(f.endswith(':walk') for f in lv) and any(f.endswith(':walk:nn') for f in lv)
        # 32-wide tiles: the resident filter at CinP 64, 32 and 16, and the streamed one
        assert {f.split(':')[3] for f in lv if f.split(':')[1] == 'TN32'} == {'BRES64', 'BRES32', 'BRES16', 'BRES0'}, (H, lv)
        # Cout = 128 with a single chunk, which falls to 64-wide tiles
        assert any(c.N == 128 and c.form.split(':')[1] == 'TN64' for c in R.GEMM16P if c.H == H), H
        assert {f.split(':')[2] for f in lv} == ({'CK16'} if H == 4 else {'CK16', 'CK32'})
        assert {c.mode for c in R.GEMM16P if c.H == H} == {'plain', 'act', 'cat'}
    assert {'ring:KS1', 'ring:KS2', 'mfma:8x32x1:NR1:S16=3', 'mfma:8x32x1:NR2:S16=0', 'mfmaD:4x4x16:NR2:S16=1'} <= forms
    for s in (0, 1, 2):
        for tile in ('8x32x1', '8x16x1', '8x8x2', '4x4x8'):
            assert any(f.startswith('mfma:' + tile) and f.endswith('S16=%d' % s) for f in forms), (tile, s)
        for tile in ('16x16x1', '8x8x4', '4x4x16'):
            assert any(f.startswith('mfmaD:' + tile) and f.endswith('S16=%d' % s) for f in forms), (tile, s)
    assert {c.form for c in R.WGRAD_CASES} >= {'b:c1:o1', 'b:c2:o1', 'b:c1:o2', 'b:c2:o2', 'r:c1:o1', 'r:c2:o1', 'r:c1:o2', 'r:c2:o2',
                                              't:c1:o1', 't:c2:o1', 't:c1:o2', 't:c2:o2'}
