"""tests/flownet2_f16_ops_restatement.py on the CPU (no GPU): the convolutions against torch.nn.functional in float64 on half-rounded
operands, the whole layer bit for bit against the half graph of tests/test_flownet2_fp16.py, the layouts against the header's index
formulas element by element, the edges of rn_f16 and the double rounding of act_out_f16, the dispatch restatements against the case
tables of tests/test_gpu_flownet2_f16_ops.py, and torch's float32 evaluation of every GPU case inside every bar and cap of that module."""
import pytest
import torch
import torch.nn.functional as F

import flownet2_f16_ops_restatement as R
import test_gpu_flownet2_f16_ops as G
from _util import gen
from test_flownet2_fp16 import _half_layer_ref

H16 = torch.float16


def _h(v):
    return torch.tensor(v, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ convolutions
CONV = [(False, 1, 1, 2, 5, 7, 19, 6), (False, 3, 1, 2, 6, 9, 5, 7), (False, 3, 2, 3, 11, 14, 19, 5), (False, 3, 2, 1, 12, 13, 7, 4),
        (False, 5, 2, 2, 9, 10, 3, 6), (False, 7, 2, 2, 21, 22, 3, 8), (True, 4, 2, 2, 4, 6, 2, 2), (True, 4, 2, 3, 5, 7, 19, 6)]


@pytest.mark.parametrize('de,Rk,stride,B,H,W,Cin,Cout', CONV)
def test_pre64_vs_torch_float64_on_half_rounded_operands(de, Rk, stride, B, H, W, Cin, Cout):
    g = gen(de, Rk, stride, B, H, W, Cin, Cout)
    x = torch.randn(B, H, W, Cin, generator=g).half()
    w = torch.randn(*((Cin, Cout, 4, 4) if de else (Cout, Cin, Rk, Rk)), generator=g).half()
    bias = torch.randn(Cout, generator=g)                      # fp32, not fp16-representable: added unrounded
    xn = x.double().permute(0, 3, 1, 2)
    if de:
        ref = F.conv_transpose2d(xn, w.double(), bias.double(), stride=2, padding=1)
    else:
        ref = F.conv2d(xn, w.double(), bias.double(), stride=stride, padding=(Rk - 1) // 2)
    got = R.pre64(de, x, w, bias, stride)
    ref = ref.permute(0, 2, 3, 1)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize('de,Rk,stride,B,H,W,Cin,Cout', CONV)
@pytest.mark.parametrize('relu', [True, False])
def test_layer_bit_equal_to_the_half_graph(de, Rk, stride, B, H, W, Cin, Cout, relu):
    """integer operands: the float64 accumulation _half_layer_ref uses for the kernel's fp32 one is exact, and so is ours; biases that
    push the sums past 2048 so both roundings run"""
    g = gen(de, Rk, stride, B, H, W, Cin, Cout, relu)
    x = torch.randint(-3, 4, (B, H, W, Cin), generator=g).half()
    w = torch.randint(-2, 3, (Cin, Cout, 4, 4) if de else (Cout, Cin, Rk, Rk), generator=g).float()
    bias = torch.randint(2500, 6001, (Cout,), generator=g).float() * (1 - 2 * (torch.arange(Cout) % 2))      # signs alternate
    bias = (bias / 4).round() * 4                         # fp16 holds multiples of 4 up to 8192: _half_layer_ref rounds the bias
    ref, _ = _half_layer_ref('deconv' if de else 'conv', x.permute(0, 3, 1, 2), w, bias, stride, Rk, relu)
    got = R.act_out_f16(R.pre64(de, x, w.half(), bias, stride), 0.1 if relu else 1.0)
    assert torch.equal(got.view(torch.int16), ref.permute(0, 2, 3, 1).contiguous().view(torch.int16))
    assert float(ref.float().abs().max()) > 2048 and bool((ref < 0).any())


# ------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize('transposed', [0, 1])
def test_panel_layout_f16(transposed):
    """every element against the header's formula: [taps][KP/8][NP][8], k = kq * 8 + j; padding zero; values rn_f16(w)"""
    K, KP, N, NP, Rk = 11, 16, 35, 64, 4 if transposed else 3
    g = gen(K, N, transposed)
    w = torch.randn(*((K, N) if transposed else (N, K)), Rk, Rk, generator=g)
    p = R.pack_panel_f16(w, KP, NP, transposed)
    assert p.dtype == H16 and p.numel() == Rk * Rk * KP * NP
    for tap in range(Rk * Rk):
        ky, kx = divmod(tap, Rk)
        for k in range(KP):
            for n in range(NP):
                v = p[((tap * (KP // 8) + k // 8) * NP + n) * 8 + k % 8]
                if k < K and n < N:
                    want = (w[k, n, ky, kx] if transposed else w[n, k, ky, kx]).half()
                    assert v.view(torch.int16) == want.view(torch.int16)
                else:
                    assert v.view(torch.int16) == 0


@pytest.mark.parametrize('Rk,Cin,KP', [(7, 3, 64), (3, 6, 32)])
def test_row_k_layout_f16(Rk, Cin, KP):
    """8-half pixels: [N][kx * 8 + c][ky]; zero at the pad channels c >= Cin and from k = R * 8 on"""
    g = gen(Rk, Cin, KP)
    w = torch.randn(5, Cin, Rk, Rk, generator=g)
    r = R.rowk_weight_f16(w)
    assert tuple(r.shape) == (5, KP, Rk)
    for n in range(5):
        for k in range(KP):
            kx, c = divmod(k, 8)
            for ky in range(Rk):
                assert r[n, k, ky] == (w[n, c, ky, kx] if kx < Rk and c < Cin else 0)


# ------------------------------------------------------------------------------------------------ rn_f16, act_out_f16
def test_rn_f16_ties_subnormals_and_overflow():
    u = 2.0 ** -10                                             # fp16 spacing in [1, 2)
    eps = 2.0 ** -20                                          # well above float32's spacing: the first rounding keeps the side
    for v, below, at, above in [(1 + u / 2, 1.0, 1.0, 1 + u),                  # tie between 1 (even) and 1 + u
                                (1 + 3 * u / 2, 1 + u, 1 + 2 * u, 1 + 2 * u),  # tie between 1 + u (odd) and 1 + 2u
                                (2049.0, 2048.0, 2048.0, 2050.0), (2051.0, 2050.0, 2052.0, 2052.0), (-2049.0, -2050.0, -2048.0, -2048.0),
                                (4098.0, 4096.0, 4096.0, 4100.0), (4102.0, 4100.0, 4104.0, 4104.0)]:
        s = abs(v) * eps
        assert float(R.rn_f16(_h(v - s))) == below and float(R.rn_f16(_h(v))) == at and float(R.rn_f16(_h(v + s))) == above, v
    # subnormals: multiples of 2^-24 below 2^-14 are kept, odd multiples of 2^-25 are ties to even
    m = torch.arange(0, 2048, dtype=torch.float64)
    assert torch.equal(R.rn_f16(m * 2.0 ** -24).double(), m * 2.0 ** -24)
    odd = torch.arange(1, 2048, 2, dtype=torch.float64)       # ties at odd * 2^-25 between (odd - 1) / 2 and (odd + 1) / 2
    want = torch.where(((odd - 1) / 2) % 2 == 0, (odd - 1) / 2, (odd + 1) / 2) * 2.0 ** -24
    assert torch.equal(R.rn_f16(odd * 2.0 ** -25).double(), want)
    assert torch.equal(R.rn_f16(-odd * 2.0 ** -25).double(), -want)
    assert torch.equal(R.rn_f16(odd * 2.0 ** -25 * (1 + 2.0 ** -20)).double(), (odd + 1) / 2 * 2.0 ** -24)
    assert torch.equal(R.rn_f16(odd * 2.0 ** -25 * (1 - 2.0 ** -20)).double(), (odd - 1) / 2 * 2.0 ** -24)
    # overflow edge: 65520 is the tie between 65504 and 2^16
    assert float(R.rn_f16(_h(65519.0))) == 65504.0 and float(R.rn_f16(_h(65519.99))) == 65504.0
    assert float(R.rn_f16(_h(65520.0))) == float('inf') and float(R.rn_f16(_h(-65520.0))) == float('-inf')
    assert float(R.rn_f16(_h(65504.0))) == 65504.0
    # ONE rounding to float32 first: 1 + u/2 + 2^-40 is above the tie in float64, on it in float32
    assert float(R.rn_f16(_h(1 + u / 2 + 2.0 ** -40))) == 1.0


def test_act_out_f16_rounds_before_and_after_the_leaky_relu():
    s = float(torch.tensor(0.1, dtype=torch.float32))
    # -2049: first rounding -> -2048, times 0.1f = -204.80000305..., -> -204.75 (spacing 0.125 in [128, 256))
    assert float(R.act_out_f16(_h(-2049.0), 0.1)) == -204.75
    # -2051 -> -2052 -> -205.2000... -> -205.25; without the first rounding -205.1000... -> -205.125
    assert float(R.act_out_f16(_h(-2051.0), 0.1)) == -205.25
    assert float(R.rn_f16(_h(-2051.0 * s))) == -205.125
    # positive values are rounded once, slope 1 leaves the rounded value
    assert float(R.act_out_f16(_h(2051.0), 0.1)) == 2052.0 and float(R.act_out_f16(_h(-2051.0), 1.0)) == -2052.0
    assert float(R.act_out_f16(_h(-65520.0), 0.1)) == float('-inf') and float(R.act_out_f16(_h(65520.0), 0.1)) == float('inf')
    z = R.act_out_f16(_h([0.0, -3 * 2.0 ** -24]), 0.1)
    assert float(z[0]) == 0 and float(z[1]) == 0                   # 0.3 * 2^-24 rounds to zero
    # the fp32 product is rounded before the second fp16 rounding: against the exact product rounded once
    r = torch.arange(-4096, 0, dtype=torch.float64)
    twice = R.act_out_f16(r, 0.1)
    assert torch.equal(twice, (R.rn_f16(r).float() * torch.tensor(0.1)).half())
    assert torch.equal(twice, _half_layer_ref('conv', r.half().view(1, 1, 1, -1), torch.ones(1, 1, 1, 1), None, 1, 1, True)[0].view(-1))


def test_splitk_finish_f16_is_the_fixed_order_float32_sum():
    g = gen(5, 7)
    ws = torch.randn(3 * 10 * 32 + 64, generator=g) * 1000
    bias = torch.randn(24, generator=g)
    v = bias.expand(10, 24).clone()
    for k in range(3):
        v += ws[k * 320:(k + 1) * 320].view(10, 32)[:, :24]
    assert torch.equal(R.splitk_finish_f16(ws, 3, 10, 24, 32, bias, 0.1), R.act_out_f16(v.double(), 0.1))
    rev = bias.expand(10, 24).clone()
    for k in (2, 1, 0):
        rev += ws[k * 320:(k + 1) * 320].view(10, 32)[:, :24]
    assert not torch.equal(v, rev)                                 # the order is visible in float32
    # the GPU test's own workspace: the reverse order changes more than a tenth of the fp16 results
    ws, ks, M, Cout, CoutP, bias, slope = G.finish_case()
    flipped = ws.view(ks, M, CoutP).flip(0).reshape(-1)
    a, b = R.splitk_finish_f16(ws, ks, M, Cout, CoutP, bias, slope), R.splitk_finish_f16(flipped, ks, M, Cout, CoutP, bias, slope)
    assert float((a != b).double().mean()) > 0.1


# ------------------------------------------------------------------------------------------------ dispatch and coverage
def test_case_tables_name_every_form():
    for c in G.DIRECT + G.ROWK + G.SPLITK:
        assert G.conv_form(c) == c.form, c.name
        assert c.CinP % 32 == 0 and c.CoutP % 32 == 0 and c.Cin <= c.CinP < c.Cin + 32 or c.rowk, c.name
    reached = {(c.de, c.Rk, c.stride, c.Cin, c.form) for c in G.DIRECT}
    for _, de, Rk, s in G.GEOMS:
        for Cin in (19, 75):
            for form in ('nr1', 'nr2', 'tw16_nr1', 'tw16_nr2'):
                assert (de, Rk, s, Cin, form) in reached, (de, Rk, s, Cin, form)
        if (de, Rk, s) in ((False, 1, 1), (False, 3, 1), (True, 4, 2)):
            assert (de, Rk, s, 19, 'n16') in reached and (de, Rk, s, 75, 'n16') in reached
    # the gates: stride 2 with Cout <= 16 takes NR = 1, narrow wins over N16, Cout = 17 leaves N16
    assert any(c.stride == 2 and not c.de and c.Cout <= 16 and c.form == 'nr1' for c in G.DIRECT)
    assert any(c.Cout <= 16 and c.form == 'tw16_nr1' and (c.Rk, c.stride) == (3, 1) for c in G.DIRECT)
    assert any(c.Cout == 17 and c.form == 'nr1' for c in G.DIRECT)
    assert any(c.slope == 1.0 and not c.has_bias for c in G.DIRECT) and any(c.raw_bias for c in G.DIRECT)
    assert any('sub' in c.groups and 'ovf' in c.groups for c in G.DIRECT)
    # most direct cases leave total % 8 != 0, so workgroups behind the remapped total return early
    ragged = 0
    for c in G.DIRECT:
        LH, LW = (c.H, c.W) if c.de else G.conv_geometry(c)[:2]
        tiles = ((LH + 7) // 8) * (1 if c.form.startswith('tw16') else (LW + 31) // 32)
        ragged += (G.B_CONV * (4 if c.de else 1) * (c.CoutP // (64 if c.form.endswith('nr2') else 32)) * tiles) % 8 != 0
    assert ragged > len(G.DIRECT) // 2
    # row-K: both geometries, NR 1 and 2, and an extent with LW <= 16 that stays on 32-wide tiles
    for Rk, s in ((7, 2), (3, 1)):
        for form in ('nr1', 'nr2'):
            assert any(c.Rk == Rk and c.form == form for c in G.ROWK)
            assert any(c.Rk == Rk and c.form == form and R.conv_out_size(c.W, Rk, s) <= 16 for c in G.ROWK)
    assert {(c.Rk, c.stride, c.de, c.form, c.pad0) for c in G.SPLITK} == {
        (3, 1, False, 'nr1', 2), (3, 1, False, 'nr1', 3), (3, 1, False, 'nr1', 5), (3, 1, False, 'nr1', 6), (3, 2, False, 'nr1', 4),
        (1, 1, False, 'nr2', 2), (4, 2, True, 'nr1', 3), (3, 1, False, 'n16', 2), (3, 1, False, 'tw16_nr2', 3)}
    assert any(lo >= hi for c in G.SPLITK for lo, hi in G.slab_ranges(c))          # a slab without a chunk
    # n2: every form of launch_n2<vv_h>, both sides of every threshold
    for n in G.N2:
        assert R.n2_form_f16(n[1] * n[2] * n[3], n[4]) == n[0], n
    assert {n[0] for n in G.N2} == {'tile16', 'tile32', 'split8', 'split32', 'split64', 'tap16', 'tap32', 'tap64'}
    assert any(n[0] == 'split8' and n[1] * n[2] * n[3] >= 100000 and n[4] > 32 for n in G.N2)
    assert {(n[4] + 3) // 4 for n in G.N2 if n[0] == 'split8' and n[1] == 3} == {32, 33, 49}
    assert any(n[2] == 1 for n in G.N2) and any(n[3] == 1 for n in G.N2) and G.N2_EXTRA in G.N2
    npix = {n[1] * n[2] * n[3] for n in G.N2}
    assert npix >= {1023, 1024, 4095, 4096, 4160, 20099, 20169}    # 1024 and 4096 from both sides, 20000 just above (4160 below)
    assert {n[4] for n in G.N2} >= {16, 17, 32, 33, 318, 320}


# ------------------------------------------------------------------------------------------------ float32 evaluation of every GPU case
def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize('c', G.DIRECT + G.ROWK + G.SPLITK, ids=_ids(G.DIRECT + G.ROWK + G.SPLITK))
def test_float32_evaluation_of_conv_cases_is_inside_every_bar(c):
    for group in c.groups:
        D = G.conv_data(c, group)
        G.conv_check(c, group, D, G.conv_eval32(c, D), rec=False)


@pytest.mark.parametrize('n', G.N2, ids=['%s-%dx%dx%d-%d' % n for n in G.N2])
def test_float32_evaluation_of_n2_cases_is_inside_every_bar(n):
    for group in G.n2_groups(n):
        D = G.n2_data(n, group)
        G.check_out('n2_' + n[0], n, R.act_out_f16(D['r32'].double(), D['slope']), D['pre'], D['ref'], D['e32'], D['slope'], group, rec=False, width=D['width'])


@pytest.mark.parametrize('c', G.C2, ids=['%dx%d-bias%d' % c for c in G.C2])
def test_float32_evaluation_of_c2_cases_is_inside_every_bar(c):
    for group in ('E', 'R'):
        D = G.c2_data(c, group)
        G.c2_check(c, group, D, R.act_out_f16(D['r32'].double(), D['slope']), rec=False)


def test_pack_edges_round_as_the_kernel_must():
    w = G.pack_weight(9, 19, 32, 40, 64, 0)
    p = R.pack_panel_f16(w, 32, 64, 0)
    got = {v: float(R.rn_f16(torch.tensor(v, dtype=torch.float32))) for v in G.PACK_EDGES}
    assert got[1 + 2.0 ** -11] == 1.0 and got[1 + 3 * 2.0 ** -11] == 1 + 2.0 ** -9 and got[2049.0] == 2048.0 and got[-2051.0] == -2052.0
    assert got[2.0 ** -25] == 0.0 and got[-3 * 2.0 ** -25] == -2.0 ** -23 and got[5 * 2.0 ** -25] == 2.0 ** -23
    assert got[2.0 ** -14 - 2.0 ** -25] == 2.0 ** -14 and got[65519.0] == 65504.0 and got[65520.0] == float('inf')
    assert got[-70000.0] == float('-inf') and got[1e-9] == 0.0
    assert bool(torch.isinf(p).any()) and int(((p != 0) & (p.abs() < 2.0 ** -14)).sum()) >= 3
