"""Restatement of the bf16 3x3 convolution family (vv_conv_mfma with VV_CONV_BF16, vv_conv_bf16.hip, vv_conv_ring16.hip,
vv_wgrad_bf16) written from the definitions in include/vecvad_hip.h, not from the kernels: the operand the kernel forms is
reproduced EXACTLY (nearest-even bf16 of the once-rounded fused a*x + b), the contraction is torch's conv2d /
conv_transpose2d / conv2d_weight in the dtype asked for.  float64 is the reference, float32 the yardstick of the float-summation
rule (docs/bf16_ops_parity.md).  The case tables of tests/test_gpu_bf16_ops.py live here so that tests/test_bf16_ops_host.py checks
the same inputs without a GPU."""
import functools
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from _util import away_from_zero, gen

# include/vecvad_hip.h
IN_PLAIN, IN_ACT, IN_CAT = 0, 1, 3
CONV_BF16, CONV_SRC_BF16, CONV_OUT_BF16, CONV_ALLSRC_BF16, CONV_RELU, CONV_NO_GEMM16, CONV_NO_RING = 1, 2, 8, 16, 32, 64, 128
WGRAD_DY_BF16, WGRAD_X_BF16 = 1, 2
MODES = {'plain': IN_PLAIN, 'act': IN_ACT, 'cat': IN_CAT}


def rn_bf16(t):
    """nearest-even rounding to 8 significant bits; the value is first rounded once to float32, as in the kernels"""
    return t.float().bfloat16().to(t.dtype)


def twosum_residual(a, x, b):
    """error-free TwoSum of the float64 product a*x (exact: 24 + 24 bits) and b: the part of a*x + b that float64 lost"""
    p = a.double() * x.double()
    b = b.double().expand_as(p)
    s = p + b
    bb = s - p
    return (p - (s - bb)) + (b - bb)


def _act(x, a, b):
    """max(float32(a x + b), 0) with a x + b exact in float64 (asserted by the callers through twosum_residual): the kernels' fmaf
    rounds the exact value once, and so does .float()"""
    return torch.relu((a.double() * x.double() + b.double()).float())


def operand(x0, a, b, mode, x1=None, dtype=torch.float64):
    """the bf16 operand a launch forms from its source(s), NCHW: x0 [B, C0, H, W], a / b [C0]; VV_IN_CAT: the activated src0
    channels beside the plain src1 channels.  The operand is the same whatever dtype the contraction then runs in."""
    if mode == 'plain':
        v = x0.float()
    else:
        v = _act(x0, a.view(1, -1, 1, 1), b.view(1, -1, 1, 1))
        if mode == 'cat':
            v = torch.cat([v, x1.float()], 1)
    return rn_bf16(v).to(dtype)


def _w(w, dtype):
    return rn_bf16(w.float()).to(dtype)


def _bias(t, bias, relu, dtype):
    if bias is not None:
        t = t + bias.to(dtype).view(1, -1, 1, 1)      # bias stays fp32
    return torch.relu(t) if relu else t


def conv3(op, w, bias=None, relu=False):
    """nn.Conv2d(k3, p1): w [N, K, 3, 3]"""
    return _bias(F.conv2d(op, _w(w, op.dtype), None, padding=1), bias, relu, op.dtype)


def conv3_dgrad(op, w, bias=None, relu=False):
    """data gradient of nn.Conv2d(k3, p1) with weight w [K, N, 3, 3] (K = the layer's output channels = the channels of `op`)"""
    return _bias(F.conv_transpose2d(op, _w(w, op.dtype), None, padding=1), bias, relu, op.dtype)


def convT_fwd(op, wt, bias=None):
    """nn.ConvTranspose2d(k3, s2, p1, op1): wt [K, N, 3, 3]"""
    return _bias(F.conv_transpose2d(op, _w(wt, op.dtype), None, stride=2, padding=1, output_padding=1), bias, False, op.dtype)


def convT_dgrad(op, wt, bias=None):
    """its data gradient: wt [N, K, 3, 3] (the layer's [Cin, Cout]), op = dy at 2H x 2W"""
    return _bias(F.conv2d(op, _w(wt, op.dtype), None, stride=2, padding=1), bias, False, op.dtype)


def wgrad3(act, dy):
    """weight gradient of nn.Conv2d(k3, p1): [Cout, Cin, 3, 3]"""
    return torch.nn.grad.conv2d_weight(act, (dy.shape[1], act.shape[1], 3, 3), dy, padding=1)


def wgradT(act, dy):
    """weight gradient of nn.ConvTranspose2d(k3, s2, p1, op1): [Cin, Cout, 3, 3]; conv_transpose2d(x, Wt) is the data gradient of
    conv2d(., Wt, stride 2, pad 1), so dWt = conv2d_weight(dy, Wt.shape, x)"""
    return torch.nn.grad.conv2d_weight(dy, (act.shape[1], dy.shape[1], 3, 3), act, stride=2, padding=1)


def bn_partial_ref(stored_dA, z, a, b, mean, invstd, dtype=torch.float64):
    """vv_conv_params.bn_partial: sum dz and sum dz * xhat per channel, dz = dA [a z + b > 0], xhat = (z - mean) invstd; NCHW in,
    ([C], [C]) out.  Evaluated on the dA the launch STORED."""
    v = lambda t: t.to(dtype).view(1, -1, 1, 1)
    dA, z = stored_dA.to(dtype), z.to(dtype)
    dz = torch.where(v(a) * z + v(b) > 0, dA, torch.zeros_like(dA))
    return dz.sum((0, 2, 3)), (dz * ((z - v(mean)) * v(invstd))).sum((0, 2, 3))


# ---------------------------------------------------------------------------------------------------------------- bars
FLOOR = 16 * 2.0 ** -23


def eabs(ref32, ref64):
    """e = max(8 err_ref32, 16 * 2^-23) * max|ref64|: the absolute fp32 error the float-summation rule allows in front of a rounding"""
    m = ref64.abs().max().item()
    e32 = (ref32.double() - ref64).abs().max().item() / max(m, 1e-300)
    return max(8 * e32, FLOOR) * m, e32


def bf16_out_check(got, ref64, ref32, pre64=None):
    """both rules for a bf16 output (docs/bf16_ops_parity.md): the bound on every element, and the interval rule -- bit-equal to
    rn_bf16(ref64) unless rn_bf16(ref64 - e) != rn_bf16(ref64 + e), and then between those two.  pre64 (VV_CONV_RELU launches): the
    reference in front of the ReLU, ref64 = relu(pre64) -- the fp32 error e sits on the sum, the ReLU behind it is exact and monotone,
    so the interval is [rn_bf16(relu(pre64 - e)), rn_bf16(relu(pre64 + e))]: an element well below zero is not excused, it is 0.
    Returns the figures; `ok` says whether every element obeys both."""
    got = got.double()
    e, e32 = eabs(ref32, ref64)
    bound_ok = bool(((got - ref64).abs() <= 2.0 ** -8 * ref64.abs() + (1 + 2.0 ** -8) * e).all())
    if pre64 is None:
        lo, hi = rn_bf16(ref64 - e), rn_bf16(ref64 + e)
    else:
        lo, hi = rn_bf16(torch.relu(pre64 - e)), rn_bf16(torch.relu(pre64 + e))
    mid = rn_bf16(ref64)
    exc = lo != hi
    diff = got != mid
    inside = bool(((got >= lo) & (got <= hi))[exc].all()) and not bool(diff[~exc].any())
    m = ref64.abs().max().item()
    return NS(ok=bound_ok and inside, bound_ok=bound_ok, inside=inside, excused=exc.double().mean().item(),
              differing=diff.double().mean().item(), err_ref32=e32, err_hip=(got - ref64).abs().max().item() / max(m, 1e-300))


EXCUSED_CAP, DIFFER_CAP = 0.08, 0.005


def tie_shares(ref64):
    """group E: share of the (integer / half-integer) reference values that bf16 has to round, and of exact ties among them"""
    r = rn_bf16(ref64)
    rounded = r != ref64
    f = ref64.float()
    assert torch.equal(f.double(), ref64)          # (the values of group E are exact in float32)
    # a tie: the value is exactly half way between two neighbouring bf16 numbers <=> its float32 pattern has the low 16 bits 0x8000
    ties = rounded & ((f.contiguous().view(torch.int32) & 0xFFFF) == 0x8000)
    return rounded.double().mean().item(), ties.double().mean().item()


# --------------------------------------------------------------------------------------------------------------- cases
def conv_case(name, kind, H, B, K, N, mode='plain', src='all16', out16=True, stats=False, relu=False, split=0, bnf=False, extra=0,
              G=2, csplit=0, shared=False, bias=True, form=None):
    """kind: conv3 | dgrad3 (VV_CONV3 with the forward / data-gradient panel) | convT_fwd | convT_dgrad.  K: GEMM-K channels (= CinP),
    N: output channels.  src: f32 (S16 = 0) | src16 (VV_CONV_SRC_BF16, S16 = 1) | all16 (VV_CONV_ALLSRC_BF16, S16 = 2).
    shared: one source for all UNets (gstride = 0).  form: the launch the dispatch has to select (asserted by the GPU test)."""
    if mode == 'cat' and not csplit:
        csplit = K // 2
    return NS(name=name, kind=kind, H=H, B=B, K=K, N=N, mode=mode, src=src, out16=out16, stats=stats, relu=relu, split=split, bnf=bnf,
              extra=extra, G=G, csplit=csplit if mode == 'cat' else K, shared=shared, bias=bias, form=form)


def conv_flags(c):
    f = CONV_BF16 | c.extra | (CONV_OUT_BF16 if c.out16 else 0) | (CONV_RELU if c.relu else 0)
    return f | {'f32': 0, 'src16': CONV_SRC_BF16, 'all16': CONV_ALLSRC_BF16}[c.src]


def src_hw(c):
    return 2 * c.H if c.kind == 'convT_dgrad' else c.H


def out_hw(c):
    return 2 * c.H if c.kind == 'convT_fwd' else c.H


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _grid12(t):
    return torch.round(t * 4096) / 4096


def _exact_x(x, a, b):
    """full fp32 sources: the few draws (tiny |x| beside a large b) whose a x + b needs more than 53 bits are moved onto the 2^-12
    grid as well; x [G, B, C, H, W], a / b [G, C].  The callers assert the TwoSum residual of the result."""
    res = twosum_residual(a.view(a.shape[0], 1, -1, 1, 1), x, b.view(b.shape[0], 1, -1, 1, 1))
    bad = res != 0
    if x.shape[0] == 1:      # one source shared by all UNets
        bad = bad.any(0, keepdim=True)
    return torch.where(bad, _grid12(x), x)


def conv_data(c, group):
    """CPU tensors of a case: x0 / x1 [G or 1, B, C, Hs, Hs] (bf16-valued where the tensor is bf16), a / b [G, Kact], w [G, ...],
    bias [G, N]; bnf: z [G, B, N, H, H] and bn = (a, b, mean, invstd) [G, N] each.  group 'E': exact arithmetic, 'R': random."""
    g = gen(len(c.name), sum(map(ord, c.name)), c.H, c.B, c.K, c.N, group == 'E')
    Gs, Hs, k0 = (1 if c.shared else c.G), src_hw(c), c.csplit
    wshape = {'conv3': (c.N, c.K), 'dgrad3': (c.K, c.N), 'convT_fwd': (c.K, c.N), 'convT_dgrad': (c.N, c.K)}[c.kind]
    d = NS(x1=None, a=None, b=None, bias=None, z=None, bn=None)
    E = group == 'E'
    src16 = c.src != 'f32'
    if E:
        d.x0 = _ints(g, (Gs, c.B, k0, Hs, Hs), 0 if c.mode != 'plain' else -3, 3)
        if c.mode == 'cat':
            d.x1 = _ints(g, (Gs, c.B, c.K - k0, Hs, Hs), -3, 3)
        d.w = _ints(g, (c.G,) + wshape + (3, 3), -2, 2)
        if c.bias:
            d.bias = _ints(g, (c.G, c.N), -4000, 4000)
        if c.mode != 'plain':
            d.a = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.G, k0), generator=g)]
            d.b = _ints(g, (c.G, k0), -4, 4) * 0.5
    else:
        rnd = rn_bf16 if src16 else (lambda t: t)
        d.x0 = rnd(torch.randn(Gs, c.B, k0, Hs, Hs, generator=g))
        if c.mode == 'cat':
            d.x1 = rnd(torch.randn(Gs, c.B, c.K - k0, Hs, Hs, generator=g))
        d.w = torch.randn((c.G,) + wshape + (3, 3), generator=g) * 0.1
        if c.bias:
            d.bias = torch.randn(c.G, c.N, generator=g)
        if c.mode != 'plain':
            d.a = torch.rand(c.G, k0, generator=g) + 0.5
            d.b = torch.randn(c.G, k0, generator=g) * 0.2
            if not src16:      # full fp32 sources: a and b on the 2^-12 grid keep a x + b exact in float64
                d.a, d.b = _grid12(d.a), _grid12(d.b)
                d.x0 = _exact_x(d.x0, d.a, d.b)
    if c.bnf:
        if E:
            d.z = _ints(g, (c.G, c.B, c.N, c.H, c.H), -3, 3)
            pick = lambda: torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.G, c.N), generator=g)]
            d.bn = (pick(), _ints(g, (c.G, c.N), -4, 4) * 0.5 + 0.25, _ints(g, (c.G, c.N), -2, 2) * 0.5, pick())
        else:
            ba, bb = torch.rand(c.G, c.N, generator=g) + 0.5, torch.randn(c.G, c.N, generator=g) * 0.2
            z = rn_bf16(torch.randn(c.G, c.B, c.N, c.H, c.H, generator=g))
            # kept away from a z + b = 0 AFTER the rounding to bf16 (nudged values are rounded again, then asserted)
            z = rn_bf16(away_from_zero(z.permute(0, 1, 3, 4, 2), ba.view(c.G, 1, 1, 1, -1), bb.view(c.G, 1, 1, 1, -1)).permute(0, 1, 4, 2, 3))
            assert (ba.double().view(c.G, 1, -1, 1, 1) * z.double() + bb.double().view(c.G, 1, -1, 1, 1)).abs().min().item() >= 1e-3
            d.z = z.contiguous()
            d.bn = (ba, bb, torch.randn(c.G, c.N, generator=g) * 0.1, torch.rand(c.G, c.N, generator=g) + 0.5)
    return d


def conv_operand(c, d, gi, dtype):
    s = 0 if c.shared else gi
    return operand(d.x0[s], None if d.a is None else d.a[gi], None if d.b is None else d.b[gi], c.mode,
                   None if d.x1 is None else d.x1[s], dtype)


def conv_exact(c, d):
    """the TwoSum residual of every a x + b of the case: must be 0 everywhere"""
    if c.mode == 'plain':
        return 0.0
    worst = 0.0
    for gi in range(c.G):
        x = d.x0[0 if c.shared else gi]
        worst = max(worst, twosum_residual(d.a[gi].view(1, -1, 1, 1), x, d.b[gi].view(1, -1, 1, 1)).abs().max().item())
    return worst


def conv_ref(c, d, dtype):
    """[G, B, N, Ho, Ho] in dtype, before any output rounding"""
    fn = {'conv3': conv3, 'dgrad3': conv3_dgrad, 'convT_fwd': convT_fwd, 'convT_dgrad': convT_dgrad}[c.kind]
    outs = []
    for gi in range(c.G):
        op = conv_operand(c, d, gi, dtype)
        bias = None if d.bias is None else d.bias[gi]
        outs.append(fn(op, d.w[gi], bias, c.relu) if c.kind in ('conv3', 'dgrad3') else fn(op, d.w[gi], bias))
    return torch.stack(outs)


@functools.lru_cache(maxsize=4)
def _conv_refs(key, group):
    c = NS(**vars(CONV_BY_NAME[key]))
    c.relu = False
    d = conv_data(c, group)
    return d, conv_ref(c, d, torch.float64), conv_ref(c, d, torch.float32)


def conv_refs(c, group):
    """(data, ref64, ref32, pre64) of a case, computed once and shared (never modified) by the tests that need them; cases that
    differ only in the kernel they select (`extra`, `form`) share `data_of` and therefore the tensors.  pre64: the float64 reference
    in front of the ReLU of a VV_CONV_RELU launch, else None."""
    d, r64, r32 = _conv_refs(getattr(c, 'data_of', c.name), group)
    return (d, torch.relu(r64), torch.relu(r32), r64) if c.relu else (d, r64, r32, None)


def exact_bound(c, d):
    """9 Cin max|operand| max|w| + max|bias|: below 2^24 every product and partial sum of group E is exact in fp32"""
    mx = max(conv_operand(c, d, gi, torch.float32).abs().max().item() for gi in range(c.G))
    return 9 * c.K * mx * d.w.abs().max().item() + (0 if d.bias is None else d.bias.abs().max().item())


ALL16 = dict(src='all16', out16=True)
# conv_gemm16p_kernel: all-bf16 flags, H <= 16.  form = 'p:TN<tile width>:CK<chunk>:BRES<resident filter channels>'
GEMM16P = [
    # 16x16
    conv_case('p16_tn128', 'conv3', 16, 3, 64, 128, 'act', stats=True, form='p:TN128:CK32:BRES0'),
    conv_case('p16_tn128_1chunk', 'conv3', 16, 2, 32, 128, 'plain', stats=True, form='p:TN64:CK32:BRES0'),
    conv_case('p16_tn64_ck16', 'conv3', 16, 3, 48, 64, 'cat', csplit=16, stats=True, form='p:TN64:CK16:BRES0'),
    conv_case('p16_tn32_res64', 'conv3', 16, 5, 64, 32, 'cat', stats=True, form='p:TN32:CK32:BRES64'),
    conv_case('p16_tn32_res32', 'dgrad3', 16, 3, 32, 32, 'plain', stats=True, form='p:TN32:CK32:BRES32'),
    conv_case('p16_tn32_res16', 'conv3', 16, 3, 16, 32, 'act', stats=True, form='p:TN32:CK16:BRES16'),
    conv_case('p16_tn32_nores', 'conv3', 16, 3, 48, 32, 'act', stats=True, form='p:TN32:CK16:BRES0'),
    # G NN NT = 3 * 1 * 90 = 270 > ncu, not a multiple of 8: workgroups walk several tiles, cross a UNet boundary
    conv_case('p16_walk_stats', 'conv3', 16, 90, 64, 64, 'act', stats=True, G=3, form='p:TN64:CK32:BRES0:walk'),
    conv_case('p16_walk_relu', 'conv3', 16, 90, 64, 64, 'plain', relu=True, stats=True, G=3, form='p:TN64:CK32:BRES0:walk'),
    conv_case('p16_walk_split_in', 'dgrad3', 16, 45, 32, 128, 'plain', split=64, stats=True, G=3, form='p:TN64:CK32:BRES0:walk'),
    conv_case('p16_walk_split_span', 'dgrad3', 16, 90, 64, 64, 'plain', split=32, stats=True, G=3, form='p:TN64:CK32:BRES0:walk'),
    # NN = 3 does not divide the workgroup stride of 32: 2 * 3 * 45 = 270 units, a workgroup's second unit is another N tile
    conv_case('p16_walk_nn', 'conv3', 16, 45, 32, 192, 'act', stats=True, G=2, form='p:TN64:CK32:BRES0:walk:nn'),
    # 8x8 (tiles of 4 images: ragged B % 4 != 0)
    conv_case('p8_tn128', 'conv3', 8, 9, 64, 128, 'cat', stats=True, form='p:TN128:CK32:BRES0'),
    conv_case('p8_tn128_ck16', 'conv3', 8, 6, 48, 128, 'act', stats=True, form='p:TN128:CK16:BRES0'),
    conv_case('p8_tn64', 'dgrad3', 8, 7, 32, 64, 'plain', stats=True, form='p:TN64:CK32:BRES0'),
    conv_case('p8_tn32_res64', 'conv3', 8, 5, 64, 32, 'act', stats=True, form='p:TN32:CK32:BRES64'),
    conv_case('p8_tn32_res16', 'conv3', 8, 5, 16, 32, 'plain', stats=True, form='p:TN32:CK16:BRES16'),
    conv_case('p8_tn32_nores', 'conv3', 8, 6, 48, 32, 'cat', csplit=16, stats=True, form='p:TN32:CK16:BRES0'),
    conv_case('p8_tn128_1chunk', 'conv3', 8, 5, 32, 128, 'act', stats=True, form='p:TN64:CK32:BRES0'),
    conv_case('p8_tn32_res32', 'dgrad3', 8, 7, 32, 32, 'plain', stats=True, form='p:TN32:CK32:BRES32'),
    conv_case('p8_walk', 'conv3', 8, 357, 32, 64, 'act', stats=True, G=3, form='p:TN64:CK32:BRES0:walk'),       # 3 * 90 = 270 units
    conv_case('p8_walk_nn', 'conv3', 8, 179, 32, 192, 'plain', stats=True, G=2, form='p:TN64:CK32:BRES0:walk:nn'),  # 2 * 3 * 45 units
    # 4x4 (tiles of 16 images: ragged B % 16 != 0; CK = 16 only)
    conv_case('p4_tn128', 'conv3', 4, 33, 32, 128, 'act', stats=True, form='p:TN128:CK16:BRES0'),
    conv_case('p4_tn64', 'conv3', 4, 17, 32, 64, 'cat', stats=True, form='p:TN64:CK16:BRES0'),
    conv_case('p4_tn32_res32', 'dgrad3', 4, 40, 32, 32, 'plain', stats=True, form='p:TN32:CK16:BRES32'),
    conv_case('p4_tn32_res64', 'conv3', 4, 5, 64, 32, 'act', stats=True, form='p:TN32:CK16:BRES64'),
    conv_case('p4_tn32_nores', 'conv3', 4, 21, 48, 32, 'plain', stats=True, form='p:TN32:CK16:BRES0'),
    conv_case('p4_tn128_1chunk', 'conv3', 4, 19, 16, 128, 'plain', stats=True, form='p:TN64:CK16:BRES0'),
    conv_case('p4_tn32_res16', 'conv3', 4, 21, 16, 32, 'act', stats=True, form='p:TN32:CK16:BRES16'),
    conv_case('p4_walk', 'conv3', 4, 1430, 16, 64, 'act', stats=True, G=3, form='p:TN64:CK16:BRES0:walk'),      # 3 * 90 = 270 units
    conv_case('p4_walk_nn', 'conv3', 4, 715, 16, 192, 'act', stats=True, G=2, form='p:TN64:CK16:BRES0:walk:nn'),   # 2 * 3 * 45 units
]

# conv_ring16_kernel (32x32, CinP 16 | 32, Cout 32, G B 4 >= 2048) and, with VV_CONV_NO_RING, conv_mfma_kernel<8,32,1,1,CONV3,16,true,2|3>
_RING = [
    ('ring_plain', dict(K=16, mode='plain')),
    ('ring_act', dict(K=32, mode='act')),
    ('ring_stats', dict(K=16, mode='act', stats=True)),
    ('ring_bnf', dict(K=16, mode='plain', bnf=True, kind='dgrad3')),
    ('ring_relu', dict(K=16, mode='plain', relu=True, stats=True)),
]
RING = []
for _n, _kw in _RING:
    _kw = dict(_kw)
    _kind = _kw.pop('kind', 'conv3')
    for _extra, _tag in ((0, ''), (CONV_NO_RING, '_noring')):
        _c = conv_case(_n + _tag, _kind, 32, 86, N=32, G=6, extra=_extra,
                       form=('ring:KS%d' % (_kw['K'] // 16)) if not _extra else 'mfma:8x32x1:NR1:S16=%d' % (3 if _kw.get('bnf') else 2), **_kw)
        _c.data_of = _n
        RING.append(_c)

# conv_mfma_kernel<.., BF = true>.  form = 'mfma:<tile>:NR<n>:S16=<s>'
MFMA = []
for _H, _B, _tile in ((32, 2, '8x32x1'), (16, 3, '8x16x1'), (8, 5, '8x8x2'), (4, 19, '4x4x8')):
    # S16 = 0: fp32 tensors, ACT / CAT with a, b on the 12-bit grid; fp32 output
    MFMA.append(conv_case('m%d_f32_act' % _H, 'conv3', _H, _B, 32, 32, 'act', src='f32', out16=False, stats=True,
                          form='mfma:%s:NR1:S16=0' % _tile))
    MFMA.append(conv_case('m%d_f32_cat' % _H, 'conv3', _H, _B, 32, 64, 'cat', csplit=16, src='f32', out16=False, stats=True,
                          form='mfma:%s:NR%d:S16=0' % (_tile, 1 if _H == 32 else 2)))
    # S16 = 1: VV_CONV_SRC_BF16 (a data gradient reading a bf16 dy), fp32 output -- bf16 output would select the GEMM-shaped kernel
    MFMA.append(conv_case('m%d_src16' % _H, 'dgrad3', _H, _B, 32, 32, 'plain', src='src16', out16=False, stats=True, bias=False,
                          form='mfma:%s:NR1:S16=1' % _tile))
    MFMA.append(conv_case('m%d_src16_o16' % _H, 'dgrad3', _H, _B, 32, 64, 'plain', src='src16', out16=True, stats=True, extra=CONV_NO_GEMM16,
                          form='mfma:%s:NR%d:S16=1' % (_tile, 1 if _H == 32 else 2)))
    # S16 = 2 with VV_CONV_NO_GEMM16
    MFMA.append(conv_case('m%d_all16' % _H, 'conv3', _H, _B, 48, 32, 'cat', csplit=16, stats=True, extra=CONV_NO_GEMM16,
                          form='mfma:%s:NR1:S16=2' % _tile))
    MFMA.append(conv_case('m%d_all16_relu' % _H, 'conv3', _H, _B, 32, 64, 'plain', relu=True, stats=True, extra=CONV_NO_GEMM16,
                          form='mfma:%s:NR%d:S16=2' % (_tile, 1 if _H == 32 else 2)))
# wide at 32x32: G nt Cout/64 = 8 * 128 * 1 >= 1024, one source shared by the 8 UNets
MFMA.append(conv_case('m32_wide', 'conv3', 32, 32, 16, 64, 'act', src='f32', out16=False, stats=True, G=8, shared=True,
                      form='mfma:8x32x1:NR2:S16=0'))
for _H, _B, _tile, _tiled in ((16, 3, '16x16x1', '16x16x1'), (8, 5, '8x8x4', '8x8x4'), (4, 19, '4x4x16', '4x4x16')):
    MFMA.append(conv_case('t%d_fwd_f32' % _H, 'convT_fwd', _H, _B, 32, 32, 'act', src='f32', out16=False, form='mfmaT:%s:NR1:S16=0' % _tile))
    MFMA.append(conv_case('t%d_fwd_all16' % _H, 'convT_fwd', _H, _B, 32, 32, 'act', form='mfmaT:%s:NR1:S16=2' % _tile))
    # VV_CONVT_DGRAD: ragged B on the 16-image tiles (B % 16 != 0 at 4x4, B % 4 != 0 at 8x8)
    MFMA.append(conv_case('t%d_dgrad_f32' % _H, 'convT_dgrad', _H, _B, 32, 32, 'plain', src='f32', out16=False, stats=True, bias=False,
                          form='mfmaD:%s:NR1:S16=0' % _tiled))
    MFMA.append(conv_case('t%d_dgrad_src16' % _H, 'convT_dgrad', _H, _B, 32, 64, 'plain', src='src16', out16=True, stats=True,
                          form='mfmaD:%s:NR1:S16=1' % _tiled))
    MFMA.append(conv_case('t%d_dgrad_all16' % _H, 'convT_dgrad', _H, _B, 16, 32, 'plain', stats=True, form='mfmaD:%s:NR1:S16=2' % _tiled))
# wide VV_CONVT_DGRAD: G nt Cout/64 = 8 * 128 >= 1024 at 4x4 (2048 images in tiles of 16), one dy shared by the 8 UNets
MFMA.append(conv_case('t4_dgrad_wide', 'convT_dgrad', 4, 2041, 16, 64, 'plain', src='src16', out16=True, stats=True, G=8, shared=True,
                      form='mfmaD:4x4x16:NR2:S16=1'))

CONV_CASES = GEMM16P + RING + MFMA
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
assert len(CONV_BY_NAME) == len(CONV_CASES)


def walk_info(G, NN, NT, ncu):
    """What the persistent workgroups of conv_gemm16p_kernel do with a launch of G * NN * NT units, restated from vv_conv_bf16.hip:155-183
    (UnitCur / UnitStep: unit u = (g NT + pt) NN + nn), :233-239 (XCD x owns units [x nper, (x + 1) nper), its grid / 8 workgroups take
    them strided) and :696-706 (launch_p: the grid).  Returns (longest run of tiles folded into one stats row, whether some workgroup's
    consecutive units differ in the UNet, whether some differ in the N tile)."""
    total = G * NN * NT
    nper = (total + 7) // 8
    grid = (min(ncu, nper * 8) + 7) & ~7
    wgx = grid // 8
    run_max, cross_g, cross_nn = 1, False, False
    for x in range(8):
        uend = min((x + 1) * nper, total)
        for j in range(wgx):
            us = list(range(x * nper + j, uend, wgx))
            run = 1
            for u0, u1 in zip(us, us[1:]):
                g0, n0, g1, n1 = u0 // (NN * NT), u0 % NN, u1 // (NN * NT), u1 % NN
                cross_g |= g0 != g1
                cross_nn |= n0 != n1
                run = run + 1 if (g0 == g1 and n0 == n1) else 1      # (the run ends where the next unit is another UNet / N tile)
                run_max = max(run_max, run)
    return run_max, cross_g, cross_nn


def expected_form(c, ncu):
    """The launch vv_conv_mfma selects for a case, restated from the C++ (line numbers at the time of writing):
    vv_conv.hip:599-626 (vv_conv_mfma), :495-540 (dispatch), vv_common.h:46-49 (vv_gemm16_flags), vv_conv_bf16.hip:695-728 (launch_p,
    dispatch_p), :746-751 (vv_conv_gemm16), vv_conv_ring16.hip:364-382."""
    flags = conv_flags(c)
    kind3 = c.kind in ('conv3', 'dgrad3')
    sm = 2 if flags & CONV_ALLSRC_BF16 else (1 if flags & CONV_SRC_BF16 else 0)
    gemm16 = kind3 and (flags & CONV_OUT_BF16) and (flags & (CONV_SRC_BF16 | CONV_ALLSRC_BF16)) and not (flags & CONV_NO_GEMM16)
    if gemm16 and c.H <= 16:
        ck32 = c.K % 32 == 0 and (c.mode != 'cat' or c.csplit % 32 == 0)
        CK = 32 if (ck32 and c.H != 4) else 16
        if c.N % 128 == 0 and c.K // CK >= 2:
            TN, BRES = 128, 0
        elif c.N % 64 == 0:
            TN, BRES = 64, 0
        elif c.K == 64 and 64 % CK == 0:
            TN, BRES = 32, 64
        elif c.K == 32 and 32 % CK == 0:
            TN, BRES = 32, 32
        elif c.K == 16 and CK == 16:
            TN, BRES = 32, 16
        else:
            TN, BRES = 32, 0
        NI = {16: 1, 8: 4, 4: 16}[c.H]
        total = c.G * (c.N // TN) * ((c.B + NI - 1) // NI)
        _, cross_g, cross_nn = walk_info(c.G, c.N // TN, (c.B + NI - 1) // NI, ncu)
        walk = total > ncu and total % 8 != 0 and cross_g      # some workgroup takes a second tile, and one of another UNet
        return 'p:TN%d:CK%d:BRES%d%s%s' % (TN, CK, BRES, ':walk' if walk else '', ':nn' if walk and cross_nn else '')
    if (sm == 2 and kind3 and c.H == 32 and c.K in (16, 32) and c.N % 64 != 0 and not (flags & CONV_NO_RING) and (flags & CONV_OUT_BF16)
            and c.mode in ('plain', 'act') and c.G * (c.N // 32) * c.B * 4 >= 2048):
        return 'ring:KS%d' % (c.K // 16)
    t256 = {32: (8, 32, 1), 16: (16, 16, 1), 8: (8, 8, 4), 4: (4, 4, 16)}[c.H]
    if kind3:
        if sm == 2 and c.bnf:
            return 'mfma:8x32x1:NR1:S16=3'
        if c.H == 32:
            nt = c.B * 4
            wide = c.N % 64 == 0 and c.G * nt * (c.N // 64) >= 1024
            return 'mfma:8x32x1:NR%d:S16=%d' % (2 if wide else 1, sm)
        tile = {16: '8x16x1', 8: '8x8x2', 4: '4x4x8'}[c.H]      # dispatch<BF, VV_CONV3>: 128-pixel tiles, 64-wide whenever Cout % 64 == 0
        return 'mfma:%s:NR%d:S16=%d' % (tile, 2 if c.N % 64 == 0 else 1, sm)
    nt = ((c.B + t256[2] - 1) // t256[2]) * (c.H // t256[0])
    if c.kind == 'convT_fwd':
        return 'mfmaT:%dx%dx%d:NR1:S16=%d' % (t256 + (sm,))
    wide = c.N % 64 == 0 and c.G * nt * (c.N // 64) >= 1024
    return 'mfmaD:%dx%dx%d:NR%d:S16=%d' % (t256 + (2 if wide else 1, sm))


# ------------------------------------------------------------------------------------------------------ weight gradient
def wgrad_case(name, kind, H, B, Cin, CinP, Cout, ks, mode='act', ring=False, form=None, G=2):
    """kind: conv3 | convT.  ks: 1 | 'mid' | 'all'.  ring: VV_WGRAD_X_BF16 | VV_WGRAD_DY_BF16 (bf16 tensors).  form = '<launch>:c<ci
    blocks>:o<co blocks>'"""
    return NS(name=name, kind=kind, H=H, B=B, Cin=Cin, CinP=CinP, Cout=Cout, ks=ks, mode=mode, ring=ring, form=form, G=G,
              csplit=CinP // 2 if mode == 'cat' else CinP)


WGRAD_CASES = [
    # tile form (fp32 tensors, launch_b): every block shape, all four levels
    wgrad_case('wb32_c1o1', 'conv3', 32, 2, 12, 16, 32, 'mid', form='b:c1:o1'),
    wgrad_case('wb16_c2o2', 'conv3', 16, 5, 64, 64, 64, 'mid', form='b:c2:o2'),
    wgrad_case('wb8_c2o1', 'conv3', 8, 9, 64, 64, 32, 'all', 'cat', form='b:c2:o1'),
    wgrad_case('wb4_c1o2', 'conv3', 4, 33, 32, 32, 64, 1, form='b:c1:o2'),
    wgrad_case('wb4_c2o2', 'conv3', 4, 19, 64, 64, 64, 'mid', 'plain', form='b:c2:o2'),
    # ring form (bf16 tensors, launch_r) at 32 / 16 / 8; at 4x4 the same flags stay on launch_b
    wgrad_case('wr32_c1o1', 'conv3', 32, 3, 12, 16, 32, 'mid', ring=True, form='r:c1:o1'),
    wgrad_case('wr32_c2o1', 'conv3', 32, 2, 64, 64, 32, 1, ring=True, form='r:c2:o1'),
    wgrad_case('wr16_c1o2', 'conv3', 16, 5, 32, 32, 64, 'all', 'plain', ring=True, form='r:c1:o2'),
    wgrad_case('wr8_c2o2', 'conv3', 8, 9, 64, 64, 64, 'mid', 'cat', ring=True, form='r:c2:o2'),
    wgrad_case('wr4_b', 'conv3', 4, 33, 32, 32, 32, 'mid', ring=True, form='b:c1:o1'),
    # transposed conv (launch_t), incl. the 2 x 2 block shape that TW = 4 excludes
    wgrad_case('wt16_c2o1', 'convT', 16, 3, 64, 64, 32, 'mid', form='t:c2:o1'),
    wgrad_case('wt8_c2o2', 'convT', 8, 5, 64, 64, 64, 1, form='t:c2:o2'),
    wgrad_case('wt8_c1o1', 'convT', 8, 2, 32, 32, 32, 'all', form='t:c1:o1'),
    wgrad_case('wt4_c2o2', 'convT', 4, 17, 64, 64, 64, 'mid', form='t:c2:o1'),
    wgrad_case('wt4_c1o2', 'convT', 4, 9, 32, 32, 64, 'all', form='t:c1:o2'),
]
WGRAD_BY_NAME = {c.name: c for c in WGRAD_CASES}


def wgrad_form(c):
    """vv_wgrad_bf16.hip:917-948 (vv_wgrad_bf16), :859-866 (ring_ok), :843-847 (ring_block_shape), :767-771 (block_shape)"""
    nci, nco = (c.CinP + 31) // 32, c.Cout // 32
    cb, ob = (2 if nci % 2 == 0 else 1), (2 if nco % 2 == 0 else 1)
    if c.kind == 'conv3' and c.ring and c.H >= 8 and (c.mode != 'cat' or c.csplit % 32 == 0):
        return 'r:c%d:o%d' % (cb, ob)
    if c.kind != 'conv3' and c.H == 4 and cb * ob == 4:
        ob = 1
    return '%s:c%d:o%d' % ('b' if c.kind == 'conv3' else 't', cb, ob)


def wgrad_data(c, group):
    """x0 / x1 [G, B, C, H, H] (channels >= Cin zero, b = 0 there), a / b [G, CinP], dy [G, B, Cout, Hd, Hd]"""
    g = gen(len(c.name), sum(map(ord, c.name)), c.H, c.B, c.CinP, c.Cout, group == 'E', 7)
    Hd = 2 * c.H if c.kind == 'convT' else c.H
    k0 = c.csplit
    d = NS(x1=None, a=None, b=None)
    if group == 'E':
        d.x0 = _ints(g, (c.G, c.B, k0, c.H, c.H), 0 if c.mode != 'plain' else -3, 3)
        if c.mode == 'cat':
            d.x1 = _ints(g, (c.G, c.B, c.CinP - k0, c.H, c.H), -3, 3)
        d.dy = _ints(g, (c.G, c.B, c.Cout, Hd, Hd), -3, 3)
        if c.mode != 'plain':
            d.a = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.G, k0), generator=g)]
            d.b = _ints(g, (c.G, k0), -4, 4) * 0.5
    else:
        rnd = rn_bf16 if c.ring else (lambda t: t)
        d.x0 = rnd(torch.randn(c.G, c.B, k0, c.H, c.H, generator=g))
        if c.mode == 'cat':
            d.x1 = rnd(torch.randn(c.G, c.B, c.CinP - k0, c.H, c.H, generator=g))
        d.dy = rnd(torch.randn(c.G, c.B, c.Cout, Hd, Hd, generator=g))
        if c.mode != 'plain':
            d.a = torch.rand(c.G, k0, generator=g) + 0.5
            d.b = torch.randn(c.G, k0, generator=g) * 0.2
            if not c.ring:
                d.a, d.b = _grid12(d.a), _grid12(d.b)
                d.x0 = _exact_x(d.x0, d.a, d.b)
    if c.Cin < c.CinP:      # zero padding: the channels are zeros and b = 0 there (relu(a 0 + 0) = 0)
        assert c.mode == 'act'
        d.x0[:, :, c.Cin:] = 0
        d.b[:, c.Cin:] = 0
    return d


def wgrad_exact(c, d):
    if c.mode == 'plain':
        return 0.0
    return max(twosum_residual(d.a[gi].view(1, -1, 1, 1), d.x0[gi], d.b[gi].view(1, -1, 1, 1)).abs().max().item() for gi in range(c.G))


def wgrad_exact_bound(c, d):
    """2 * pixels * max|operand| * max|dy|: below 2^24 every partial sum of group E (multiples of 0.5) is exact in fp32"""
    mx = max(operand(d.x0[gi], None if d.a is None else d.a[gi], None if d.b is None else d.b[gi], c.mode,
                     None if d.x1 is None else d.x1[gi], torch.float32).abs().max().item() for gi in range(c.G))
    return 2 * d.dy[0, :, 0].numel() * mx * d.dy.abs().max().item()


def wgrad_ref(c, d, dtype):
    """[G, Cout, Cin, 3, 3] (conv3) or [G, Cin, Cout, 3, 3] (convT)"""
    outs = []
    for gi in range(c.G):
        act = operand(d.x0[gi], None if d.a is None else d.a[gi], None if d.b is None else d.b[gi], c.mode,
                      None if d.x1 is None else d.x1[gi], dtype)[:, :c.Cin]
        dy = rn_bf16(d.dy[gi]).to(dtype)
        outs.append(wgrad3(act, dy) if c.kind == 'conv3' else wgradT(act, dy))
    return torch.stack(outs)


@functools.lru_cache(maxsize=4)
def _wgrad_refs(name, group):
    c = WGRAD_BY_NAME[name]
    d = wgrad_data(c, group)
    return d, wgrad_ref(c, d, torch.float64), wgrad_ref(c, d, torch.float32)


def wgrad_refs(c, group):
    return _wgrad_refs(c.name, group)
