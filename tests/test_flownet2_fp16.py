"""FlowNet2(fp16=True): fp16 activations on fp16 MFMA with fp32 accumulation ("fp16 storage fp32 math", the reference's
FlowNet2_src/main.py:123-125).  CPU: the module accepts the flag and keeps the fp32 parameter set.  GPU: every layer form of the
fp16 convolution, the fp16 correlation and glue kernels within one fp16 ulp of the half graph's value (tests/flownet2_fp16_restatement.py,
pinned to the reference's own half graph by tests/golden/flownet2_fp16_128x192.npz), and the whole forward against that golden and the
fp32 oracle (128 x 192) or the fp32 HIP forward (1024 x 448, the driver).  The 1024 x 448 comparison deviates from the fp32 oracle
on purpose: the oracle's CPU forward at that size is slow, and the fp32 HIP forward is itself pinned to it at 1e-3 x max."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _util import load_golden
from test_flownet2 import _inputs, _seeded_sd
import flownet2_fp16_restatement as HR


def test_flownet2_fp16_constructs_with_the_fp32_parameter_set():
    from vec_vad_amd.flownet2 import FlowNet2, FlowNetC
    a, b = FlowNet2(), FlowNet2(fp16=True)
    assert b.fp16 and not a.fp16
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].shape == sb[k].shape and sa[k].dtype == sb[k].dtype == torch.float32, k
    b.load_state_dict(sa)                       # a fp32 checkpoint loads unchanged
    assert FlowNetC(fp16=True).fp16
    with pytest.raises(NotImplementedError):
        FlowNet2(with_bn=True, fp16=True)


def test_half_graph_restatement_reproduces_the_fp16_golden():
    """The CPU restatement of the half graph against the imported reference's FlowNet2(fp16=True) + .half() (the golden)."""
    torch.set_num_threads(min(8, torch.get_num_threads()))
    _, sd, _ = _seeded_sd()
    g = load_golden('flownet2_fp16_128x192')
    out = HR.flownet2_fp16_forward(sd, _inputs())
    assert out.dtype == torch.float16 and list(out.shape) == list(g['out_shape'])
    assert torch.equal(out, torch.from_numpy(g['out']))


def _ulp16(a):
    """fp16 ulp of |a| (float64 tensor)."""
    a = a.abs().clamp_min(2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(a)) - 10)


def _half_layer_ref(kind, x16, w, b, stride, R, relu):
    """The half graph of conv / deconv [+ LeakyReLU(0.1)]: fp16 operands, exact (fp64) accumulation, bias added, rounded to fp16;
    LeakyReLU on the rounded value, rounded again.  Also returns sum |x| |w| per output (the scale of fp32 accumulation round-off)."""
    xd, wd = x16.double(), w.half().double()
    bd = None if b is None else b.half().double()
    if kind == 'conv':
        op = lambda x_, w_, b_: F.conv2d(x_, w_, b_, stride=stride, padding=(R - 1) // 2)
    else:
        op = lambda x_, w_, b_: F.conv_transpose2d(x_, w_, b_, stride=2, padding=1)
    y = op(xd, wd, bd).float().half()
    if relu:
        y = torch.where(y > 0, y, (y.float() * 0.1).half())
    return y, op(xd.abs(), wd.abs(), None)


F16_CONV_CASES = [  # (kind, R, stride, Cin, Cout, H, W, relu)
    # row-K first layers (3-channel 7x7 s2, 6-channel 3x3), ragged sizes, several tiles per row
    ('conv', 7, 2, 3, 64, 37, 139, True), ('conv', 3, 1, 6, 64, 17, 70, False),
    # k in {1, 3, 5, 7}, stride 1 / 2, odd channel counts (K padding), 32- and 64-wide N tiles, N masking
    ('conv', 7, 2, 12, 64, 40, 72, True), ('conv', 5, 2, 64, 128, 32, 48, True), ('conv', 3, 1, 473, 256, 16, 24, True),
    ('conv', 3, 2, 256, 512, 16, 24, True), ('conv', 1, 1, 256, 32, 16, 24, True), ('conv', 3, 1, 194, 64, 32, 48, False),
    ('conv', 3, 1, 11, 64, 24, 40, True), ('conv', 3, 1, 96, 48, 9, 33, True),
    # at most 16 output channels: v_mfma_f32_16x16x32_f16
    ('conv', 3, 1, 82, 16, 20, 36, False), ('deconv', 4, 2, 162, 16, 12, 20, True),
    # the H/64 level (8 x 16 tiles), split-K on the H/32 / H/64 levels
    ('conv', 3, 1, 1024, 1024, 7, 16, True), ('conv', 3, 2, 512, 1024, 14, 32, True), ('conv', 3, 1, 512, 512, 14, 32, True),
    ('deconv', 4, 2, 1024, 512, 7, 16, True), ('deconv', 4, 2, 1026, 256, 4, 6, True), ('deconv', 4, 2, 386, 64, 13, 19, True),
    # two-channel heads: predict_flow (tile / split / tap forms) and upsampled_flow
    ('conv', 3, 1, 1026, 2, 4, 6, False), ('conv', 3, 1, 770, 2, 28, 20, False), ('conv', 3, 1, 386, 2, 40, 56, False),
    ('conv', 3, 1, 194, 2, 104, 100, False), ('conv', 3, 1, 16, 2, 120, 100, False), ('conv', 3, 1, 32, 2, 101, 103, False),
    ('conv', 3, 1, 194, 2, 48, 50, False),      # 32 lanes per pixel: 4096 <= pixels < 20000 with Cin < 320
    ('deconv', 4, 2, 2, 2, 4, 6, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize('kind,R,stride,Cin,Cout,H,W,relu', F16_CONV_CASES)
def test_conv2d_f16_within_one_ulp_of_half_graph(kind, R, stride, Cin, Cout, H, W, relu):
    from vec_vad_amd.flownet2 import _Runner, _Buf, _to_buf
    g = torch.Generator().manual_seed(R * 1000 + Cin + 7)
    x16 = torch.randn(2, Cin, H, W, generator=g).half()
    if kind == 'conv':
        m = nn.Conv2d(Cin, Cout, R, stride=stride, padding=(R - 1) // 2)
    else:
        m = nn.ConvTranspose2d(Cin, Cout, 4, 2, 1, bias=Cin != 2)
    with torch.no_grad():
        ref, absum = _half_layer_ref(kind, x16, m.weight, m.bias, stride, R, relu)
    layer = (nn.Sequential(m, nn.LeakyReLU(0.1)) if relu else m).cuda()
    src = _to_buf(x16.cuda())
    assert src.t.dtype == torch.float16 and src.cs % 8 == 0
    dst = _Buf(2, ref.shape[2], ref.shape[3], Cout + 12, 'cuda', torch.float16)      # a channel slice of a wider buffer
    _Runner()(layer, src, dst, 8)
    torch.cuda.synchronize()
    out = dst.t[..., 8:8 + Cout].permute(0, 3, 1, 2).cpu()
    d = (out.double() - ref.double()).abs()
    # one fp16 ulp of the reference element; where the sum cancels to far below its terms the fp32 accumulation round-off of two
    # summation orders (~2^-24 sqrt(n) of sum |x w|) exceeds that ulp, so it is allowed on top (2^-16 sum |x w|)
    tol = _ulp16(ref.double()) + 2.0 ** -16 * absum
    assert bool(torch.isfinite(out).all())
    frac_equal = float((out == ref).double().mean())
    print('bit-equal fraction %.5f, max |d| / fp16 ulp %.2f' % (frac_equal, float((d / _ulp16(ref.double())).max())))
    assert float((d / tol).max()) <= 1.0, (float((d / tol).max()), float(d.max()))
    assert frac_equal >= 0.99, frac_equal         # (measured 0.998 - 1.0: the two summation orders differ only in fp32 round-off)
    assert float(dst.t[..., :8].abs().max()) == 0 and float(dst.t[..., 8 + Cout:].abs().max()) == 0   # neighbours untouched


@pytest.mark.gpu
def test_flownet_prep_f16_within_one_ulp():
    from vec_vad_amd import _lib as L
    inp = _inputs()
    B, _, _, H, W = inp.shape
    lib = L.lib()
    x6 = torch.zeros(B, H, W, 8, dtype=torch.float16, device='cuda')
    i0, i1 = torch.zeros_like(x6), torch.zeros_like(x6)
    ws = torch.zeros(int(lib.vv_flownet_prep_workspace_bytes(B)) // 4, device='cuda')
    L.check(lib.vv_flownet_prep_f16(inp.cuda().data_ptr(), B, H, W, 255.0, ws.data_ptr(), ws.numel() * 4, x6.data_ptr(),
                                    i0.data_ptr(), i1.data_ptr(), torch.cuda.current_stream().cuda_stream), 'prep_f16')
    torch.cuda.synchronize()
    # the half graph (flownet2.py:66-72): mean rounded, x - mean rounded, / rgb_max rounded
    x = inp.half()
    mean = x.float().view(B, 3, -1).mean(-1).half().view(B, 3, 1, 1, 1)
    xn = ((x - mean).float() / 255.0).half()
    ref = torch.cat((xn[:, :, 0], xn[:, :, 1]), 1).permute(0, 2, 3, 1)
    out = x6[..., :6].cpu()
    d = (out.double() - ref.double()).abs()
    assert float((d / _ulp16(ref.double())).max()) <= 1.0
    assert torch.equal(i0[..., :3].cpu(), out[..., :3]) and torch.equal(i1[..., :3].cpu(), out[..., 3:6])


def _nhwc(t, cs):
    """NCHW CPU tensor -> [B,H,W,cs] fp16 CUDA buffer (pad channels zero)."""
    B, C, H, W = t.shape
    b = torch.zeros(B, H, W, cs, dtype=torch.float16, device='cuda')
    b[..., :C] = t.permute(0, 2, 3, 1).cuda()
    return b


def _within_one_ulp(out, ref, extra=None):
    d = (out.double() - ref.double()).abs()
    tol = _ulp16(ref.double()) + (0 if extra is None else extra)
    r = float((d / tol).max())
    print('bit-equal fraction %.5f, max |d| / tol %.2f' % (float((out == ref).double().mean()), r))
    assert r <= 1.0, (r, float(d.max()))


@pytest.mark.gpu
def test_correlation_nhwc_f16_within_one_ulp():
    """vv_correlation_nhwc_f16: widened maps, the fp32 correlation, rounded, LeakyReLU on the rounded value, rounded
    (nn.Sequential(tofp32(), corr, tofp16()) + corr_activation on half, FlowNetC.py:31,90-91), into channels [32, 473)."""
    from vec_vad_amd import _lib as L
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 1, 256, 10, 64
    a = (torch.randn(B, C, H, W, generator=g) * 0.7).half()
    b = (torch.randn(B, C, H, W, generator=g) * 0.7).half()
    ref = torch.from_numpy(HR.correlation_fwd(a.numpy(), b.numpy(), 20, 1, 20, 1, 2, 1))
    ref = torch.where(ref > 0, ref, (ref.float() * 0.1).half())
    absum = torch.from_numpy(HR.ops.correlation_fwd(a.float().abs().numpy(), b.float().abs().numpy(), 20, 1, 20, 1, 2, 1)).double()
    f1, f2 = _nhwc(a, C), _nhwc(b, C)
    out = torch.zeros(B, H, W, 480, dtype=torch.float16, device='cuda')
    L.check(L.lib().vv_correlation_nhwc_f16(f1.data_ptr(), f2.data_ptr(), C, B, C, H, W, out.data_ptr(), 480, 32, 0.1,
                                            torch.cuda.current_stream().cuda_stream), 'correlation_nhwc_f16')
    torch.cuda.synchronize()
    o = out.cpu()
    assert float(o[..., :32].abs().max()) == 0 and float(o[..., 473:].abs().max()) == 0
    # (a sum of 256 products that cancels: fp32 round-off of two summation orders allowed on top, as for the convolutions)
    _within_one_ulp(o[..., 32:473].permute(0, 3, 1, 2), ref, 2.0 ** -16 * absum)


def _glue_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, 6, H, W, generator=g) - 0.5).half()                    # normalised frame pair, +-0.5
    f_a = (torch.randn(B, 2, H // 4, W // 4, generator=g) * 0.15).half()      # flow2 maps: a few pixels after x div_flow
    f_b = (torch.randn(B, 2, H // 4, W // 4, generator=g) * 0.15).half()
    return x, f_a, f_b


@pytest.mark.gpu
def test_warp_pack12_f16_within_one_ulp():
    """vv_warp_pack12_f16 against the half graph of flownet2.py:76-86: upsample x4 (bilinear) of the rounded flow2 * div_flow,
    Resample2d widened and rounded, x0 - warped rounded, ChannelNorm widened and rounded, flow / div_flow rounded."""
    from vec_vad_amd import _lib as L
    B, H, W = 2, 64, 96
    x, f2, _ = _glue_inputs(B, H, W, 5)
    fl = F.interpolate(f2 * 20.0, scale_factor=4, mode='bilinear', align_corners=False)
    warped = torch.from_numpy(HR.resample2d_fwd(x[:, 3:].numpy(), fl.numpy()))
    nrm = torch.from_numpy(HR.channelnorm_fwd((x[:, :3] - warped).numpy()))
    ref = torch.cat([x, warped, fl / 20.0, nrm], 1)
    assert ref.dtype == torch.float16
    x6, img1, fb = _nhwc(x, 8), _nhwc(x[:, 3:], 8), _nhwc(f2, 8)
    out = torch.zeros(B, H, W, 16, dtype=torch.float16, device='cuda')
    L.check(L.lib().vv_warp_pack12_f16(x6.data_ptr(), img1.data_ptr(), fb.data_ptr(), 8, B, H, W, 1, 20.0, 20.0, out.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), 'warp_pack12_f16')
    torch.cuda.synchronize()
    o = out.cpu()
    _within_one_ulp(o[..., :12].permute(0, 3, 1, 2), ref)


@pytest.mark.gpu
def test_fusion_pack11_f16_within_one_ulp():
    """vv_fusion_pack11_f16 against the half graph of flownet2.py:105-136: nearest x4 of the rounded flownets2 flow2 * div_flow and
    flownetsd flow2 / div_flow, their ChannelNorms, both warps and brightness-error norms, widened and rounded."""
    from vec_vad_amd import _lib as L
    B, H, W = 2, 64, 96
    x, s2f2, sdf2 = _glue_inputs(B, H, W, 9)
    sdf2 = (sdf2.float() * 20.0).half()                       # flownetsd's flow2 is divided by div_flow
    up = lambda t: F.interpolate(t, scale_factor=4, mode='nearest')
    s2 = up(s2f2 * 20.0)
    sdfl = up(sdf2 / 20.0)
    cn = lambda t: torch.from_numpy(HR.channelnorm_fwd(t.numpy()))
    rs = lambda f: torch.from_numpy(HR.resample2d_fwd(x[:, 3:].numpy(), f.numpy()))
    ref = torch.cat((x[:, :3], sdfl, s2, cn(sdfl), cn(s2), cn(x[:, :3] - rs(sdfl)), cn(x[:, :3] - rs(s2))), 1)
    assert ref.dtype == torch.float16
    x6, img1, s2b, sdb = _nhwc(x, 8), _nhwc(x[:, 3:], 8), _nhwc(s2f2, 8), _nhwc(sdf2, 8)
    out = torch.zeros(B, H, W, 16, dtype=torch.float16, device='cuda')
    L.check(L.lib().vv_fusion_pack11_f16(x6.data_ptr(), img1.data_ptr(), s2b.data_ptr(), 8, sdb.data_ptr(), 8, B, H, W, 20.0,
                                         out.data_ptr(), torch.cuda.current_stream().cuda_stream), 'fusion_pack11_f16')
    torch.cuda.synchronize()
    o = out.cpu()
    _within_one_ulp(o[..., :11].permute(0, 3, 1, 2), ref)
    assert float(o[..., 11:].abs().max()) == 0


def _pool_bytes(net):
    return sum(t.numel() * t.element_size() for ts in net._pool.by_key.values() for t in ts)


def _bars(out, ref):
    out, ref = out.double(), ref.double()
    d = (out - ref).abs()
    return float(d.max()), 3.5e-3 * float(ref.abs().max()), float(d.mean()), 1.6e-3 * float(ref.abs().mean())


@pytest.mark.gpu
def test_flownet2_fp16_forward_vs_fp32_oracle(monkeypatch):
    from oracle import flownet2_oracle as FO
    from vec_vad_amd.flownet2 import FlowNet2
    torch.set_num_threads(min(8, torch.get_num_threads()))
    net32, sd, g = _seeded_sd()
    net32.load_state_dict(sd)
    net32 = net32.cuda().eval()
    net = FlowNet2(fp16=True)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    inp = _inputs()
    out = net(inp.cuda()).cpu()
    assert out.dtype == torch.float32 and list(out.shape) == list(g['out_shape'])
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, out.half().float())               # fp16-valued
    # the imported reference's own half graph (the fp16 golden), and the fp32 oracle
    gold = torch.from_numpy(load_golden('flownet2_fp16_128x192')['out']).float()
    mx, mx_bar, mean, mean_bar = _bars(out, gold)
    print('vs fp16 golden: max %.3g (bar %.3g) mean %.3g (bar %.3g)' % (mx, mx_bar, mean, mean_bar))
    assert mx <= mx_bar and mean <= mean_bar, (mx, mx_bar, mean, mean_bar)
    ref = FO.flownet2_forward(sd, inp)
    mx, mx_bar, mean, mean_bar = _bars(out, ref)
    print('vs fp32 oracle: max %.3g (bar %.3g) mean %.3g (bar %.3g)' % (mx, mx_bar, mean, mean_bar))
    assert mx <= mx_bar and mean <= mean_bar, (mx, mx_bar, mean, mean_bar)
    out32 = net32(inp.cuda()).cpu()
    assert not torch.equal(out, out32)                        # the fp16 path ran
    # a float16 input returns float16
    out_h = net(inp.half().cuda())
    assert out_h.dtype == torch.float16 and torch.equal(out_h.float().cpu(), out)
    # hipGraph replay, the serial schedule, every fork point of the FlowNetSD branch: the same bits
    assert torch.equal(net.forward_graphed(inp.cuda()).cpu(), out)
    assert torch.equal(net.forward_graphed(inp.cuda()).cpu(), out)
    monkeypatch.setenv('VV_FN2_OVERLAP', '0')
    assert torch.equal(net(inp.cuda()).cpu(), out)
    monkeypatch.delenv('VV_FN2_OVERLAP')
    for at in ('0', '2'):
        monkeypatch.setenv('VV_FN2_SD_AT', at)
        assert torch.equal(net(inp.cuda()).cpu(), out)
    monkeypatch.delenv('VV_FN2_SD_AT')
    # activation pool: fp16 storage
    assert _pool_bytes(net) <= 0.55 * _pool_bytes(net32), (_pool_bytes(net), _pool_bytes(net32))


@pytest.mark.gpu
def test_flownet2_fp16_fullsize_vs_fp32():
    """1024 x 448 (the benchmark size), the golden's seeded weights (what the bars were measured with): against the fp32 HIP forward
    (itself pinned to the fp32 oracle at 1e-3 x max), replay bit-equal."""
    from vec_vad_amd.flownet2 import FlowNet2
    net32, sd, _ = _seeded_sd()
    net32.load_state_dict(sd)
    net32 = net32.cuda().eval()
    net = FlowNet2(fp16=True)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(1, 3, 2, 448, 1024, generator=g) * 255).cuda()
    ref = net32(x).cpu()
    out = net(x).cpu()
    assert bool(torch.isfinite(out).all())
    mx, mx_bar, mean, mean_bar = _bars(out, ref)
    assert mx <= mx_bar and mean <= mean_bar, (mx, mx_bar, mean, mean_bar)
    assert torch.equal(net.forward_graphed(x).cpu(), out)


@pytest.mark.gpu
def test_calc_optical_flow_fp16_driver():
    import calc_optical_flow as COF
    from vec_vad_amd.flownet2 import FlowNet2
    net32, sd, _ = _seeded_sd()
    net32.load_state_dict(sd)
    net32 = net32.cuda().eval()
    net = FlowNet2(fp16=True)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    rng = np.random.default_rng(3)
    base = rng.integers(0, 255, (1, 3, 240, 360), dtype=np.uint8)
    frames = np.concatenate([base, np.roll(base, 2, axis=3), np.roll(base, 4, axis=3)], 0)
    ref = COF.flow_of_frames(net32, frames, (0, 1, 2)).cpu()
    out = COF.flow_of_frames(net, frames, (0, 1, 2)).cpu()
    assert out.dtype == torch.float32 and list(out.shape) == [240, 360, 2]
    mx, mx_bar, mean, mean_bar = _bars(out, ref)
    assert mx <= mx_bar and mean <= mean_bar, (mx, mx_bar, mean, mean_bar)
