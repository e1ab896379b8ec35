"""The float64 restatements of tests/train_ops_restatement.py against torch autograd of the nn modules the reference model uses
(model/unet.py: nn.ConvTranspose2d(k3, s2, p1, op1), nn.BatchNorm2d -> nn.ReLU -> nn.MaxPool2d(2), nn.Conv2d(C, oc, 1); train.py:
torch.optim.Adam(eps=1e-7)) and of the eval-mode nn.Conv2d(k3, p1) -> nn.BatchNorm2d pair.
They guard the reference side of every test in tests/test_gpu_train_ops.py and tests/test_gpu_outconv.py and need no GPU.  Everything runs in float64 on small
shapes: agreement to 1e-11 of the tensor's maximum (two float64 evaluations that differ in summation order only)."""
import numpy as np
import pytest
import torch

import train_ops_restatement as R

F64 = torch.float64


def _close(got, ref, tol=1e-11):
    scale = max(ref.abs().max().item(), 1e-300)
    err = (got - ref).abs().max().item()
    assert err <= tol * scale, (err, scale)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize('B,H,W,Cin,Cout', [(2, 4, 4, 5, 3), (1, 3, 5, 2, 4), (3, 1, 1, 3, 2)])
def test_transposed_conv_restatement_matches_autograd(B, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(B * 100 + H * 10 + Cin)
    m = torch.nn.ConvTranspose2d(Cin, Cout, 3, stride=2, padding=1, output_padding=1).double()
    with torch.no_grad():
        m.weight.copy_(torch.randn(Cin, Cout, 3, 3, generator=g, dtype=F64))
        m.bias.copy_(torch.randn(Cout, generator=g, dtype=F64))
    pre = torch.randn(B, H, W, Cin, generator=g, dtype=F64)
    a, b = torch.rand(Cin, generator=g, dtype=F64) + 0.5, torch.randn(Cin, generator=g, dtype=F64) * 0.2
    x = R.act_in(pre, a, b).requires_grad_(True)
    dy = torch.randn(B, 2 * H, 2 * W, Cout, generator=g, dtype=F64)
    y = m(_nchw(x))
    assert y.shape == (B, Cout, 2 * H, 2 * W)
    y.backward(_nchw(dy))
    _close(R.convT_forward(x.detach(), m.weight.detach(), m.bias.detach()), _nhwc(y.detach()))
    _close(R.convT_data_gradient(dy, m.weight.detach()), x.grad)
    _close(R.convT_weight_gradient(x.detach(), dy), m.weight.grad)
    _close(dy.sum((0, 1, 2)), m.bias.grad)                        # the bias gradient vv_bias_grad / vv_bias_from_partials form


@pytest.mark.parametrize('B,H,C,tiles', [(4, 6, 5, 4), (3, 2, 7, 1), (1, 1, 3, 1)])
def test_batchnorm_finalize_restatement_matches_module(B, H, C, tiles):
    """train mode: a, b, mean, invstd and the running buffers after one forward of nn.BatchNorm2d(momentum 0.1); eval mode: a, b from
    the running buffers.  The per-tile sums are those of `tiles` slices of the batch.  B = H = 1: one value per channel, the unbiased
    variance of the running update is undefined (torch refuses that forward), the restatement falls back to the biased one."""
    g = torch.Generator().manual_seed(B * 10 + C)
    x = torch.randn(B, H, H, C, generator=g, dtype=F64) * 1.5 + 3.0
    bn = torch.nn.BatchNorm2d(C, eps=1e-5, momentum=0.1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.running_mean.copy_(torch.randn(C, generator=g, dtype=F64))
        bn.running_var.copy_(torch.rand(C, generator=g, dtype=F64) + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    parts = x.reshape(-1, C).chunk(tiles)
    stats = torch.stack([torch.stack([p.sum(0), (p * p).sum(0)]) for p in parts])
    count = B * H * H
    a, b, mean, invstd, rm, rv = R.bn_finalize(stats, count, bn.weight.detach(), bn.bias.detach(), rm0, rv0, 0.1, 1e-5, True)
    if count > 1:
        bn.train()
        out = bn(_nchw(x)).detach()
        _close(a * x + b, _nhwc(out), 1e-9)                       # E[x^2] - mean^2 in float64 at mean 3, std 1.5
        _close(rm, bn.running_mean)
        _close(rv, bn.running_var, 1e-9)
        _close(mean, x.reshape(-1, C).mean(0))
        _close(invstd, 1 / torch.sqrt(x.reshape(-1, C).var(0, unbiased=False) + 1e-5), 1e-9)
    else:
        _close(mean, x.reshape(-1, C)[0])
        _close(invstd, torch.full((C,), 1e-5, dtype=F64) ** -0.5, 1e-6)
        _close(rv, 0.9 * rv0, 1e-6)                               # biased variance 0 (to round-off) instead of a division by zero
    with torch.no_grad():
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    bn.eval()
    a, b, mean, invstd, rm, rv = R.bn_finalize(None, count, bn.weight.detach(), bn.bias.detach(), rm0, rv0, 0.1, 1e-5, False)
    _close(a * x + b, _nhwc(bn(_nchw(x)).detach()))
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and torch.equal(mean, rm0)


def _bn_case(B, H, C, seed, ties):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(B, H, H, C, generator=g, dtype=F64)
    if ties:                                                     # exact ties inside windows: copy the top-left value over its right neighbour
        y[:, 0::2, 1::2] = torch.where(torch.rand(B, H // 2, H // 2, C, generator=g) < 0.5, y[:, 0::2, 0::2], y[:, 0::2, 1::2])
        y[:, 1::2, 1::2] = torch.where(torch.rand(B, H // 2, H // 2, C, generator=g) < 0.3, y[:, 0::2, 1::2], y[:, 1::2, 1::2])
    gamma = torch.rand(C, generator=g, dtype=F64) + 0.5
    beta = torch.randn(C, generator=g, dtype=F64) * 0.3 + (0.5 if ties else 0.0)
    dA = torch.randn(B, H, H, C, generator=g, dtype=F64)
    dP = torch.randn(B, H // 2, H // 2, C, generator=g, dtype=F64)
    return y, gamma, beta, dA, dP


@pytest.mark.parametrize('ties', [False, True])
@pytest.mark.parametrize('pool', [False, True])
def test_batchnorm_relu_pool_backward_restatement_matches_autograd(pool, ties):
    """loss = <relu(bn(y)), dA> + <maxpool2(relu(bn(y))), dP>, train-mode nn.BatchNorm2d: d loss / d y, d gamma, d beta.  `ties`: half of
    the windows hold the same (mostly positive) activation twice or three times -- at::max_pool2d sends the gradient to the first."""
    B, H, C = 3, 6, 5
    y, gamma, beta, dA, dP = _bn_case(B, H, C, 11 + pool, ties)
    bn = torch.nn.BatchNorm2d(C, eps=1e-5).double().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    yy = _nchw(y).requires_grad_(True)
    act = torch.relu(bn(yy))
    loss = (act * _nchw(dA)).sum()
    if pool:
        loss = loss + (torch.nn.MaxPool2d(2)(act) * _nchw(dP)).sum()
    loss.backward()
    flat = y.reshape(-1, C)
    mean, invstd = flat.mean(0), 1 / torch.sqrt(flat.var(0, unbiased=False) + 1e-5)
    a = gamma * invstd
    b = beta - mean * a
    if ties:
        actr = R.act_in(y, a, b)
        win = actr.reshape(B, H // 2, 2, H // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(-1, 4)
        top = win.max(1, keepdim=True).values
        assert (((win == top).sum(1) > 1) & (top[:, 0] > 0)).float().mean().item() > 0.1          # the case really has positive ties
    dy, dgamma, dbeta, _ = R.bn_relu_pool_backward(y, a, b, mean, invstd, gamma, dA, dP if pool else None)
    _close(dy, _nhwc(yy.grad), 1e-10)
    _close(dgamma, bn.weight.grad, 1e-10)
    _close(dbeta, bn.bias.grad, 1e-10)


def test_pool_route_sends_gradient_to_first_maximum():
    act = torch.tensor([[1.0, 1.0, 0.0, 2.0], [1.0, 0.5, 2.0, 2.0]], dtype=F64).reshape(1, 2, 4, 1)
    r = R.pool_route(act, torch.tensor([5.0, 7.0], dtype=F64).reshape(1, 1, 2, 1))
    assert r.reshape(2, 4).tolist() == [[5.0, 0.0, 0.0, 7.0], [0.0, 0.0, 0.0, 0.0]]


@pytest.mark.parametrize('B,HW,C,oc', [(3, 7, 8, 3), (2, 5, 4, 2), (1, 3, 8, 1), (2, 4, 8, 4)])
def test_output_conv_restatement_matches_autograd(B, HW, C, oc):
    """nn.Conv2d(C, oc, 1) on relu(a y + b), loss = 0.5 gscale sum (out - tgt)^2: out, score, d loss / d out, and the gradients with
    respect to the activation, the weight and the bias; the BatchNorm-backward sums against their definition on the autograd dA."""
    g = torch.Generator().manual_seed(B * 1000 + HW * 10 + oc)
    conv = torch.nn.Conv2d(C, oc, 1).double()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(oc, C, 1, 1, generator=g, dtype=F64))
        conv.bias.copy_(torch.randn(oc, generator=g, dtype=F64))
    y = torch.randn(B, HW, C, generator=g, dtype=F64)
    a, b = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64) * 0.3
    mean, invstd = torch.randn(C, generator=g, dtype=F64) * 0.1, torch.rand(C, generator=g, dtype=F64) + 0.5
    tgt = torch.randn(B, HW, oc, generator=g, dtype=F64)
    gscale = 0.37
    v = R.act_in(y, a, b).requires_grad_(True)
    out = conv(v.permute(0, 2, 1)[..., None])[..., 0].permute(0, 2, 1)          # [B, HW, oc]
    (0.5 * gscale * ((out - tgt) ** 2).sum()).backward()
    w, bias = conv.weight.detach()[:, :, 0, 0], conv.bias.detach()
    out4, score, dout4 = R.outconv_forward(y, a, b, w, bias, oc, tgt, gscale)
    _close(out4[..., :oc], out.detach())
    _close(score, ((out.detach() - tgt) ** 2).sum((1, 2)))
    _close(dout4[..., :oc], gscale * (out.detach() - tgt))
    assert out4[..., oc:].abs().sum().item() == 0.0 and dout4[..., oc:].abs().sum().item() == 0.0
    dA, dWc, dbc, dW, db, s1, s2 = R.outconv_backward(dout4, y, a, b, w, mean, invstd)
    _close(dA, v.grad)
    _close(dW[:oc], conv.weight.grad[:, :, 0, 0])
    _close(db[:oc], conv.bias.grad)
    _close(dWc.sum(0), dW)
    _close(dbc.sum(0), db)
    assert dWc[:, oc:].abs().sum().item() == 0.0 and dbc[:, oc:].abs().sum().item() == 0.0
    gate = (v.detach() > 0).double()
    _close(s1, (v.grad * gate).sum(1))
    _close(s2, (v.grad * gate * (y - mean) * invstd).sum(1))
    # dA_stored replaces the dA of the sums only
    st = dA + 0.25
    r2 = R.outconv_backward(dout4, y, a, b, w, mean, invstd, dA_stored=st)
    assert torch.equal(r2[0], dA) and torch.equal(r2[1], dWc)
    _close(r2[5], (st * gate).sum(1))
    _close(r2[6], (st * gate * (y - mean) * invstd).sum(1))


@pytest.mark.parametrize('Cin,Cout', [(3, 5), (4, 2)])
def test_fold_bn_restatement_matches_conv_then_eval_batchnorm(Cin, Cout):
    """nn.Conv2d(k3, p1) -> nn.BatchNorm2d.eval() equals the convolution with the folded filter and bias (running_var down to 1e-6)"""
    g = torch.Generator().manual_seed(Cin * 10 + Cout)
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).double()
    bn = torch.nn.BatchNorm2d(Cout, eps=1e-5).double().eval()
    with torch.no_grad():
        conv.weight.copy_(torch.randn(Cout, Cin, 3, 3, generator=g, dtype=F64))
        conv.bias.copy_(torch.randn(Cout, generator=g, dtype=F64))
        bn.weight.copy_(torch.rand(Cout, generator=g, dtype=F64) + 0.5)
        bn.bias.copy_(torch.randn(Cout, generator=g, dtype=F64))
        bn.running_mean.copy_(torch.randn(Cout, generator=g, dtype=F64))
        bn.running_var.copy_(10.0 ** (-6 * torch.rand(Cout, generator=g, dtype=F64)))
        bn.running_var[0] = 1e-6
        x = torch.randn(2, Cin, 5, 4, generator=g, dtype=F64)
        ref = bn(conv(x))
        wf, bf = R.fold_bn(conv.weight.reshape(Cout, -1), conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, 1e-5)
        _close(torch.nn.functional.conv2d(x, wf.view(Cout, Cin, 3, 3), bf, padding=1), ref)


def test_adam_restatement_matches_torch_optimizer():
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(3, 40, generator=g, dtype=F64)
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-7, weight_decay=0.0)
    q, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t in range(1, 5):
        grad = torch.randn(3, 40, generator=g, dtype=F64) * (10.0 ** (t - 3))
        p.grad = grad.clone()
        opt.step()
        q, m, v = R.adam_step(q, grad, m, v, t, 1e-3, 0.9, 0.999, 1e-7)
        _close(q, p.detach(), 1e-13)
        _close(m, opt.state[p]['exp_avg'], 1e-13)
        _close(v, opt.state[p]['exp_avg_sq'], 1e-13)
    # grad_scale scales the gradient before anything else
    a = R.adam_step(q, grad, m, v, 5, 1e-3, 0.9, 0.999, 1e-7, grad_scale=0.25)
    b = R.adam_step(q, grad * 0.25, m, v, 5, 1e-3, 0.9, 0.999, 1e-7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_bucket_major_layout_is_a_permutation_with_contiguous_buckets():
    G, bounds = 3, [0, 8, 12, 40]
    grad = torch.arange(G * 40, dtype=F64).reshape(G, 40)
    flat = R.to_bucket_major(grad, bounds)
    assert sorted(flat.tolist()) == grad.reshape(-1).tolist()
    for lo, hi in zip(bounds[:-1], bounds[1:]):                   # bucket k: [G, width] at offset G * lo
        assert torch.equal(flat[G * lo:G * hi].reshape(G, hi - lo), grad[:, lo:hi])
    assert torch.equal(R.from_bucket_major(flat, G, bounds), grad)
    assert torch.equal(R.to_bucket_major(grad, [0, 40]), grad.reshape(-1))


def test_adapter_restatements_match_elementwise_definitions():
    rng = np.random.RandomState(3)
    N, T, Tf, HW = 4, 3, 2, 6
    raw = rng.randint(0, 256, (N, T, HW, 3)).astype(np.uint8)
    flow = rng.randn(N, Tf, HW, 2).astype(np.float32)
    idx = np.array([2, 0, 2])
    x, xof = R.cube_gather(raw, flow, idx)
    assert x.dtype == np.float32 and x.shape == (3, HW, 3 * T) and xof.shape == (3, HW, 2 * Tf)
    for bi, n in enumerate(idx):
        for t in range(T):
            for c in range(3):
                assert np.array_equal(x[bi, :, t * 3 + c], raw[n, t, :, c].astype(np.float32) / np.float32(255))
        for t in range(Tf):
            for c in range(2):
                assert np.array_equal(xof[bi, :, t * 2 + c], flow[n, t, :, c])
    x_all, none = R.cube_gather(raw, None)
    assert none is None and np.array_equal(x_all[2], x[0])
    # the reference's adapter (vad_datasets.py: [T, H, W, C] -> [H, W, T C] of a ToTensor()-scaled cube)
    assert np.array_equal(x_all[1], np.transpose(raw[1].astype(np.float32) / np.float32(255), (1, 0, 2)).reshape(HW, -1))

    cube = torch.randn(7, 5, dtype=F64)
    chmap = torch.tensor([[0, 1, -1, 3, 4, -1, -1, -1], [-1, 4, 4, 0, 2, 1, -1, -1]])
    out = R.cube_erase(cube, chmap)
    for gi in range(2):
        for k in range(8):
            s = int(chmap[gi, k])
            assert torch.equal(out[gi, :, k], cube[:, s] if s >= 0 else torch.zeros(7, dtype=F64))

    y = torch.randn(2, 4, 6, 5, dtype=F64)
    a, b = torch.rand(5, dtype=F64) + 0.5, torch.randn(5, dtype=F64)
    ref = torch.nn.MaxPool2d(2)(torch.relu(_nchw(y) * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)))
    assert torch.equal(R.pool_act(y, a, b), _nhwc(ref))

    src = torch.randn(2, 5, 6, dtype=F64)
    assert torch.equal(R.nchw_to_nhwc(src), src.transpose(1, 2))
    out4 = torch.randn(2, 6, 4, dtype=F64)
    dst = torch.randn(2, 7, 6, dtype=F64)
    d2 = R.out4_to_nchw(out4, dst, 3, 2)
    assert torch.equal(d2[:, :2], dst[:, :2]) and torch.equal(d2[:, 5:], dst[:, 5:])
    for c in range(3):
        assert torch.equal(d2[:, 2 + c], out4[:, :, c])
    back = R.nchw_to_out4(d2, 3, 2)
    assert torch.equal(back[:, :, :3], out4[:, :, :3]) and back[:, :, 3].abs().max().item() == 0.0
