"""VV_FUSE_BN_APPLY: the BatchNorm-backward apply pass folded into the data- and weight-gradient loads (vv_bn_bwd_sums + VV_IN_BNBWD /
vv_wgrad_params.dy_bn) must give the same bits as the separate apply pass (VV_FUSE_BN_APPLY=0): losses, every gradient (incl. dgamma /
dbeta) and the Adam state after three fused fp32 train steps of Net4, and a single data-gradient / weight-gradient launch against
vv_bn_bwd_apply + the plain launch."""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def _steps(fold, B, graph, sums, nsteps=3):
    from oracle import unet_oracle as O
    from model.unet import SelfCompleteNet4
    from vec_vad_amd.trainer import FusedTrainer
    env = {'VV_FUSE_BN_APPLY': fold, 'VV_GRAPH': graph, 'VV_FUSE_BN_SUMS': sums}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        net = SelfCompleteNet4(features_root=32, tot_raw_num=5, tot_of_num=1, border_mode='predict', rawRange=None,
                               useFlow=True, padding=False)
        net.load_state_dict(O.seeded_state_dict('net4', nf=32, padding=False, seed=1))
        net = net.cuda().train()
        tr = FusedTrainer(net)
        losses = []
        for s in range(nsteps):
            raw, flow = O.seeded_cubes(B, 1, 10 + s)
            ws = tr.step_cubes(torch.from_numpy(raw).cuda(), torch.from_numpy(flow).cuda(), torch.arange(B, device='cuda'))
            losses.append(torch.stack([torch.as_tensor(v, device='cuda').float() for v in tr.losses(ws)]))
        torch.cuda.synchronize()
        bank = tr.bank
        return (torch.stack(losses), bank.grads.clone(), bank.params.clone(),
                bank.adam_m.clone() if bank.adam_m is not None else None, bank.adam_v.clone() if bank.adam_v is not None else None)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize('B,graph,sums', [(256, '1', '1'), (32, '0', '1'), (37, '1', '0'), (32, '1', '0')])
def test_fold_bitwise_equal_train_steps(B, graph, sums):
    ref = _steps('0', B, graph, sums)
    out = _steps('1', B, graph, sums)
    for name, r, o in zip(('losses', 'grads', 'params', 'adam_m', 'adam_v'), ref, out):
        if r is None:
            assert o is None
            continue
        assert torch.equal(r, o), (name, (r - o).abs().max().item())


def _bn_setup(G, B, H, C_, g, dA_cs=None):
    M = B * H * H
    cs = dA_cs or C_
    z = torch.randn(G, M, C_, generator=g).cuda()
    dA = torch.randn(G, M, cs, generator=g).cuda()
    a = (torch.rand(G, C_, generator=g) + 0.5).cuda()
    b = (torch.randn(G, C_, generator=g) * 0.3).cuda()
    mean = (torch.randn(G, C_, generator=g) * 0.1).cuda()
    inv = (torch.rand(G, C_, generator=g) + 0.5).cuda()
    gamma = (torch.rand(G, C_, generator=g) + 0.5).cuda()
    return z, dA, a, b, mean, inv, gamma


@pytest.mark.parametrize('H,Cin,Cout,B,slice_', [(16, 32, 64, 5, False), (8, 64, 128, 9, False), (8, 256, 128, 3, True),
                                                 (16, 128, 64, 2, True), (32, 32, 32, 3, False)])
def test_fold_single_launch_bitwise(H, Cin, Cout, B, slice_):
    """one layer: vv_bn_bwd_reduce, then (a) vv_bn_bwd_apply + plain data / weight gradient, (b) vv_bn_bwd_sums + the folded launches;
    dA optionally a channel slice of a wider tensor (the concat case)"""
    from vec_vad_amd import _lib as L
    lib = L.lib()
    G = 2
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device='cpu').manual_seed(H * 7 + Cin + Cout + B)
    cs, off = (Cout + 32, 16) if slice_ else (Cout, 0)
    z, dA, a, b, mean, inv, gamma = _bn_setup(G, B, H, Cout, g, cs)
    x = torch.randn(G, B * H * H, Cin, generator=g).cuda()
    w = (torch.randn(G, Cout, Cin, 3, 3, generator=g) * 0.1).cuda()
    nblk = lib.vv_bn_bwd_nblk(B, H, H, Cout)
    part = torch.zeros(G, nblk * 2 * Cout, device='cuda')
    dz = torch.zeros(G, B * H * H, Cout, device='cuda')
    bp = L.BnBwdParams(G, B, H, H, Cout, 0, z.data_ptr(), z.stride(0), a.data_ptr(), b.data_ptr(), mean.data_ptr(), inv.data_ptr(),
                       Cout, L.view(dA, cs, off, dA.stride(0)), None, 0, dz.data_ptr(), dz.stride(0), part.data_ptr())
    L.check(lib.vv_bn_bwd_reduce(C.byref(bp), st), 'reduce')
    dg = [torch.zeros(G, Cout, device='cuda') for _ in range(4)]
    scr = torch.zeros(G, 2 * Cout, device='cuda')
    tab = torch.zeros(G, L.BNBWD_TAB_ROWS * Cout, device='cuda')
    L.check(lib.vv_bn_bwd_apply(C.byref(bp), gamma.data_ptr(), Cout, dg[0].data_ptr(), dg[1].data_ptr(), Cout, scr.data_ptr(), st), 'apply')
    L.check(lib.vv_bn_bwd_sums(C.byref(bp), gamma.data_ptr(), Cout, dg[2].data_ptr(), dg[3].data_ptr(), Cout, tab.data_ptr(),
                               tab.stride(0), st), 'sums')
    assert torch.equal(dg[0], dg[2]) and torch.equal(dg[1], dg[3])
    # data gradient (F(2x2) per-tile kernel; the 32x32 level would take the ring kernel: weight gradient only there)
    if H != 32:
        ent = (L.PackEntry * 1)(L.PackEntry(0, 0, 1, Cout, Cout, Cin))
        et = torch.frombuffer(bytearray(bytes(ent)), dtype=torch.uint8).cuda()
        pk = torch.zeros(G, 16 * Cout * Cin, device='cuda')
        L.check(lib.vv_pack_wino(et.data_ptr(), 1, G, w.data_ptr(), w[0].numel(), pk.data_ptr(), pk.stride(0), Cout * Cin, st), 'pack')
        outs = []
        for fold in (False, True):
            o = torch.full((G, B * H * H, Cin), 7.0, device='cuda')
            cp = L.ConvParams(L.CONV3, L.IN_PLAIN, G, B, H, H, Cout, Cout, Cin, L.view(dz, Cout, 0, dz.stride(0)), None, None, 0,
                              L.NULL_VIEW, 0, L.CONV_NO_RING, None, pk.data_ptr(), pk.stride(0), None, 0, L.view(o, Cin, 0, o.stride(0)), None)
            if fold:
                cp.in_mode, cp.src0, cp.src1 = L.IN_BNBWD, L.view(dA, cs, off, dA.stride(0)), L.view(z, Cout, 0, z.stride(0))
                cp.a, cp.ab_gstride = tab.data_ptr(), tab.stride(0)
            L.check(lib.vv_conv_wino(C.byref(cp), st), 'dgrad')
            outs.append(o)
        assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()
    # weight gradient (Winograd form)
    ks = 2
    nsl = ((Cin + 31) // 32) * (Cout // 32) * ks
    outs = []
    for fold in (False, True):
        wpart = torch.zeros(G, nsl * 9 * 1024, device='cuda')
        wp = L.WgradParams(L.CONV3, L.IN_PLAIN, G, B, H, H, Cin, Cin, Cout, ks, L.view(x, Cin, 0, x.stride(0)), None, None, 0,
                           L.NULL_VIEW, 0, 256, None, L.view(dz, Cout, 0, dz.stride(0)), wpart.data_ptr(), wpart.stride(0))
        if fold:
            wp.dy, wp.dy_z = L.view(dA, cs, off, dA.stride(0)), L.view(z, Cout, 0, z.stride(0))
            wp.dy_bn, wp.dy_bn_gstride = tab.data_ptr(), tab.stride(0)
        L.check(lib.vv_wgrad_mfma(C.byref(wp), st), 'wgrad')
        outs.append(wpart)
    assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()
