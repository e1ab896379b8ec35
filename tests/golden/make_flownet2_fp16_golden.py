"""Golden for FlowNet2(fp16=True) from the REAL reference python modules (authoring container only).

Same recipe as make_flownet2_golden.py (formula-seeded weights, the same 128x192 input pair, the three CUDA ops stubbed by the
numpy restatements of oracle/flow_ops_oracle.py), run as the reference's FlowNet2(fp16=True) + .half() on CPU.  As written, the
reference's fp16 graph raises TypeError: Correlation and every Resample2d are wrapped in nn.Sequential(tofp32(), op, tofp16())
(FlowNetC.py:31, flownet2.py:29-49) and then called with two tensors (FlowNetC.py:90, flownet2.py:79).  The only patch is the
two-argument form of those five wrappers (widen both inputs, run the op, round the result), plus a ChannelNorm stub that widens,
computes and rounds (its CUDA op is float-only).  Only outputs are stored."""
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import flow_ops_oracle as ops  # noqa: E402
from oracle import flownet2_oracle as FO  # noqa: E402
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from _util import digest  # noqa: E402

sys.modules['png'] = types.ModuleType('png')
import torch.nn.init as I  # noqa: E402
I.uniform = I.uniform_
I.xavier_uniform = I.xavier_uniform_


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


class Correlation(nn.Module):
    def __init__(self, pad_size=0, kernel_size=0, max_displacement=0, stride1=1, stride2=2, corr_multiply=1):
        super().__init__()
        self.a = (pad_size, kernel_size, max_displacement, stride1, stride2, corr_multiply)

    def forward(self, x, y):
        return _t(ops.correlation_fwd(x.detach().numpy(), y.detach().numpy(), *self.a))


class Resample2d(nn.Module):
    def __init__(self, kernel_size=1):
        super().__init__()

    def forward(self, x, f):
        return _t(ops.resample2d_fwd(x.contiguous().detach().numpy(), f.contiguous().detach().numpy()))


class ChannelNorm(nn.Module):
    """widen, compute, round (the CUDA op is float-only)"""
    def __init__(self, norm_deg=2):
        super().__init__()

    def forward(self, x):
        return _t(ops.channelnorm_fwd(x.float().contiguous().detach().numpy())).to(x.dtype)


m = types.ModuleType('FlowNet2_src.models.components.ops')
m.Correlation, m.Resample2d, m.ChannelNorm = Correlation, Resample2d, ChannelNorm
sys.modules['FlowNet2_src.models.components.ops'] = m
sys.path.insert(0, '/root/reference')
from FlowNet2_src.models.flownet2 import FlowNet2  # noqa: E402


class TwoArg(nn.Module):
    """nn.Sequential(tofp32(), op, tofp16()) as the two-argument op the reference calls it as."""
    def __init__(self, wrapped):
        super().__init__()
        self.op = wrapped[1]

    def forward(self, a, b):
        return self.op(a.float(), b.float()).half()


def main():
    torch.manual_seed(0)
    net = FlowNet2(fp16=True)
    net.flownetc.corr = TwoArg(net.flownetc.corr)
    for i in (1, 2, 3, 4):
        setattr(net, 'resample%d' % i, TwoArg(getattr(net, 'resample%d' % i)))
    net.eval()
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = FO.seeded_state_dict(shapes, seed=0)
    net.load_state_dict(sd)
    net.half()
    H, W = 128, 192
    rng = np.random.default_rng(42)
    base = rng.uniform(0, 255, (1, 3, 1, H, W)).astype(np.float32)
    second = np.roll(base, (2, 3), axis=(3, 4)) + rng.normal(0, 2, base.shape).astype(np.float32)
    inp = torch.from_numpy(np.clip(np.concatenate([base, second], 2), 0, 255).astype(np.float32))
    t0 = time.perf_counter()
    with torch.no_grad():
        out = net(inp.half())
    dt = time.perf_counter() - t0
    assert out.dtype == torch.float16
    np.savez_compressed(os.path.join(HERE, 'flownet2_fp16_128x192.npz'), out=out.numpy(), out_digest=digest(out.float()),
                        out_shape=np.array(out.shape))
    print('flownet2 fp16 golden written in %.2f s; |flow| max %g' % (dt, float(out.float().abs().max())))


if __name__ == '__main__':
    main()
