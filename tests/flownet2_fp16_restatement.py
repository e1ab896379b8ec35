"""CPU restatement of FlowNet2's half graph (test infrastructure): the reference's FlowNet2(fp16=True) after .half(), with its
``nn.Sequential(tofp32(), op, tofp16())`` wrappers of Correlation / Resample2d taken as two-argument ops (FlowNetC.py:31,
flownet2.py:29-49).  Convolutions, LeakyReLU, up-sampling and the arithmetic between the sub-networks are torch CPU half ops in
the reference's order (the graph of oracle/flownet2_oracle.py); the three native ops are the oracle's numpy restatements on widened
(fp32) inputs, their results rounded to fp16 once.  ChannelNorm gets the same treatment (its CUDA op is float-only).
Pinned to tests/golden/flownet2_fp16_128x192.npz (a run of the imported reference) by test_flownet2_fp16.py; the GPU tests use it
where the reference does not exist."""
import contextlib

import numpy as np
import torch

from oracle import flow_ops_oracle as ops
from oracle import flownet2_oracle as FO


def correlation_fwd(a, b, *args):
    return ops.correlation_fwd(np.asarray(a, np.float32), np.asarray(b, np.float32), *args).astype(np.float16)


def resample2d_fwd(img, flow):
    return ops.resample2d_fwd(np.asarray(img, np.float32), np.asarray(flow, np.float32)).astype(np.float16)


def channelnorm_fwd(x):
    return ops.channelnorm_fwd(np.asarray(x, np.float32)).astype(np.float16)


class _HalfOps:
    """The oracle's numpy ops with widen -> compute in fp32 -> round to fp16."""
    correlation_fwd = staticmethod(correlation_fwd)
    resample2d_fwd = staticmethod(resample2d_fwd)
    channelnorm_fwd = staticmethod(channelnorm_fwd)


@contextlib.contextmanager
def _half_native_ops():
    saved = FO.ops
    FO.ops = _HalfOps
    try:
        yield
    finally:
        FO.ops = saved


@torch.no_grad()
def flownet2_fp16_forward(sd, inputs, rgb_max=255.0, div_flow=20.0, return_parts=False):
    """sd: fp32 reference-named state_dict (rounded to fp16 here, = .half()); inputs [B,3,2,H,W] 0..255 -> fp16 flow [B,2,H,W]."""
    sd16 = {k: v.half() for k, v in sd.items()}
    with _half_native_ops():
        return FO.flownet2_forward(sd16, inputs.half(), rgb_max=rgb_max, div_flow=div_flow, return_parts=return_parts)
