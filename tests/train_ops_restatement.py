"""Plain torch / numpy restatements of the operations a train step of the UNet bank runs besides its 3x3 convolutions (and of the
eval-mode BatchNorm folding), one function per operation, written from the operation's definition and not from the HIP kernels (vec_vad_amd/csrc/vv_conv.hip, vv_wgrad.hip,
vv_elem.hip).  Every function computes in the dtype of its arguments: float64 tensors give the reference of tests/test_gpu_train_ops.py
and tests/test_gpu_outconv.py, the same call on float32 tensors gives the "plain float32 evaluation" those tests measure the kernels' round-off against.
tests/test_train_ops_host.py checks each function in float64 against torch autograd of the nn modules the reference model uses
(model/unet.py: nn.ConvTranspose2d(k3, s2, p1, op1), nn.BatchNorm2d -> nn.ReLU -> nn.MaxPool2d(2), nn.Conv2d(C, oc, 1); train.py:
torch.optim.Adam(eps=1e-7)).

Activations are NHWC ([B, H, W, C]) as the kernels store them; filters keep the PyTorch parameter layouts.
"""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------- ConvTranspose2d(k3, s2, p1, op1)
# y[b, 2i - 1 + ky, 2j - 1 + kx, co] += x[b, i, j, ci] * W[ci, co, ky, kx]      (stride 2, padding 1; output_padding 1 -> 2H x 2W)

def act_in(x, a, b):
    """how a VV_IN_ACT launch reads its input: relu(a[c] * x + b[c])"""
    return torch.relu(a * x + b)


def convT_forward(x, w, bias=None):
    """x [B, H, W, Cin], w [Cin, Cout, 3, 3], bias [Cout] -> [B, 2H, 2W, Cout]"""
    B, H, W, _ = x.shape
    Cout = w.shape[1]
    buf = x.new_zeros(B, 2 * H + 1, 2 * W + 1, Cout)          # buf[r + 1] = output row r, r = -1 .. 2H - 1
    for ky in range(3):
        for kx in range(3):
            buf[:, ky:ky + 2 * H - 1:2, kx:kx + 2 * W - 1:2] += x @ w[:, :, ky, kx]
    y = buf[:, 1:, 1:]
    return y + bias if bias is not None else y.clone()


def _dy_taps(dy):
    """dy [B, 2H, 2W, Cout] -> the nine [B, H, W, Cout] tensors dy[b, 2i - 1 + ky, 2j - 1 + kx] (zero outside)"""
    B, H2, W2, C = dy.shape
    pad = dy.new_zeros(B, H2 + 1, W2 + 1, C)
    pad[:, 1:, 1:] = dy
    return [[pad[:, ky:ky + H2 - 1:2, kx:kx + W2 - 1:2] for kx in range(3)] for ky in range(3)]


def convT_data_gradient(dy, w):
    """dx[b, i, j, ci] = sum_{co, ky, kx} dy[b, 2i - 1 + ky, 2j - 1 + kx, co] W[ci, co, ky, kx]"""
    taps = _dy_taps(dy)
    dx = 0
    for ky in range(3):
        for kx in range(3):
            dx = dx + taps[ky][kx] @ w[:, :, ky, kx].t()
    return dx


def convT_weight_gradient(x, dy):
    """dW[ci, co, ky, kx] = sum_{b, i, j} x[b, i, j, ci] dy[b, 2i - 1 + ky, 2j - 1 + kx, co]"""
    taps = _dy_taps(dy)
    Cin, Cout = x.shape[-1], dy.shape[-1]
    dw = x.new_zeros(Cin, Cout, 3, 3)
    xf = x.reshape(-1, Cin)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = xf.t() @ taps[ky][kx].reshape(-1, Cout)
    return dw


# ---------------------------------------------------------------------------------------------- BatchNorm2d(eps, momentum)

def bn_finalize(stats, count, gamma, beta, running_mean, running_var, momentum, eps, train):
    """stats [ntiles, 2, C]: per-tile sums and sums of squares of the normalised tensor; count = its pixels per channel.
    -> a, b, mean, invstd, running_mean', running_var' (eval mode: statistics = the running buffers, which stay as they are)"""
    if train:
        mean = stats[:, 0].sum(0) / count
        var = (stats[:, 1].sum(0) / count - mean * mean).clamp_min(0)          # biased
        unbiased = var * count / (count - 1) if count > 1 else var
        rm = (1 - momentum) * running_mean + momentum * mean
        rv = (1 - momentum) * running_var + momentum * unbiased
    else:
        mean, var, rm, rv = running_mean, running_var, running_mean, running_var
    invstd = 1 / torch.sqrt(var + eps)
    a = gamma * invstd
    return a, beta - mean * a, mean, invstd, rm, rv


def pool_first_max(act):
    """act [B, H, W, C] -> index 0..3 (row-major inside the 2x2 window) of the FIRST maximum of every window, [B, H/2, W/2, C]"""
    B, H, W, C = act.shape
    win = act.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    best, idx = win[..., 0], torch.zeros(win.shape[:-1], dtype=torch.long)
    for k in range(1, 4):
        up = win[..., k] > best
        best, idx = torch.where(up, win[..., k], best), torch.where(up, torch.full_like(idx, k), idx)
    return idx


def pool_route(act, dpool):
    """gradient of MaxPool2d(2) wrt its input: dpool [B, H/2, W/2, C] lands on the first maximum of its window, zero elsewhere"""
    B, H, W, C = act.shape
    onehot = torch.nn.functional.one_hot(pool_first_max(act), 4).to(dpool.dtype)          # [B, H2, W2, C, 4]
    r = (onehot * dpool[..., None]).reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3)
    return r.reshape(B, H, W, C)


def bn_relu_pool_backward(y, a, b, mean, invstd, gamma, dA, dpool=None):
    """y [B, H, W, C] = the conv output in front of BatchNorm; activation = relu(a y + b) with a = gamma invstd, b = beta - mean a;
    dA = gradient wrt the activation, dpool = gradient wrt MaxPool2d(2)(activation) or None.  -> dy, dgamma, dbeta, dz"""
    z = a * y + b
    d = dA if dpool is None else dA + pool_route(torch.relu(z), dpool)
    dz = d * (z > 0).to(d.dtype)
    xhat = (y - mean) * invstd
    dbeta = dz.sum((0, 1, 2))
    dgamma = (dz * xhat).sum((0, 1, 2))
    n = y.shape[0] * y.shape[1] * y.shape[2]
    dy = gamma * invstd * (dz - dbeta / n - xhat * (dgamma / n))
    return dy, dgamma, dbeta, dz


# ---------------------------------------------------------------------------------------------- output conv, nn.Conv2d(C, oc, 1)
# (include/vecvad_hip.h, vv_outconv_params) one group: y [B, HW, C] = the conv output in front of the last BatchNorm, w [oc, C],
# bias [oc], tgt [B, HW, oc] = the target channels of this group; four output channels are stored, those >= oc are 0

def outconv_forward(y, a, b, w, bias, oc, tgt, gscale):
    """v = relu(a y + b); out[p][co] = bias[co] + sum_c v[p][c] W[co][c]; score[cube] = sum (out - tgt)^2; dout = gscale (out - tgt)
    -> out4 [B, HW, 4], score [B], dout4 [B, HW, 4]"""
    v = act_in(y, a, b)
    out = v @ w[:oc].t() + bias[:oc]
    e = out - tgt[..., :oc]
    out4, dout4 = y.new_zeros(y.shape[:-1] + (4,)), y.new_zeros(y.shape[:-1] + (4,))
    out4[..., :oc] = out
    dout4[..., :oc] = gscale * e
    return out4, (e * e).sum((1, 2)), dout4


def outconv_backward(dout4, y, a, b, w, mean, invstd, dA_stored=None):
    """dout4 [B, HW, 4] (channels >= oc = w.shape[0] are not read) -> dA [B, HW, C] = sum_co dout[co] W[co]; per cube dW [B, 4, C] =
    sum_p dout[p][co] v[p][c] and db [B, 4] = sum_p dout[p][co] (rows >= oc zero); their sums over the cubes [4, C], [4]; per cube the
    BatchNorm-backward sums [B, C] of g = dA [v > 0] and of g xhat, xhat = (y - mean) invstd -- of dA_stored where given (what a
    kernel stored, a bf16 rounding for instance) instead of the dA formed here"""
    oc = w.shape[0]
    v = act_in(y, a, b)
    d = dout4[..., :oc]
    dA = d @ w
    dWc, dbc = y.new_zeros(y.shape[0], 4, y.shape[-1]), y.new_zeros(y.shape[0], 4)
    dWc[:, :oc] = d.transpose(1, 2) @ v
    dbc[:, :oc] = d.sum(1)
    g = (dA if dA_stored is None else dA_stored) * (v > 0).to(y.dtype)
    xhat = (y - mean) * invstd
    return dA, dWc, dbc, dWc.sum(0), dbc.sum(0), g.sum(1), (g * xhat).sum(1)


# ---------------------------------------------------------------------------------------------- eval mode: BatchNorm folded into the conv

def fold_bn(w, bias, gamma, beta, running_mean, running_var, eps):
    """w [Cout, row] (row = Cin * 9 filter elements per output channel), the rest [Cout]; a = gamma / sqrt(running_var + eps)
    -> a[c] w[c][k],  a[c] (bias[c] - running_mean[c]) + beta[c]"""
    a = gamma / torch.sqrt(running_var + eps)
    return a[:, None] * w, a * (bias - running_mean) + beta


# ---------------------------------------------------------------------------------------------- Adam, torch.optim.Adam(eps=1e-7)

def adam_scalars(lr, beta1, beta2, t):
    """step size lr / (1 - beta1^t) and sqrt(1 - beta2^t) of step t (python floats = float64)"""
    return lr / (1.0 - beta1 ** t), (1.0 - beta2 ** t) ** 0.5


def adam_step(p, g, m, v, t, lr, beta1, beta2, eps, grad_scale=1.0, scalars=None):
    """one step (t counts from 1) on tensors of any shape; -> p', m', v'.  weight_decay 0, amsgrad off.
    scalars: (step size, sqrt(1 - beta2^t)) when the caller formed them (from betas it holds in another precision)."""
    g = g * grad_scale
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    step_size, bc2_sqrt = scalars if scalars is not None else adam_scalars(lr, beta1, beta2, t)
    return p - step_size * m / (v.sqrt() / bc2_sqrt + eps), m, v


def to_bucket_major(grad, bounds):
    """grad [G, U] -> flat [G * U]: bucket k = columns [bounds[k], bounds[k+1]) of every row, stored contiguously as [G, width_k],
    the buckets one behind the other (every data-parallel all-reduce then covers one contiguous range)"""
    return torch.cat([grad[:, lo:hi].reshape(-1) for lo, hi in zip(bounds[:-1], bounds[1:])])


def from_bucket_major(flat, G, bounds):
    """the inverse permutation: flat [G * U] -> [G, U]"""
    out, off = [], 0
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        out.append(flat[off:off + G * (hi - lo)].reshape(G, hi - lo))
        off += G * (hi - lo)
    return torch.cat(out, 1)


# ---------------------------------------------------------------------------------------------- adapters (exact)

def cube_gather(raw, flow, idx=None):
    """raw uint8 [N, T, HW, 3], flow float32 [N, Tf, HW, 2] (either may be None), idx [B] or None (= all, in order)
    -> x float32 [B, HW, 3T] = raw / 255 (one float32 division), xof float32 [B, HW, 2Tf]: frames become channel groups"""
    x = xof = None
    if raw is not None:
        r = raw if idx is None else raw[idx]
        x = (r.astype(np.float32) / np.float32(255)).transpose(0, 2, 1, 3).reshape(r.shape[0], r.shape[2], -1)
    if flow is not None:
        f = flow if idx is None else flow[idx]
        xof = f.transpose(0, 2, 1, 3).reshape(f.shape[0], f.shape[2], -1).copy()
    return x, xof


def cube_erase(cube, chmap):
    """cube [npix, Cc], chmap [G, CP] (source channel or -1) -> [G, npix, CP]: out[g, p, k] = cube[p, chmap[g, k]], 0 where -1"""
    out = cube[:, chmap.clamp_min(0)].permute(1, 0, 2)
    return out * (chmap >= 0).to(cube.dtype)[:, None, :]


def pool_act(y, a, b):
    """y [B, 2 H2, 2 W2, C] -> MaxPool2d(2)(relu(a y + b)) [B, H2, W2, C]"""
    B, H, W, C = y.shape
    return act_in(y, a, b).reshape(B, H // 2, 2, W // 2, 2, C).amax((2, 4))


def nchw_to_nhwc(src):
    """[B, C, HW] -> [B, HW, C]"""
    return src.permute(0, 2, 1).contiguous()


def out4_to_nchw(out4, dst, oc, choff):
    """out4 [B, HW, 4]; dst [B, Ctot, HW]: channels [choff, choff + oc) of dst take channels [0, oc) of out4, the rest stays"""
    dst = dst.clone()
    dst[:, choff:choff + oc] = out4[:, :, :oc].permute(0, 2, 1)
    return dst


def nchw_to_out4(src, oc, choff):
    """src [B, Ctot, HW] -> [B, HW, 4]: channels [choff, choff + oc) of src, zeros behind them"""
    out = src.new_zeros(src.shape[0], src.shape[2], 4)
    out[:, :, :oc] = src[:, choff:choff + oc].permute(0, 2, 1)
    return out
