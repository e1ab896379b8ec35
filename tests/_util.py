"""Shared helpers for the parity tests."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def digest(t, k=8):
    """Same digest as tests/golden/make_goldens.py: [sum, sum|x|, sum x^2, cos-weighted sum, k strided samples]."""
    a = torch.as_tensor(t).detach().double().reshape(-1).cpu()
    idx = torch.linspace(0, a.numel() - 1, k).long()
    w = torch.cos(torch.arange(a.numel(), dtype=torch.float64) * 0.37)
    return np.concatenate([[a.sum().item(), a.abs().sum().item(), (a * a).sum().item(), (a * w).sum().item()],
                           a[idx].numpy()])


def small_config(test_block_mode=True):
    """The stock config.cfg shrunk for the script-level tests, written to ./config.cfg and returned: one epoch, batches of 4, and
    for UCSDped2 a 2x2 block grid with ``train_block_mode = 9`` (and ``test_block_mode = 9`` unless told otherwise)."""
    cfg = open(os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), 'config.cfg')).read()
    cfg = cfg.replace('epochs = 10', 'epochs = 1').replace('batch_size = 128', 'batch_size = 4')
    cfg = cfg.replace('[UCSDped2]\n', '[UCSDped2]\nh_block = 2\nw_block = 2\ntrain_block_mode = 9\n'
                      + ('test_block_mode = 9\n' if test_block_mode else ''))      # dataset-level overrides
    open('config.cfg', 'w').write(cfg)
    return cfg


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))


def digest_close(d, g, rtol, atol_scale=1.0):
    """Compare digests: entries 0..3 are sums (tolerance relative to sum|x| / sqrt(sum x^2)), 4.. are samples."""
    d, g = np.asarray(d, dtype=np.float64), np.asarray(g, dtype=np.float64)
    scale_abs = max(g[1], 1e-30)
    ok = abs(d[0] - g[0]) <= rtol * scale_abs * atol_scale
    ok &= abs(d[1] - g[1]) <= rtol * scale_abs
    ok &= abs(d[2] - g[2]) <= 2 * rtol * max(g[2], 1e-30)
    ok &= abs(d[3] - g[3]) <= rtol * scale_abs * atol_scale
    n = max(1.0, float(len(g) - 4))
    rms = np.sqrt(max(g[2], 0.0)) if g[2] > 0 else 0.0
    samp_tol = rtol * (np.abs(g[4:]) + np.abs(g[4:]).max() + 1e-30)
    ok &= bool(np.all(np.abs(d[4:] - g[4:]) <= samp_tol * 4))
    return bool(ok)


def observe(name, **vals):
    """Observed deviations of a parity check: printed (pytest -s / -rP) and appended to gpurun_out/observed.jsonl so that the bars
    in the tests can be set from measurements (bars at ~2x the observed value)."""
    import json
    import os
    rec = dict(test=name, **{k: float(v) for k, v in vals.items()})
    print('OBSERVED', json.dumps(rec))
    try:
        root = os.environ.get('GRAFT_REPO_ROOT') or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        os.makedirs(os.path.join(root, 'gpurun_out'), exist_ok=True)
        with open(os.path.join(root, 'gpurun_out', 'observed.jsonl'), 'a') as f:
            f.write(json.dumps(rec) + '\n')
    except OSError:
        pass


# ---- kernel-level parity against a float64 restatement (tests/test_gpu_train_ops.py, tests/test_gpu_outconv.py) ----
FLOOR = 16 * 2.0 ** -23      # floor of the float-summation bar
SENT = 3.0                   # sentinel behind and beside every output


def gen(*key):
    return torch.Generator(device='cpu').manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def err(got, ref):
    ref = ref.double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def bar(op, what, got, ref64, ref32, family='train_ops'):
    """the float-summation bar: err_hip of the kernel against err_ref32 of the SAME restatement evaluated in float32 on the same inputs,
    err_hip <= max(8 err_ref32, 16 * 2^-23); prints / records the figures before it asserts"""
    e_hip, e_32 = err(got, ref64), err(ref32, ref64)
    observe(family + ':' + op, err_hip=e_hip, err_ref32=e_32)
    assert e_hip <= max(8 * e_32, FLOOR), (op, what, e_hip, e_32)


def away_from_zero(y, a, b, margin=1e-3):
    """y [.., C] float32 nudged so that no |a y + b| (float64 of the float32 values) is below the margin"""
    z = a.double() * y.double() + b.double()
    bad = z.abs() < 4 * margin
    tgt = torch.where(z >= 0, 8 * margin, -8 * margin)
    y = torch.where(bad, ((tgt - b.double()) / a.double()).float(), y)
    assert (a.double() * y.double() + b.double()).abs().min().item() >= margin
    return y
