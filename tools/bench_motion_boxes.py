#!/usr/bin/env python
"""Time the motion foreground stage (vec_vad_amd/motion.py) on the GPU: microseconds per frame for the three frame sizes at
16 windows per launch, split into upload (H2D copy of the chunk's frames), mask kernel (``vv_motion_mask``) and box kernels
(``vv_mask_boxes``, five launches).  Device events around repeated launches after a warm-up; the numpy restatement's time per
frame on the same host is printed next to it as orientation only.  Prints one JSON line; needs the GPU (no fallback).

    timeout 300 python tools/bench_motion_boxes.py [--reps 50] [--warmup 5] [--out motion_boxes.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from vec_vad_amd.motion import CONSTANTS, mask_boxes, motion_mask  # noqa: E402

SIZES = (('UCSDped2', 240, 360), ('avenue', 360, 640), ('ShanghaiTech', 480, 856))


def scene(rng, F, H, W):
    """a static texture with sensor noise and rectangles that move a few pixels per frame (3-channel, like decoded frames)"""
    base = rng.integers(20, 60, (H, W, 1)).repeat(3, axis=2)
    fr = np.empty((F, H, W, 3), np.uint8)
    rects = [(rng.integers(0, H - 40), rng.integers(0, W - 60), rng.integers(8, 40), rng.integers(8, 60), rng.integers(-7, 8),
              rng.integers(-7, 8), rng.integers(100, 256, 3)) for _ in range(12)]
    for t in range(F):
        img = base + rng.integers(0, 15, (H, W, 3))
        for (y, x, h, w, vy, vx, col) in rects:
            yy, xx = int(np.clip(y + vy * t, 0, H - 1)), int(np.clip(x + vx * t, 0, W - 1))
            img[yy:yy + h, xx:xx + w] = col
        fr[t] = np.clip(img, 0, 255)
    return fr


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--windows', type=int, default=16)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-restatement', action='store_true')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_motion_boxes.py measures on the GPU; there is no fallback'
    N = a.windows
    rng = np.random.default_rng(0)
    res = {'windows_per_launch': N, 'reps': a.reps, 'device': torch.cuda.get_device_name(0), 'sizes': {}}
    for name, H, W in SIZES:
        k = CONSTANTS[name]
        host = scene(rng, N + 2, H, W)                                 # N consecutive frames + one neighbour on each side
        pinned = torch.from_numpy(host).pin_memory()
        win = [[i, i + 1, i + 2] for i in range(N)]
        dev = pinned.cuda()
        mask = motion_mask(dev, win, k['ksize'], k['binary_thr'], None, k['extend'])
        count, _ = mask_boxes(mask, k['area_thr'], k['extend'])
        t_up = timed(lambda: pinned.to('cuda', non_blocking=True), a.reps, a.warmup)
        t_mask = timed(lambda: motion_mask(dev, win, k['ksize'], k['binary_thr'], None, k['extend']), a.reps, a.warmup)
        t_box = timed(lambda: mask_boxes(mask, k['area_thr'], k['extend']), a.reps, a.warmup)
        r = {'frame': [H, W, 3], 'ksize': k['ksize'], 'boxes_per_frame': float(count.float().mean()),
             'mask_set_fraction': float((mask != 0).float().mean()),
             'upload_us_per_frame': t_up / N, 'mask_kernel_us_per_frame': t_mask / N, 'box_kernels_us_per_frame': t_box / N,
             'note': 'mask / box figures include the wrapper (index upload, workspace allocation, the count readback)'}
        if not a.no_restatement:
            import motion_boxes_restatement as MR
            t0 = time.perf_counter()
            for i in range(2):
                MR.get_mt_bboxes(host[win[i]], np.zeros((0, 4)), name)
            r['numpy_restatement_us_per_frame'] = (time.perf_counter() - t0) * 1e6 / 2
        res['sizes'][name] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
