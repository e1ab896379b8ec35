#!/usr/bin/env python
"""Time the smoothing of score masks (``[mi355x] smooth_masks = True``): the filter of one chunk on the device next to its numpy
restatement (``tests/smooth_restatement.py``) on the host, and ``test.main`` with the key off and on.

  chunk leg: a 240x360 volume of ``--chunk`` frames plus the temporal halo (64 + 2 * 2 = 68 frames at the default windows), random boxes
    of normal-distributed scores on every frame, two videos.  ``scoring.smooth_masks`` (allocation of the work buffer included) and the
    bare ``vv_smooth_masks`` call on a work buffer kept between calls are timed with device events after a warm-up; the restatement runs
    once on the host and its result must equal the device's, bit for bit.
  main legs: the synthetic UCSDped2-shaped tree of ``tools/synthetic_tree.py``; the cube files are extracted once, outside the timed
    runs (``test_foreground_saved = True`` afterwards), then ``test.main`` is timed with the key off and on (``save_score_masks`` off in
    both, so the difference is the stage itself and the kept groups, not the files).

Every GPU step runs in a child process of its own under its own time limit, one GPU process at a time.  Prints one JSON line; needs
the GPU.

    timeout 1500 python tools/time_smooth_masks.py --frames 400 [--boxes 12] [--chunk 64] [--reps 500] [--work DIR] [--out smooth.json]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

from synthetic_tree import make_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 240, 360


def chunk_leg(chunk, kt, ks, reps):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch
    from vec_vad_amd import scoring, _lib
    import smooth_restatement as R
    rt = kt // 2
    F = chunk + 2 * rt
    rng = np.random.default_rng(3)
    host = np.full((F, H, W), -100000.0)
    for f in range(F):
        for _ in range(12):
            y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            y1, x1 = min(H, y0 + int(rng.integers(8, 65))), min(W, x0 + int(rng.integers(8, 65)))
            host[f, y0:y1, x0:x1] = np.maximum(host[f, y0:y1, x0:x1], rng.standard_normal())
    vid = np.repeat([1, 2], [F // 2, F - F // 2]).astype(np.int32)
    masks = torch.from_numpy(host).cuda()

    def events(fn):
        """Milliseconds of every one of ``reps`` calls of ``fn`` after two warm-up calls, by device events."""
        fn()
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return out

    wrapper = events(lambda: scoring.smooth_masks(masks, vid, kt, ks, lo=rt, hi=rt + chunk))
    l = _lib.lib()
    work = torch.empty(int(l.vv_smooth_masks_work(F, H, W, kt, ks)), dtype=torch.uint8, device='cuda')
    out = torch.empty((chunk, H, W), dtype=torch.float64, device='cuda')
    fmax = torch.empty(chunk, dtype=torch.float64, device='cuda')
    vid_d = torch.from_numpy(vid).cuda()
    st = torch.cuda.current_stream().cuda_stream

    def bare_call():
        _lib.check(l.vv_smooth_masks(masks.data_ptr(), vid_d.data_ptr(), F, H, W, rt, rt + chunk, kt, ks, out.data_ptr(), fmax.data_ptr(),
                                     work.data_ptr(), st), 'vv_smooth_masks')

    bare = events(bare_call)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):              # one window over all calls: the per-call figure without an event pair around each
        bare_call()
    b.record()
    b.synchronize()
    back_to_back = a.elapsed_time(b) / reps
    t0 = time.perf_counter()
    want, want_max = R.smooth(host, vid, kt, ks)
    t_host = time.perf_counter() - t0
    same = bool(np.array_equal(out.cpu().numpy(), want[rt:rt + chunk]) and np.array_equal(fmax.cpu().numpy(), want_max[rt:rt + chunk]))
    painted = int((host[rt:rt + chunk] != -100000.0).sum())
    print(json.dumps({'buffer_frames': F, 'chunk_frames': chunk, 'smooth_frames': kt, 'smooth_pixels': ks, 'reps': reps,
                      'painted_fraction': painted / float(chunk * H * W), 'work_bytes': int(work.numel()),
                      'smooth_masks_ms': {'median': float(np.median(wrapper)), 'min': float(min(wrapper)), 'max': float(max(wrapper))},
                      'vv_smooth_masks_ms': {'median': float(np.median(bare)), 'min': float(min(bare)), 'max': float(max(bare))},
                      'vv_smooth_masks_back_to_back_ms': back_to_back,
                      'host_restatement_ms': 1e3 * t_host, 'restatement_equals_device': same}))


def main_leg():
    sys.path.insert(0, ROOT)
    import torch
    import test as S
    from vec_vad_amd import scoring
    sync = torch.cuda.synchronize
    times = {k: [] for k in ('stage', 'paint', 'smooth')}

    def timed(fn, key):
        """``fn`` with the synchronised wall time of every call appended to ``times[key]``."""
        def run(*a, **k):
            sync()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            sync()
            times[key].append(time.perf_counter() - t0)
            return out
        return run

    stage = S._smooth_stage

    def in_stage(*a, **k):      # paint_masks also serves device_score_masks: only the calls of the stage are counted
        keep = scoring.paint_masks, scoring.smooth_masks
        scoring.paint_masks, scoring.smooth_masks = timed(keep[0], 'paint'), timed(keep[1], 'smooth')
        try:
            return stage(*a, **k)
        finally:
            scoring.paint_masks, scoring.smooth_masks = keep

    S._smooth_stage = timed(in_stage, 'stage')
    sync()
    t0 = time.perf_counter()
    S.main('config.cfg')
    sync()
    res = {'wall_s': time.perf_counter() - t0}
    if times['stage']:
        sm = times['smooth']
        whole = sm[1:-1] or sm[1:] or sm        # the first call is cold, the last chunk may be short
        res.update(stage_ms=1e3 * times['stage'][0], chunks=len(sm), paint_calls=len(times['paint']), paint_ms_total=1e3 * sum(times['paint']),
                   smooth_first_ms=1e3 * sm[0], smooth_median_ms=1e3 * float(np.median(whole)), smooth_ms_total=1e3 * sum(sm))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--reps', type=int, default=500)
    ap.add_argument('--smooth-frames', type=int, default=5)
    ap.add_argument('--smooth-pixels', type=int, default=9)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', choices=('chunk', 'main'), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == 'chunk':
        return chunk_leg(a.chunk, a.smooth_frames, a.smooth_pixels, a.reps)
    if a.leg == 'main':
        return main_leg()
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='smooth_masks_tree_') if own else os.path.abspath(a.work)
    if not own:
        os.makedirs(work, exist_ok=False)
    out_path = os.path.abspath(a.out) if a.out else None
    os.chdir(work)
    env = dict(os.environ, PYTHONPATH=ROOT)
    me = [sys.executable, os.path.abspath(__file__)]

    def child(args, limit):
        print('running', ' '.join(args[1:]), file=sys.stderr, flush=True)
        out = subprocess.run(args, check=True, env=env, stdout=subprocess.PIPE, timeout=limit).stdout.decode()
        return json.loads(out.strip().splitlines()[-1])

    try:
        res = dict(frames=a.frames, boxes_per_frame=a.boxes)
        res['chunk'] = child(me + ['--leg', 'chunk', '--chunk', str(a.chunk), '--reps', str(a.reps), '--smooth-frames', str(a.smooth_frames),
                                   '--smooth-pixels', str(a.smooth_pixels)], 300)
        make_tree({'train': (6, 6), 'test': (a.frames // 2, a.frames - a.frames // 2)}, a.boxes)
        stock = open(os.path.join(ROOT, 'config.cfg')).read().replace('epochs = 10', 'epochs = 1')
        for key in ('save_score_masks = True', 'smooth_masks = False', 'smooth_frames = 5', 'smooth_pixels = 9', 'direct_frames_per_chunk = 64'):
            assert key in stock, key
        stock = (stock.replace('save_score_masks = True', 'save_score_masks = False')
                 .replace('smooth_frames = 5', 'smooth_frames = %d' % a.smooth_frames)
                 .replace('smooth_pixels = 9', 'smooth_pixels = %d' % a.smooth_pixels)
                 .replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = %d' % a.chunk))
        open('config.cfg', 'w').write(stock)
        print('training and extracting the cube files', file=sys.stderr, flush=True)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        subprocess.run([sys.executable, os.path.join(ROOT, 'test.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)   # cube files
        saved = stock.replace('test_foreground_saved = False', 'test_foreground_saved = True')
        for tag, text in (('off', saved), ('on', saved.replace('smooth_masks = False', 'smooth_masks = True'))):
            shutil.rmtree('results', ignore_errors=True)
            open('config.cfg', 'w').write(text)
            res['main_' + tag] = child(me + ['--leg', 'main'], 900)
        res['smooth_frame_scores_written'] = os.path.exists('results/UCSDped2/frame_scores_smooth_obj_det_with_motion_SelfComplete.npy')
        from vec_vad_amd import build as B
        res['library_hash'] = B.wanted()[1][:16]
        line = json.dumps(res)
        print(line)
        if out_path:
            with open(out_path, 'w') as f:
                f.write(line + '\n')
    finally:
        os.chdir(ROOT)
        if own:
            shutil.rmtree(work)


if __name__ == '__main__':
    main()
