#!/usr/bin/env python
"""Time test.py's test stage with ``[mi355x] pixel_maps`` off and on, on the synthetic UCSDped2-shaped tree of
``tools/synthetic_tree.py`` (240x360 frames), with ``pixel_criterion = True`` in every leg (the fine criterion needs it) and
``save_score_masks`` on (the stock value) or off.  The cube files are extracted once, outside the timed legs
(``test_foreground_saved = True`` afterwards); one child process per leg under its own time limit, one GPU process at a time, in the
same order on the same machine, and the first leg that exits abnormally ends the run.  Each ``test.main`` leg reports its wall time
and, inside it, the launch loop (``score_index_list``, synchronised: the forward with or without the reconstruction store and the
error-map pass), the pixel stage and in it the map kernels (``error_zmaps`` + ``paint_error_masks`` + ``mask_pixel_scores``,
synchronised) and ``torch.save``.  The ``launch`` leg times ``FusedTrainer.score_cubes`` alone on a seeded 5raw+5of bank at
``--batch`` cubes with HIP events, maps off and on (replayed captures, ``--iters`` launches each after a warm-up).  Prints one JSON
line; needs the GPU.

    timeout 1200 python tools/time_pixel_maps.py --frames 400 [--boxes 12] [--batch 2048] [--work DIR] [--out maps.json]
"""
import argparse
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

from synthetic_tree import make_tree, metered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = {'off': {'save_score_masks': True, 'pixel_maps': False}, 'maps': {'save_score_masks': True, 'pixel_maps': True},
        'off-nofiles': {'save_score_masks': False, 'pixel_maps': False}, 'maps-nofiles': {'save_score_masks': False, 'pixel_maps': True}}
LEG_LIMIT = 900          # seconds a leg may take


def leg(name):
    """One test.main run in this process with wall-clock meters; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import torch
    import test as S
    from vec_vad_amd import scoring
    sync = torch.cuda.synchronize
    meter = {'launches': 0.0, 'stage': 0.0, 'maps': 0.0, 'save': 0.0}
    S.score_index_list = metered(meter, S.score_index_list, 'launches', sync)
    S._pixel_stage = metered(meter, S._pixel_stage, 'stage', sync)
    torch.save = metered(meter, torch.save, 'save')
    for fn in ('error_zmaps', 'paint_error_masks', 'mask_pixel_scores'):
        setattr(scoring, fn, metered(meter, getattr(scoring, fn), 'maps', sync))
    sync()
    t0 = time.perf_counter()
    auc = S.main('config.cfg')
    sync()
    wall = time.perf_counter() - t0
    out = {'leg': name, 'wall_s': wall, 'launch_loop_s': meter['launches'], 'pixel_stage_s': meter['stage'],
           'map_kernels_s': meter['maps'], 'torch_save_s': meter['save'], 'auc': auc,
           'peak_device_gb': torch.cuda.max_memory_allocated() / 1e9}
    res = 'results/UCSDped2/'
    for key, d in (('masks', 'score_mask'), ('error_masks', 'error_mask')):
        if os.path.isdir(res + d):
            sha = hashlib.sha256()
            n = len(os.listdir(res + d))
            for f in range(n):
                sha.update(np.ascontiguousarray(torch.load(res + '%s/%d' % (d, f), weights_only=False)).tobytes())
            out[key], out[key + '_sha'] = n, sha.hexdigest()[:16]
    for key, p in (('frame_scores', 'frame_scores'), ('pixel_scores', 'pixel_scores'), ('pixel_scores_fine', 'pixel_scores_fine')):
        p = res + '%s_obj_det_with_motion_SelfComplete.npy' % p
        if os.path.exists(p):
            out[key + '_sha'] = hashlib.sha256(np.load(p).tobytes()).hexdigest()[:16]
    print(json.dumps(out))


def launch_leg(batch, iters):
    """``score_cubes`` at ``batch`` cubes, maps off and on: milliseconds per launch from HIP events around ``iters`` replays."""
    sys.path.insert(0, ROOT)
    import torch
    from model.unet import SelfCompleteNetFull
    from vec_vad_amd.trainer import FusedTrainer
    torch.manual_seed(0)
    net = SelfCompleteNetFull(features_root=32, tot_raw_num=5, tot_of_num=5, border_mode='predict', rawRange=None, useFlow=True,
                              padding=False).cuda().eval()
    tr = FusedTrainer(net)
    g = torch.Generator(device='cuda').manual_seed(1)
    raw = torch.randint(0, 256, (batch, 5, 32, 32, 3), dtype=torch.uint8, device='cuda', generator=g)
    flow = torch.randn((batch, 5, 32, 32, 2), device='cuda', generator=g)
    idx = torch.randperm(batch, device='cuda', generator=g)
    out = {'leg': 'launch', 'batch': batch, 'iters': iters, 'graph': bool(tr._graph_ok())}
    for maps in (False, True):
        for _ in range(3):               # eager, capture, one replay
            tr.score_cubes(raw, flow, idx, maps=maps)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            res = tr.score_cubes(raw, flow, idx, maps=maps)
        e1.record()
        torch.cuda.synchronize()
        out['maps_ms' if maps else 'plain_ms'] = e0.elapsed_time(e1) / iters
        del res
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == 'launch':
        return launch_leg(a.batch, a.iters)
    if a.leg:
        return leg(a.leg)
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='pixel_maps_tree_') if own else os.path.abspath(a.work)
    if not own:
        os.makedirs(work, exist_ok=False)
    out_path = os.path.abspath(a.out) if a.out else None
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes)
        stock = open(os.path.join(ROOT, 'config.cfg')).read().replace('epochs = 10', 'epochs = 1')
        for key in ('save_score_masks = True', 'pixel_maps = False', 'pixel_criterion = False'):
            assert key in stock, key
        open('config.cfg', 'w').write(stock.replace('save_score_masks = True', 'save_score_masks = False'))
        env = dict(os.environ, PYTHONPATH=ROOT)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        subprocess.run([sys.executable, os.path.join(ROOT, 'test.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=LEG_LIMIT)   # cube files
        cfg = stock.replace('test_foreground_saved = False', 'test_foreground_saved = True').replace(
            'pixel_criterion = False', 'pixel_criterion = True')
        from vec_vad_amd import build as B
        res = {'frames': a.frames, 'boxes_per_frame': a.boxes, 'library_hash': B.wanted()[1][:16], 'legs': []}
        me = [sys.executable, os.path.abspath(__file__)]
        runs = [('launch', me + ['--leg', 'launch', '--batch', str(a.batch), '--iters', str(a.iters)], None)]
        runs += [(name, me + ['--leg', name], keys) for name, keys in LEGS.items()]
        for name, cmd, keys in runs:
            if keys is not None:
                text = cfg
                for key, val in keys.items():
                    text = text.replace('%s = %s' % (key, not val), '%s = %s' % (key, val))
                open('config.cfg', 'w').write(text)
                shutil.rmtree('results', ignore_errors=True)
            # check=True: the first leg that exits abnormally (or runs into its time limit) ends the run; nothing is started behind it
            out = subprocess.run(cmd, check=True, env=env, stdout=subprocess.PIPE, timeout=LEG_LIMIT).stdout.decode()
            res['legs'].append(json.loads(out.strip().splitlines()[-1]))
        tm = [l for l in res['legs'] if l['leg'] != 'launch']
        for key in ('frame_scores_sha', 'pixel_scores_sha', 'masks_sha', 'error_masks_sha', 'pixel_scores_fine_sha'):
            res['same_' + key[:-4]] = len({l[key] for l in tm if key in l}) == 1
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
