#!/usr/bin/env python
"""Time test.py's test stage with ``[mi355x] save_score_masks = True`` (the stock value): the host painter (``_save_masks``: a numpy
loop over boxes per frame) against ``device_score_masks = True`` (``vv_paint_masks``, one copy to the host per chunk of frames) and
against ``pixel_criterion = True``, on the synthetic UCSDped2-shaped tree of ``tools/time_direct_test.py`` (240x360 frames).  The cube
files are extracted once, outside the timed legs (``test_foreground_saved = True`` afterwards); one child process per leg, one GPU
process at a time, in the same order on the same machine.  Each leg reports the wall time of ``test.main`` and, inside it, the mask
stage split into painting (``paint_frame`` calls | ``paint_masks`` launches, synchronised), ``torch.save`` and the rest of the stage
(device-to-host copy of the chunk, background fill, per-frame copies), plus the pixel stage (ground-truth reading, ``merge_groups`` +
``pixel_scores``).  ``--parent-root DIR`` adds a first leg that runs the host painter of another checkout (built, e.g. the parent
commit) on the same tree.  Prints one JSON line; needs the GPU.

    timeout 900 python tools/time_score_masks.py --frames 400 [--boxes 12] [--parent-root DIR] [--work DIR] [--out masks.json]
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
LEGS = {'host': {}, 'device': {'device_score_masks': True}, 'pixel': {'pixel_criterion': True},
        'device+pixel': {'device_score_masks': True, 'pixel_criterion': True}}


def leg(name, root):
    """One test.main run in this process (the checkout at ``root``) with wall-clock meters; prints one JSON line."""
    sys.path.insert(0, root)
    import torch
    import test as S
    from vec_vad_amd import scoring
    sync = torch.cuda.synchronize
    meter = {'stage': 0.0, 'paint': 0.0, 'save': 0.0, 'gt_read': 0.0, 'pixel': 0.0}
    S._save_masks = metered(meter, S._save_masks, 'stage', sync)
    S.paint_frame = metered(meter, S.paint_frame, 'paint')
    torch.save = metered(meter, torch.save, 'save')
    if hasattr(S, '_pixel_stage'):
        S._pixel_stage = metered(meter, S._pixel_stage, 'stage', sync)
        scoring.paint_masks = metered(meter, scoring.paint_masks, 'paint', sync)
        scoring.merge_groups = metered(meter, scoring.merge_groups, 'pixel', sync)
        scoring.pixel_scores = metered(meter, scoring.pixel_scores, 'pixel', sync)
        import foreground as FG
        real = FG.gt_source

        class Timed:
            def __init__(self, src):
                self.src, self.read = src, metered(meter, src, 'gt_read')

            def __len__(self):
                return len(self.src)

            def __call__(self, i):
                return self.read(i)

        def gt_source(c):
            return Timed(real(c))

        FG.gt_source = gt_source
    sync()
    t0 = time.perf_counter()
    auc = S.main('config.cfg')
    sync()
    wall = time.perf_counter() - t0
    sha = hashlib.sha256()
    n = len(os.listdir('results/UCSDped2/score_mask'))
    for f in range(n):
        sha.update(np.ascontiguousarray(torch.load('results/UCSDped2/score_mask/%d' % f, weights_only=False)).tobytes())
    out = {'leg': name, 'wall_s': wall, 'mask_stage_s': meter['stage'] - meter['gt_read'] - meter['pixel'], 'paint_s': meter['paint'],
           'torch_save_s': meter['save'], 'copy_and_rest_s': meter['stage'] - meter['paint'] - meter['save'] - meter['gt_read'] - meter['pixel'],
           'gt_read_s': meter['gt_read'], 'pixel_scores_s': meter['pixel'], 'auc': auc, 'masks': n, 'masks_sha': sha.hexdigest()[:16]}
    p = 'results/UCSDped2/pixel_scores_obj_det_with_motion_SelfComplete.npy'
    if os.path.exists(p):
        out['pixel_scores_sha'] = hashlib.sha256(np.load(p).tobytes()).hexdigest()[:16]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--parent-root', default=None)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--root', default=ROOT, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg, a.root)
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='score_mask_tree_') if own else os.path.abspath(a.work)
    if not own:
        os.makedirs(work, exist_ok=False)
    out_path = os.path.abspath(a.out) if a.out else None
    parent = os.path.abspath(a.parent_root) if a.parent_root else None
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes)
        stock = open(os.path.join(ROOT, 'config.cfg')).read().replace('epochs = 10', 'epochs = 1')
        assert 'save_score_masks = True' in stock
        open('config.cfg', 'w').write(stock.replace('save_score_masks = True', 'save_score_masks = False'))
        env = dict(os.environ, PYTHONPATH=ROOT)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        subprocess.run([sys.executable, os.path.join(ROOT, 'test.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)   # cube files
        cfg = stock.replace('test_foreground_saved = False', 'test_foreground_saved = True')
        from vec_vad_amd import build as B
        res = {'frames': a.frames, 'boxes_per_frame': a.boxes, 'library_hash': B.wanted()[1][:16], 'legs': []}
        runs = ([('parent-host', parent, {})] if parent else []) + [(name, ROOT, keys) for name, keys in LEGS.items()]
        for name, root, keys in runs:
            text = cfg
            for key in keys:
                text = text.replace('%s = False' % key, '%s = True' % key)
            open('config.cfg', 'w').write(text)
            shutil.rmtree('results', ignore_errors=True)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, '--root', root], check=True,
                                 env=dict(os.environ, PYTHONPATH=root), stdout=subprocess.PIPE, timeout=900).stdout.decode()
            res['legs'].append(json.loads(out.strip().splitlines()[-1]))
        res['same_masks'] = len({l['masks_sha'] for l in res['legs']}) == 1
        res['same_pixel_scores'] = len({l['pixel_scores_sha'] for l in res['legs'] if 'pixel_scores_sha' in l}) == 1
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
