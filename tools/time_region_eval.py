#!/usr/bin/env python
"""Time the region stage of test.py (``[mi355x] region_criterion = True``) per chunk of frames, on the synthetic UCSDped2-shaped tree
of ``tools/synthetic_tree.py`` (240x360 frames, ground truth on every second frame), split into labelling (``label_regions``), match
(``region_match``) and links (``region_links``), each call synchronised, next to two other times of the same run: the ``pixel_scores``
stage (``pixel_criterion = True`` in the same ``test.main``) and the numpy restatement of the region stage
(``tests/region_restatement.py``: flood fill, loops over boxes and regions) on the host, fed with the first chunk's ground truth,
cube scores and rectangles, whose results must equal the device's.  The cube files are extracted once, outside the timed run
(``test_foreground_saved = True`` afterwards); the timed ``test.main`` runs in a child process of its own, one GPU process at a
time.  Prints one JSON line; needs the GPU.

    timeout 900 python tools/time_region_eval.py --frames 400 [--boxes 12] [--chunk 64] [--work DIR] [--out regions.json]
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


def timed(times, fn, key, sync):
    """``fn`` with the synchronised wall time of every call appended to ``times[key]``."""
    def run(*a, **k):
        sync()
        t0 = time.perf_counter()
        out = fn(*a, **k)
        sync()
        times[key].append(time.perf_counter() - t0)
        return out
    return run


def leg(chunk):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch
    import test as S
    from vec_vad_amd import scoring
    import region_restatement as R
    sync = torch.cuda.synchronize
    times = {k: [] for k in ('label', 'match', 'links', 'stage', 'pixel', 'merge')}
    scoring.label_regions = timed(times, scoring.label_regions, 'label', sync)
    scoring.region_match = timed(times, scoring.region_match, 'match', sync)
    scoring.region_links = timed(times, scoring.region_links, 'links', sync)
    scoring.pixel_scores = timed(times, scoring.pixel_scores, 'pixel', sync)
    scoring.merge_groups = timed(times, scoring.merge_groups, 'merge', sync)
    first = {}
    stage = S.PixelEval.region_stage

    def keep_first(self, gt, off, scores, rects, a, b):
        if not first:
            first.update(gt=gt.cpu().numpy(), off=np.array(off), scores=scores.cpu().numpy(), rects=rects.cpu().numpy(), frames=b - a)
        return stage(self, gt, off, scores, rects, a, b)

    S.PixelEval.region_stage = timed(times, keep_first, 'stage', sync)
    sync()
    t0 = time.perf_counter()
    S.main('config.cfg')
    sync()
    wall = time.perf_counter() - t0
    # the same stage of the first chunk on the host, and its results against the device's
    t0 = time.perf_counter()
    labels, n_reg = R.label_frames(first['gt'])
    t_label = time.perf_counter() - t0
    t0 = time.perf_counter()
    w_area, w_best, w_state = R.match(labels, first['scores'], first['off'], first['rects'], 10)
    t_match = time.perf_counter() - t0
    t0 = time.perf_counter()
    w_links = R.links(labels, None, np.concatenate([[0], np.ones(len(labels) - 1)]))
    t_links = time.perf_counter() - t0
    d_labels, d_n = scoring.label_regions(first['gt'])
    d_area, d_best, d_state = scoring.region_match(d_labels, torch.from_numpy(first['scores']).cuda(), first['off'], first['rects'], 10)
    d_links = scoring.region_links(d_labels, None, np.concatenate([[0], np.ones(len(labels) - 1)]))
    same = bool(np.array_equal(d_labels.cpu().numpy(), labels) and np.array_equal(d_n.cpu().numpy(), n_reg)
                and np.array_equal(d_area.cpu().numpy(), w_area) and np.array_equal(d_best.cpu().numpy(), w_best)
                and np.array_equal(d_state.cpu().numpy(), w_state) and np.array_equal(d_links.cpu().numpy().view(np.uint64), w_links))
    curves = dict(np.load('results/UCSDped2/raw2flow_obj_det_with_motion_SelfComplete_region_results.npz'))

    def ms(key):
        """First (cold) call and the median of the later calls that cover a whole chunk, in milliseconds."""
        full = times[key][1:len(times['stage']) - 1] or times[key][1:] or times[key]
        return {'first_ms': 1e3 * times[key][0], 'median_ms': 1e3 * float(np.median(full)), 'calls': len(times[key])}

    print(json.dumps({'wall_s': wall, 'chunk_frames': chunk, 'chunks': len(times['stage']), 'boxes_first_chunk': int(len(first['scores'])),
                      'regions_first_chunk': int(n_reg.sum()), 'label': ms('label'), 'match': ms('match'), 'links': ms('links'),
                      'region_stage': ms('stage'), 'pixel_scores': ms('pixel'), 'merge_groups': ms('merge'),
                      'host_restatement_first_chunk_ms': {'label': 1e3 * t_label, 'match': 1e3 * t_match, 'links': 1e3 * t_links},
                      'restatement_equals_device': same, 'rbdc': float(curves['rbdc']), 'tbdc': float(curves['tbdc'])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.chunk)
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='region_eval_tree_') if own else os.path.abspath(a.work)
    if not own:
        os.makedirs(work, exist_ok=False)
    out_path = os.path.abspath(a.out) if a.out else None
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes)
        stock = open(os.path.join(ROOT, 'config.cfg')).read().replace('epochs = 10', 'epochs = 1')
        for key in ('save_score_masks = True', 'pixel_criterion = False', 'region_criterion = False', 'direct_frames_per_chunk = 64'):
            assert key in stock, key
        stock = stock.replace('save_score_masks = True', 'save_score_masks = False')
        open('config.cfg', 'w').write(stock)
        env = dict(os.environ, PYTHONPATH=ROOT)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        subprocess.run([sys.executable, os.path.join(ROOT, 'test.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)   # cube files
        open('config.cfg', 'w').write(stock.replace('test_foreground_saved = False', 'test_foreground_saved = True')
                                      .replace('pixel_criterion = False', 'pixel_criterion = True')
                                      .replace('region_criterion = False', 'region_criterion = True')
                                      .replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = %d' % a.chunk))
        shutil.rmtree('results', ignore_errors=True)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', '--chunk', str(a.chunk)], check=True, env=env,
                             stdout=subprocess.PIPE, timeout=900).stdout.decode()
        from vec_vad_amd import build as B
        res = dict(frames=a.frames, boxes_per_frame=a.boxes, library_hash=B.wanted()[1][:16], **json.loads(out.strip().splitlines()[-1]))
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
