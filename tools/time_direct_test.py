#!/usr/bin/env python
"""Time test.py's test stage from ``test.main`` entry to the saved frame scores, staged (cube files through the host) against
``[mi355x] direct_test = True``, on a synthetic UCSDped2-shaped tree (240x360 grey .tif frames, [h,w,2] flow .npy, random boxes
of which those in a still corner fail the motion test).  One child process per leg, staged first, in the same order on the same
machine; each leg reports its wall time split into decode (time inside ``get_inputs``: image decoding and flow loading, every call),
extraction (the rest of ``extract_test`` / of the ``extract_device`` generator, file writing included), cube loading (``np.load``
of the ``foreground_*`` files, staged leg only), scoring (the rest: model loading, engines, launches, evaluation, masks off) and its
peak host RSS.  Prints one JSON line; needs the GPU.  The tree is built in a fresh temporary directory that is removed at the end,
or in ``--work`` (which must not exist yet and is kept).

    timeout 900 python tools/time_direct_test.py --frames 400 [--boxes 12] [--work DIR] [--out direct_test.json]
"""
import argparse
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

from synthetic_tree import make_tree, metered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leg(direct):
    """One test.main run in this process with wall-clock meters around the three stages; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import torch
    import foreground as FG
    import vad_datasets as V
    import test as S
    meter = {'decode': 0.0, 'extract': 0.0, 'cube_load': 0.0}
    V.get_inputs = FG.get_inputs = metered(meter, V.get_inputs, 'decode')
    FG.extract_test = metered(meter, FG.extract_test, 'extract')
    real_device = FG.extract_device

    def extract_device(*a, **k):
        t0 = time.perf_counter()
        info, parts = real_device(*a, **k)
        meter['extract'] += time.perf_counter() - t0

        def timed_parts():
            while True:
                t1 = time.perf_counter()
                try:
                    p = next(parts)
                except StopIteration:
                    return
                finally:
                    torch.cuda.synchronize()
                    meter['extract'] += time.perf_counter() - t1
                yield p
        return info, timed_parts()

    FG.extract_device = extract_device
    np_load, timed_load = np.load, metered(meter, np.load, 'cube_load')
    np.load = lambda f, *a, **k: (timed_load if 'foreground_' in os.path.basename(str(f)) else np_load)(f, *a, **k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    auc = S.main('config.cfg')
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    fs = np.load('results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy')
    print(json.dumps({'direct': bool(direct), 'wall_s': wall, 'decode_s': meter['decode'], 'extract_s': meter['extract'] - meter['decode'],
                      'cube_load_s': meter['cube_load'], 'score_s': wall - meter['extract'] - meter['cube_load'],
                      'peak_rss_mb': resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 'auc': auc, 'scores_sha': __import__('hashlib').sha256(fs.tobytes()).hexdigest()[:16]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == 'direct')
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='direct_test_tree_') if own else os.path.abspath(a.work)
    if not own:
        os.makedirs(work, exist_ok=False)
    out_path = os.path.abspath(a.out) if a.out else None
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes)
        cfg = open(os.path.join(ROOT, 'config.cfg')).read()
        cfg = cfg.replace('epochs = 10', 'epochs = 1').replace('save_score_masks = True', 'save_score_masks = False')
        open('config.cfg', 'w').write(cfg)
        env = dict(os.environ, PYTHONPATH=ROOT)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        from vec_vad_amd import build as B
        res = {'frames': a.frames, 'boxes_per_frame': a.boxes, 'library_hash': B.wanted()[1][:16], 'legs': []}
        for name in ('staged', 'direct'):
            open('config.cfg', 'w').write(cfg.replace('direct_test = False', 'direct_test = %s' % (name == 'direct')))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name], check=True, env=env, stdout=subprocess.PIPE,
                                 timeout=900).stdout.decode()
            res['legs'].append(json.loads(out.strip().splitlines()[-1]))
        res['same_scores'] = res['legs'][0]['scores_sha'] == res['legs'][1]['scores_sha']
        cube_files = [f for f in os.listdir(os.path.join('data', 'raw2flow')) if 'foreground_test' in f or 'foreground_bbox_test' in f]
        res['staged_cube_file_mb'] = sum(os.path.getsize(os.path.join('data', 'raw2flow', f)) for f in cube_files) / 1e6
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
