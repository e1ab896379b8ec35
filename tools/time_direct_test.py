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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_tree(n_test, boxes_per_frame, seed=11):
    """raw_datasets/ + optical_flow/ + bbox files like UCSDped2: two short training videos and one test video of n_test frames."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = 240, 360
    for mode, sub, counts in (('train', 'Train', (6, 6)), ('test', 'Test', (n_test,))):
        all_boxes = []
        for v, n in enumerate(counts, start=1):
            name = '%s%03d' % (sub, v)
            os.makedirs(os.path.join('raw_datasets', 'UCSDped2', sub, name))
            os.makedirs(os.path.join('optical_flow', 'UCSDped2', sub, name))
            if mode == 'test':
                os.makedirs(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt'))
            for k in range(n):
                g = rng.integers(0, 256, (H, W), dtype=np.uint8)
                fl = (rng.standard_normal((H, W, 2)) * 2).astype(np.float32)
                fl[:60, :90] = 0                                   # a still corner: boxes there fail the motion test
                Image.fromarray(g).save(os.path.join('raw_datasets', 'UCSDped2', sub, name, '%04d.tif' % (k + 1)))
                np.save(os.path.join('optical_flow', 'UCSDped2', sub, name, '%04d.npy' % (k + 1)), fl)
                if mode == 'test':
                    gt = np.zeros((H, W), np.uint8)
                    if k % 2:
                        gt[100:120, 100:130] = 255
                    Image.fromarray(gt).save(os.path.join('raw_datasets', 'UCSDped2', sub, name + '_gt', '%04d.bmp' % (k + 1)))
                bb = []
                for m in range(boxes_per_frame):
                    x0, y0 = rng.uniform(95, W - 70), rng.uniform(65, H - 70)
                    bb.append([x0, y0, x0 + rng.uniform(8, 64), y0 + rng.uniform(8, 64), rng.random()])
                bb[0] = [5.0, 4.0, 40.0, 50.0, 0.9]                # inside the still corner -> dropped
                all_boxes.append(np.array(bb).reshape(-1, 5))
        arr = np.empty(len(all_boxes), dtype=object)
        for i, b in enumerate(all_boxes):
            arr[i] = b
        np.save(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_%s_obj_det_with_motion.npy' % mode), arr, allow_pickle=True)


def leg(direct):
    """One test.main run in this process with wall-clock meters around the three stages; prints one JSON line."""
    sys.path.insert(0, ROOT)
    import torch
    import foreground as FG
    import vad_datasets as V
    import test as S
    meter = {'decode': 0.0, 'extract': 0.0, 'cube_load': 0.0}

    def metered(fn, key):
        def run(*a, **k):
            t0 = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                meter[key] += time.perf_counter() - t0
        return run

    decode = metered(V.get_inputs, 'decode')
    V.get_inputs = FG.get_inputs = decode
    FG.extract_test = metered(FG.extract_test, 'extract')
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
    np_load, timed_load = np.load, metered(np.load, 'cube_load')
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
        make_tree(a.frames, a.boxes)
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
