#!/usr/bin/env python
"""Time the training stage with flow and cubes staged through files against ``[mi355x] direct_train = True`` + ``direct_flow = True``, on
a synthetic UCSDped2-shaped training split built like the tree of ``tools/synthetic_tree.py`` (240x360 grey .tif frames, random boxes
of which the first of every frame lies in a corner; here two training videos of ``--frames / 2`` frames each, no test split).  FlowNet2 carries seeded random weights
(``torch.manual_seed(0)``): its run time does not depend on them.  One child process per leg, each under its own time limit, A first,
on the same machine; the tool ends at the first child that does not exit normally:

  A  ``calc_optical_flow`` on the training split, ``pairs_per_launch=4`` (writes ``optical_flow/UCSDped2/Train...``), then ``train.main``
     with ``train_foreground_saved = False``: ``extract_train`` cuts the cubes frame by frame and writes ``foreground_train_*``,
     ``train.main`` loads those files and uploads them;
  B  no ``optical_flow/UCSDped2/Train`` and no ``foreground_train_*`` on disk, ``train.main`` with ``direct_train = True``,
     ``direct_flow = True`` (``direct_flow_pairs = 4``).

Each leg reports its wall time split into the flow stage (leg A), extraction (``extract_train`` / ``extract_train_device``, time inside
``get_inputs`` included) and training (the rest of ``train.main``: cube loading and upload in leg A, engines, steps, scoring pass,
saving), the time inside ``get_inputs`` (image decoding and ``np.load`` of flow files, every call), the bytes under
``optical_flow/UCSDped2/Train`` and in ``foreground_train_*`` when it ends, and its peak host RSS.  One epoch, stock config otherwise.
Prints one JSON line; needs the GPU.

    timeout 900 python tools/time_direct_train.py --frames 400 [--boxes 12] [--work DIR] [--out direct_train.json]
"""
import argparse
import glob
import hashlib
import json
import os
import resource
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

from synthetic_tree import make_tree, metered, tree_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_FLOW = os.path.join('optical_flow', 'UCSDped2', 'Train')
CUBE_GLOB = os.path.join('data', 'raw2flow', '*foreground_train_*')
PAIRS = 4


def leg(direct):
    sys.path.insert(0, ROOT)
    import torch
    import calc_optical_flow as COF
    import foreground as FG
    import vad_datasets as V
    import train as T
    meter = {'decode': 0.0, 'extract': 0.0}
    V.get_inputs = FG.get_inputs = metered(meter, V.get_inputs, 'decode')
    FG.extract_train = metered(meter, FG.extract_train, 'extract', sync=torch.cuda.synchronize)
    FG.extract_train_device = metered(meter, FG.extract_train_device, 'extract', sync=torch.cuda.synchronize)
    torch.manual_seed(0)
    net = COF.FlowNet2().cuda().eval()
    torch.cuda.synchronize()
    res = {'direct': bool(direct)}
    t0 = time.perf_counter()
    flow_s = 0.0
    if not direct:
        ds = V.unified_dataset_interface('UCSDped2', os.path.join('raw_datasets', 'UCSDped2'), context_frame_num=1, mode='train',
                                         border_mode='hard')
        COF.calc_optical_flow(ds, flownet2=net, log=lambda *a: None, pairs_per_launch=PAIRS)
        torch.cuda.synchronize()
        flow_s = time.perf_counter() - t0
        res['flow_stage_decode_s'] = meter['decode']
    T.main('config.cfg', flownet2=net)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    sha = hashlib.sha256()
    for name in ('model', 'raw_training_scores', 'of_training_scores'):
        obj = torch.load(os.path.join('data', 'raw2flow', 'UCSDped2_%s_obj_det_with_motion_SelfComplete.npy' % name), map_location='cpu',
                         weights_only=False)
        cell = obj[0][0]                                    # the stock 1x1 block grid: [state_dict] | score array
        for leaf in (cell if isinstance(cell, list) else [cell]):
            for v in (leaf.values() if isinstance(leaf, dict) else [leaf]):
                sha.update(np.ascontiguousarray(v.numpy() if torch.is_tensor(v) else v).tobytes())
    res.update(wall_s=wall, flow_stage_s=flow_s, extract_s=meter['extract'], train_s=wall - flow_s - meter['extract'],
               decode_s=meter['decode'], flow_bytes=tree_bytes(TRAIN_FLOW),
               cube_file_bytes=sum(os.path.getsize(p) for p in glob.glob(CUBE_GLOB)),
               peak_rss_mb=resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, outputs_sha=sha.hexdigest()[:16])
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400, help='training frames, in two videos')
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg-timeout', type=int, default=600, help='seconds each child process may take')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == 'direct')
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='direct_train_tree_') if own else os.path.abspath(a.work)
    if not own:
        os.makedirs(work, exist_ok=False)
    out_path = os.path.abspath(a.out) if a.out else None
    os.chdir(work)
    try:
        make_tree({'train': (a.frames - a.frames // 2, a.frames // 2)}, a.boxes, flow=False)      # leg A writes FlowNet2's flow, leg B needs none
        cfg = open(os.path.join(ROOT, 'config.cfg')).read().replace('epochs = 10', 'epochs = 1')
        env = dict(os.environ, PYTHONPATH=ROOT)
        from vec_vad_amd import build as B
        res = {'train_frames': a.frames, 'boxes_per_frame': a.boxes, 'pairs_per_launch': PAIRS, 'library_hash': B.wanted()[1][:16], 'legs': []}
        for name in ('staged', 'direct'):
            if name == 'direct':
                shutil.rmtree(TRAIN_FLOW)
                for p in glob.glob(CUBE_GLOB) + glob.glob(os.path.join('data', 'raw2flow', '*SelfComplete.npy')):
                    os.remove(p)
                cfg = cfg.replace('direct_train = False', 'direct_train = True').replace('direct_flow = False', 'direct_flow = True')
            open('config.cfg', 'w').write(cfg)
            # check=True / timeout: an abnormal exit or a child over its limit raises here, and nothing further is started
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name], check=True, env=env, stdout=subprocess.PIPE,
                                 timeout=a.leg_timeout).stdout.decode()
            res['legs'].append(json.loads(out.strip().splitlines()[-1]))
        res['same_outputs'] = res['legs'][0]['outputs_sha'] == res['legs'][1]['outputs_sha']
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
