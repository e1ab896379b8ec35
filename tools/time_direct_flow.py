#!/usr/bin/env python
"""Time the test stage with the optical flow staged through ``optical_flow/`` files against ``[mi355x] direct_flow = True``, on the
synthetic UCSDped2-shaped tree of ``tools/synthetic_tree.py`` (240x360 grey .tif frames, one test video).  FlowNet2 carries seeded
random weights (``torch.manual_seed(0)``): its run time does not depend on them.  One child process per leg, on the same machine:

  A  ``calc_optical_flow`` on the test split, ``pairs_per_launch=4`` (writes ``optical_flow/UCSDped2/Test...``), then ``test.main``
     with ``direct_test = True`` on those files;
  B  the ``Test`` flow tree removed, ``test.main`` with ``direct_test = True`` and ``direct_flow = True`` (``direct_flow_pairs = 4``).

Each leg reports its wall time (leg A: flow stage and test stage), the time inside ``get_inputs`` (image decoding and ``np.load`` of
flow files, every call) and the bytes under ``optical_flow/UCSDped2/Test`` when it ends.  Leg B then times, with device events
around ``--reps`` repetitions each, the three steps of one 4-pair ``chunk_flows`` launch on 240x360 frames: the ``vv_flow_pairs_prep``
launch, the graph replay and the ``vv_flow_resize_back`` launch, in milliseconds per pair.  Prints one JSON line; needs the GPU.

    timeout 900 python tools/time_direct_flow.py --frames 400 [--boxes 12] [--work DIR] [--out direct_flow.json]
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

from synthetic_tree import make_tree, metered, tree_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEST_FLOW = os.path.join('optical_flow', 'UCSDped2', 'Test')
PAIRS = 4


def step_times(net, reps):
    """Event-timed milliseconds per pair of the three steps of one ``chunk_flows`` launch (4 pairs of 240x360 3-channel frames)."""
    import torch
    from calc_optical_flow import FLOW_H, FLOW_W
    from vec_vad_amd.extract import flow_pairs_prep, flow_resize_back
    frames = torch.randint(0, 256, (PAIRS + 1, 240, 360, 3), dtype=torch.uint8, device='cuda')
    pairs = np.array([[k, k + 1] for k in range(PAIRS)], np.int32)
    rows = np.arange(PAIRS, dtype=np.int32)
    out = torch.empty((PAIRS, 240, 360, 2), device='cuda')
    static_in, static_out, graph = net.graph_entry((PAIRS, 3, 2, FLOW_H, FLOW_W))
    steps = {'prep_ms_per_pair': lambda: flow_pairs_prep(frames, pairs, FLOW_H, FLOW_W, out=static_in),
             'replay_ms_per_pair': graph.replay,
             'resize_back_ms_per_pair': lambda: flow_resize_back(static_out, rows, 240, 360, out)}
    res = {}
    for name, fn in steps.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        res[name] = t0.elapsed_time(t1) / (reps * PAIRS)
    return res


def leg(direct, reps):
    sys.path.insert(0, ROOT)
    import torch
    import calc_optical_flow as COF
    import foreground as FG
    import vad_datasets as V
    import test as S
    meter = {'decode': 0.0}
    V.get_inputs = FG.get_inputs = metered(meter, V.get_inputs, 'decode')
    torch.manual_seed(0)
    net = COF.FlowNet2().cuda().eval()
    torch.cuda.synchronize()
    res = {'direct_flow': bool(direct)}
    t0 = time.perf_counter()
    if not direct:
        ds = V.unified_dataset_interface('UCSDped2', os.path.join('raw_datasets', 'UCSDped2'), context_frame_num=1, mode='test',
                                         border_mode='hard')
        COF.calc_optical_flow(ds, flownet2=net, log=lambda *a: None, pairs_per_launch=PAIRS)
        torch.cuda.synchronize()
        res['flow_stage_s'] = time.perf_counter() - t0
        res['flow_stage_decode_s'] = meter['decode']
    auc = S.main('config.cfg', flownet2=net)
    torch.cuda.synchronize()
    res['wall_s'] = time.perf_counter() - t0
    res['decode_s'] = meter['decode']
    res['flow_bytes'] = tree_bytes(TEST_FLOW)
    fs = np.load('results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy')
    res.update(auc=auc, scores_finite=bool(np.isfinite(fs).all()), scores_sha=hashlib.sha256(fs.tobytes()).hexdigest()[:16])
    if direct:
        res.update(step_times(net, reps))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg == 'direct', a.reps)
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='direct_flow_tree_') if own else os.path.abspath(a.work)
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
        res = {'frames': a.frames, 'boxes_per_frame': a.boxes, 'pairs_per_launch': PAIRS, 'library_hash': B.wanted()[1][:16], 'legs': []}
        cfg = cfg.replace('direct_test = False', 'direct_test = True')
        shutil.rmtree(TEST_FLOW)                       # the synthetic fields: leg A writes FlowNet2's, leg B must not need any
        for name in ('staged', 'direct'):
            if name == 'direct':
                shutil.rmtree(TEST_FLOW)
            open('config.cfg', 'w').write(cfg.replace('direct_flow = False', 'direct_flow = %s' % (name == 'direct')))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name, '--reps', str(a.reps)], check=True, env=env,
                                 stdout=subprocess.PIPE, timeout=900).stdout.decode()
            res['legs'].append(json.loads(out.strip().splitlines()[-1]))
        res['same_scores'] = res['legs'][0]['scores_sha'] == res['legs'][1]['scores_sha']
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
