#!/usr/bin/env python
"""Time several cameras in one scorer (``vec_vad_amd.multistream.MultiStreamScorer``) next to what there was before it -- one
``StreamScorer`` per camera -- on the synthetic UCSDped2-shaped tree of ``tools/synthetic_tree.py`` (240x360 grey .tif frames, one test
video, ``--boxes`` boxes per frame).  FlowNet2 carries seeded random weights (``torch.manual_seed(0)``): its run time does not depend on
them.  After one epoch of ``train.py`` (a child process), for every N of ``--cameras`` and every ``stream_max_boxes`` of ``--max-boxes``
two legs alternate in ONE process, ``--reps`` times; every camera plays the same test video, all in lockstep:

  A  independent  N ``StreamScorer``s pushed round-robin; a tick ends when the results of all N pushes have been waited for;
  B  multi        one ``MultiStreamScorer(cameras=N)``: one ``push`` of N frames; the tick ends when all its results have been waited for.

Per leg: median and 95th percentile of the host time of a tick (from before the first ``push`` to after the last ``wait()``) over the
ticks after ``--warm``, and frames per second as N over the median.  The scores a tick waits for are those of the frames before (one
frame of look-ahead).  For ``--compare`` cameras (default 4) the largest difference between a frame score of leg A and of leg B is
reported too: the launch sizes differ (FlowNet2 at 1 pair against N pairs, scoring launches of ``max_boxes`` against ``N * max_boxes``
cubes), so last-bit differences are expected.

Prints one JSON line; needs the GPU.

    timeout 1100 python tools/time_multistream.py --frames 200 --boxes 12 [--cameras 1,2,4,8] [--max-boxes 16,64] [--out multistream.json]
"""
import argparse
import contextlib
import io
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


def _figures(lat, warm, cams):
    steady = 1e3 * np.array(lat[warm:])
    med = float(np.median(steady))
    return dict(tick_ms_median=med, tick_ms_p95=float(np.percentile(steady, 95)), tick_ms_max=float(steady.max()),
                ticks_timed=int(len(steady)), frames_per_s=1e3 * cams / med)


def independent_leg(c, arts, net, frames, boxes, cams, max_boxes, warm):
    import torch
    from vec_vad_amd.stream import StreamScorer
    scorers = [StreamScorer(c, *arts, frames[0].shape, flownet2=net, max_boxes=max_boxes) for _ in range(cams)]
    torch.cuda.synchronize()
    scores, lat = np.zeros((cams, len(frames))), []

    def take(k, results):
        for r in results:
            scores[k, r.frame] = r.wait()[0]

    for i in range(len(frames)):
        t = time.perf_counter()
        res = [sc.push(frames[i], boxes[i]) for sc in scorers]
        for k in range(cams):
            take(k, res[k])
        lat.append(time.perf_counter() - t)
    for k, sc in enumerate(scorers):
        take(k, sc.end_video())
    return _figures(lat, warm, cams), scores


def multi_leg(c, arts, net, frames, boxes, cams, max_boxes, warm):
    import torch
    from vec_vad_amd.multistream import MultiStreamScorer
    sc = MultiStreamScorer(c, *arts, frames[0].shape, cams, flownet2=net, max_boxes=max_boxes)
    torch.cuda.synchronize()
    scores, lat = np.zeros((cams, len(frames))), []

    def take(results):
        for r in results:
            scores[r.camera, r.frame] = r.wait()[0]

    for i in range(len(frames)):
        t = time.perf_counter()
        take(sc.push([frames[i]] * cams, [boxes[i]] * cams))
        lat.append(time.perf_counter() - t)
    take(sc.end_video())
    return _figures(lat, warm, cams), scores


def measure(a):
    import torch
    import foreground as FG
    import test as S
    import train as T
    from FlowNet2_src import FlowNet2
    from vad_datasets import get_inputs
    work = tempfile.mkdtemp(prefix='multistream_tree_')
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes, flow=True)
        cfg = open(os.path.join(ROOT, 'config.cfg')).read()
        cfg = cfg.replace('epochs = 10', 'epochs = 1').replace('save_score_masks = True', 'save_score_masks = False')
        open('config.cfg', 'w').write(cfg)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=dict(os.environ, PYTHONPATH=ROOT),
                       stdout=subprocess.DEVNULL, timeout=600)
        shutil.rmtree(os.path.join('optical_flow', 'UCSDped2', 'Test'))      # no leg may need a flow file of the test split
        torch.manual_seed(0)
        net = FlowNet2().cuda().eval()
        c = T.read_config('config.cfg')
        with contextlib.redirect_stdout(io.StringIO()):
            st = FG._stage(c, 'test', direct_flow=True)
        frames, boxes = [get_inputs(addr) for addr in st.raw_ds.all_frame_addr], st.boxes
        arts = S.load_artifacts(os.path.join(c['data_root_dir'], c['modality'], 'UCSDped2_'), c['mode_fg'], c['method'], False,
                                lambda: T.build_network(c), torch.device('cuda'))
        runs = []
        for max_boxes in a.max_boxes:
            for cams in a.cameras:
                run = dict(cameras=cams, max_boxes=max_boxes, independent=[], multi=[])
                for _ in range(a.reps):
                    fa, sa = independent_leg(c, arts, net, frames, boxes, cams, max_boxes, a.warm)
                    fb, sb = multi_leg(c, arts, net, frames, boxes, cams, max_boxes, a.warm)
                    run['independent'].append(fa)
                    run['multi'].append(fb)
                    if cams == a.compare:
                        run['largest_score_difference'] = float(np.abs(sa - sb).max())
                        run['largest_score'] = float(np.abs(sa[np.abs(sa) < 1e5]).max()) if (np.abs(sa) < 1e5).any() else None
                        run['same_unscored_frames'] = bool(((np.abs(sa) < 1e5) == (np.abs(sb) < 1e5)).all())
                runs.append(run)
                print(json.dumps(run), flush=True)           # the figures so far, should a later leg fail
        return runs
    finally:
        os.chdir(ROOT)
        shutil.rmtree(work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--cameras', type=lambda s: [int(v) for v in s.split(',')], default=[1, 2, 4, 8])
    ap.add_argument('--max-boxes', type=lambda s: [int(v) for v in s.split(',')], default=[16, 64])
    ap.add_argument('--compare', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vec_vad_amd import build as B
    out_path = os.path.abspath(a.out) if a.out else None
    res = {'frames': a.frames, 'boxes_per_frame': a.boxes, 'warm': a.warm, 'library_hash': B.wanted()[1][:16], 'runs': measure(a)}
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
