#!/usr/bin/env python
"""Time the frame-by-frame scorer (``vec_vad_amd.stream.StreamScorer``) next to the closest batch equivalent, on the synthetic
UCSDped2-shaped tree of ``tools/synthetic_tree.py`` (240x360 grey .tif frames, one test video).  FlowNet2 carries seeded random weights
(``torch.manual_seed(0)``): its run time does not depend on them.  After one epoch of ``train.py`` (a child process) the legs alternate
in one process, ``--reps`` times:

  batch   ``test.main`` with ``direct_test``, ``direct_flow``, ``direct_flow_pairs = 1`` and ``direct_frames_per_chunk = 1``: wall time
          of the call over the number of test frames (decoding, model loading, engine set-up and evaluation included);
  stream  every test frame, decoded beforehand, through one ``StreamScorer``: per frame the host clock from before ``push`` to after the
          ``wait()`` of the result that push returned (the score of the frame before: one frame of look-ahead), median and 95th
          percentile over the frames after ``--warm``; and the wall time of the whole loop with the constructor over the frames.

With ``--no-flow-branch`` the same is repeated on a tree trained and scored with ``useFlow = False`` (the flow UNets are gone; FlowNet2
still runs, because the motion test reads its flow).

With ``--stream-boxes motion`` two stream legs alternate instead, on a test video of ``--boxes`` bright rectangles that move over a
static background (``moving_frames``):

  given   the scorer is handed, for every frame, the boxes the batch route's motion stage finds for it (computed beforehand);
  motion  ``StreamScorer(boxes='motion')``: ``push`` gets the frame alone and the scorer finds the same boxes on the device.

Both report the same latency figures, the boxes per frame and the dropped boxes; the largest difference of a frame score is 0 when
every frame's boxes fit ``stream_max_boxes``.

With ``--masks``, ``--smooth`` and / or ``--render`` a third leg alternates with the other two: the same stream with those switches of
the scorer on (``render_range = -5,20``; the picture and the masks are copied out in ``wait()``, inside the timed span), reported as
``stream_pixels`` next to ``stream`` -- the comparison: same process, same box.  ``pixel_launches_us`` is the device time of the added
launches alone, each timed with events over a batch of back-to-back launches on the scorer's own buffers (``--boxes`` rectangles).

With ``--tracks`` a further leg alternates with the others: the same stream through ``StreamScorer(tracks=True)`` with the stock
``track_*`` keys, reported as ``stream_tracks`` next to ``stream``.  ``track_launch_us`` is the device time of ``vv_stream_tracks`` alone,
timed like the pixel launches: ``--boxes`` rectangles that every launch finds where the launch before left them, so a launch is one
matching round in a table of ``stream_max_tracks`` slots.

With ``--maps`` a further leg alternates with the others: the same stream through ``StreamScorer(maps=True)``, reported as
``stream_maps`` next to ``stream`` (the error mask of every frame is copied out in ``wait()``, inside the timed span).
``maps_launches_us`` is the device time of what the switch adds per scored block and round, timed like the pixel launches: the scoring
launch without and with the stored reconstructions and the error maps, ``vv_stream_zpaint`` over ``--boxes`` rectangles, and the copy
of the mask to pinned memory.  ``--no-batch`` leaves the batch leg out (the stream legs do not depend on it).

Prints one JSON line; needs the GPU.

    timeout 900 python tools/time_stream.py --frames 200 [--boxes 12] [--reps 2] [--no-flow-branch] [--out stream.json]
    timeout 900 python tools/time_stream.py --frames 200 --boxes 12 --stream-boxes motion [--out stream_motion.json]
    timeout 900 python tools/time_stream.py --frames 200 --masks --smooth --render [--out stream_masks.json]
    timeout 900 python tools/time_stream.py --frames 200 --boxes 12 --tracks [--out stream_tracks.json]
    timeout 900 python tools/time_stream.py --frames 200 --boxes 12 --maps --no-batch [--out stream_maps.json]
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
SCORES = 'results/UCSDped2/frame_scores_obj_det_with_motion_SelfComplete.npy'


def batch_leg(net, n):
    import torch
    import test as S
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        S.main('config.cfg', flownet2=net)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, ms_per_frame=1e3 * wall / n), np.load(SCORES)


def pixel_launches_us(sc, n_boxes, batch=50):
    """Device time of one launch set of each pixel-level stage of ``sc``, in microseconds: events around ``batch`` back-to-back launches
    on the scorer's own buffers, with ``n_boxes`` rectangles spread over the frame and one row of scores."""
    import torch
    from vec_vad_amd import _lib
    from vec_vad_amd.stream import stream_paint, stream_smooth
    dev, gh, gw = sc.device, sc.grid_h, sc.grid_w
    rng = np.random.default_rng(1)
    y0, x0 = rng.integers(0, gh - 40, n_boxes), rng.integers(0, gw - 40, n_boxes)
    rects = torch.from_numpy(np.stack([y0, y0 + 36, x0, x0 + 30], axis=1).astype(np.int32)).to(dev)
    scores = torch.from_numpy(rng.standard_normal((1, n_boxes)) * 3).to(dev)
    n = torch.tensor([n_boxes], dtype=torch.int32, device=dev)
    box_max = torch.zeros(n_boxes, dtype=torch.float64, device=dev)
    win = torch.tensor([sc.sched.K] + list(range(sc.sched.K)), dtype=torch.int32, device=dev)
    out = {}

    def timed(name, launch):
        launch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            launch()
        b.record()
        b.synchronize()
        out[name] = 1e3 * a.elapsed_time(b) / batch

    timed('vv_stream_paint', lambda: stream_paint(scores, n, n_boxes, rects, None, sc.mask_ring[0], box_max, sc.frame_off))
    if sc.smooth:
        timed('vv_stream_smooth', lambda: stream_smooth(sc.mask_ring, win, sc.kt, sc.ks, sc.Bsum, sc.bcnt, sc.S, sc.partial))
    if sc.render:
        st = torch.cuda.current_stream(dev).cuda_stream
        timed('vv_render_overlay', lambda: _lib.check(_lib.lib().vv_render_overlay(
            sc.raw_ring[0].data_ptr(), sc.C, 1, sc.mask_ring[0].data_ptr(), None, rects.data_ptr(), box_max.data_ptr(),
            sc.frame_off.data_ptr(), n_boxes, sc.lut.data_ptr(), sc.render_lo, sc.render_hi, sc.render_alpha, 1, sc.H, sc.W,
            sc.picture.data_ptr(), st), 'vv_render_overlay'))
    return out


def track_launch_us(sc, n_boxes, batch=50):
    """Device time of one ``vv_stream_tracks`` launch with the settings of ``sc``, in microseconds: events around ``batch`` back-to-back
    launches over a table of its own, ``n_boxes`` rectangles spread over the frame and one row of scores."""
    import torch
    from vec_vad_amd.stream import stream_tracks
    dev, gh, gw = sc.device, sc.grid_h, sc.grid_w
    rng = np.random.default_rng(1)
    y0, x0 = rng.integers(0, gh - 40, n_boxes), rng.integers(0, gw - 40, n_boxes)
    rects = torch.from_numpy(np.stack([y0, y0 + 36, x0, x0 + 30], axis=1).astype(np.int32)).to(dev)
    scores = torch.from_numpy(rng.standard_normal((1, n_boxes)) * 3).to(dev)
    n = torch.tensor([n_boxes], dtype=torch.int32, device=dev)
    t_meta = torch.zeros((sc.trk_max, 8), dtype=torch.int32, device=dev)
    t_hist = torch.zeros((sc.trk_max, sc.trk_window), dtype=torch.float64, device=dev)
    next_id = torch.ones(1, dtype=torch.int32, device=dev)
    box_track = torch.zeros((n_boxes, 2), dtype=torch.int32, device=dev)
    box_score, frame_score = torch.zeros(n_boxes, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)

    def launch():
        stream_tracks(t_meta, t_hist, next_id, scores, n, n_boxes, rects, None, gh, gw, False, sc.trk_iou, sc.trk_age, sc.trk_hits, box_track,
                      box_score, frame_score, counts)

    launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batch):
        launch()
    b.record()
    b.synchronize()
    return dict(vv_stream_tracks=1e3 * a.elapsed_time(b) / batch, live=int(counts[0]), next_id=int(counts[2]))


def maps_launches_us(sc, n_boxes, batch=50):
    """Device time of what ``maps`` adds to one scored block of one round of ``sc``, in microseconds, each timed with events around
    ``batch`` back-to-back calls on the scorer's own store and buffers: the scoring launch without and with the stored reconstructions
    and the error maps (``score_cubes`` / ``score_cubes_maps``: a graph replay plus the launches behind it), ``vv_stream_zpaint`` over
    ``n_boxes`` rectangles of 36x30 pixels, and the copy of the error mask to pinned memory (once per frame)."""
    import torch
    from vec_vad_amd.stream import stream_zpaint
    dev, gh, gw, cap = sc.device, sc.grid_h, sc.grid_w, sc.cap
    rng = np.random.default_rng(1)
    nb = min(n_boxes, cap)
    y0, x0 = rng.integers(0, gh - 40, cap), rng.integers(0, gw - 40, cap)
    rects = torch.from_numpy(np.stack([y0, y0 + 36, x0, x0 + 30], axis=1).astype(np.int32)).to(dev)
    n = torch.tensor([nb], dtype=torch.int32, device=dev)
    ones = torch.ones(cap, dtype=torch.uint8, device=dev)
    tr, stats = next(ent for ent in sc.blocks.values() if ent is not None)
    _, _, e_raw, e_of = tr.score_cubes(sc.store_raw, sc.store_flow, sc.idx, maps=True)
    e_of = e_of if sc.use_flow else None
    host = torch.empty(sc.zmask.shape, dtype=sc.zmask.dtype, pin_memory=True)
    out = {}

    def timed(name, launch):
        for _ in range(3):                               # a graph not yet captured is captured here, outside the events
            launch()
        torch.cuda.synchronize(dev)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            launch()
        b.record()
        b.synchronize()
        out[name] = 1e3 * a.elapsed_time(b) / batch

    timed('score_cubes', lambda: tr.score_cubes(sc.store_raw, sc.store_flow, sc.idx))
    timed('score_cubes_maps', lambda: tr.score_cubes(sc.store_raw, sc.store_flow, sc.idx, maps=True))
    timed('vv_stream_zpaint', lambda: stream_zpaint(e_raw, e_of, stats, sc.w_raw, sc.w_of, ones, ones, n, 0, rects, nb, None, sc.zmask, True))
    timed('error_mask_copy', lambda: host.copy_(sc.zmask, non_blocking=True))
    return dict(out, boxes=nb, cubes_per_launch=cap)


def stream_leg(net, warm, frames=None, boxes=None, mode='given', pixels=None, tracks=False, maps=False):
    """``frames`` / ``boxes`` None: the test split of the tree and its box file.  ``mode='motion'``: ``push`` gets the frames alone.
    ``pixels``: the ``masks`` / ``smooth`` / ``render`` switches of the scorer (None: all off).  ``tracks``: its ``tracks`` switch.
    ``maps``: its ``maps`` switch (the error mask is copied out in ``wait()``, inside the timed span)."""
    import torch
    import foreground as FG
    import test as S
    import train as T
    from vad_datasets import get_inputs
    from vec_vad_amd.stream import StreamScorer
    c = T.read_config('config.cfg')
    if pixels and pixels.get('render'):
        c['render_range'] = (-5.0, 20.0)
    if frames is None:
        with contextlib.redirect_stdout(io.StringIO()):
            st = FG._stage(c, 'test', direct_flow=True)
        frames, boxes = [get_inputs(a) for a in st.raw_ds.all_frame_addr], st.boxes
    n = len(frames)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arts = S.load_artifacts(os.path.join(c['data_root_dir'], c['modality'], 'UCSDped2_'), c['mode_fg'], c['method'], False,
                            lambda: T.build_network(c), torch.device('cuda'))
    sc = StreamScorer(c, *arts, frames[0].shape, flownet2=net, boxes=mode, tracks=tracks, maps=maps, **(pixels or {}))
    torch.cuda.synchronize()
    setup = time.perf_counter() - t0
    scores, lat, found, dropped = np.zeros(n), [], np.zeros(n, np.int64), 0
    fine = np.zeros(n)
    trk = dict(live_max=0, next_id=1, dropped=0, frames_with_a_track_score=0)

    def take(results):
        nonlocal dropped
        for r in results:
            scores[r.frame] = r.wait()[0]
            found[r.frame], dropped = len(r.boxes), dropped + r.dropped
            if maps:
                fine[r.frame] = r.fine_score
            if tracks:
                trk['live_max'], trk['dropped'] = max(trk['live_max'], len(r.tracks)), trk['dropped'] + r.tracks_dropped
                trk['next_id'] = max([trk['next_id']] + [int(i) + 1 for i in r.track_ids])
                trk['frames_with_a_track_score'] += r.track_score > -1e5

    for i in range(n):
        t = time.perf_counter()
        take(sc.push(frames[i]) if mode == 'motion' else sc.push(frames[i], boxes[i]))
        lat.append(time.perf_counter() - t)
    take(sc.end_video())
    wall = time.perf_counter() - t0
    steady = 1e3 * np.array(lat[warm:])
    extra = dict(pixels, pixel_launches_us=pixel_launches_us(sc, max(1, int(found.max())))) if pixels else {}
    if tracks:
        extra.update(tracks=trk, track_launch_us=track_launch_us(sc, max(1, int(found.max()))))
    if maps:
        extra.update(maps_launches_us=maps_launches_us(sc, max(1, int(found.max()))), fine_above_score=int((fine > scores).sum()),
                     fine_support_is_the_scores=bool(((fine > -1e5) == (scores > -1e5)).all()))
    return dict(extra, setup_s=setup, wall_s=wall, wall_ms_per_frame=1e3 * wall / n, push_to_wait_ms_median=float(np.median(steady)),
                push_to_wait_ms_p95=float(np.percentile(steady, 95)), push_to_wait_ms_max=float(steady.max()),
                frames_timed=int(len(steady)), look_ahead_frames=1, max_boxes=sc.cap, boxes_per_frame_mean=float(found.mean()),
                boxes_per_frame_max=int(found.max()), dropped=int(dropped)), scores


def moving_frames(n, rects, seed=5):
    """``n`` grey 240x360 frames for the motion stage: a static low-contrast background (values 96..103) and ``rects`` bright 10 px wide
    rectangles, each in a cell of its own, each moving its own width per frame and turning at the cell's ends -- so the places a
    rectangle has in the three frames of a window touch and the motion stage finds ONE box per rectangle, about ``rects`` per frame."""
    rng = np.random.default_rng(seed)
    H, W = 240, 360
    back = rng.integers(96, 104, (H, W), dtype=np.uint8)
    cols = int(np.ceil(np.sqrt(rects * 1.5)))
    rows = -(-rects // cols)
    ch, cw = H // rows, W // cols
    K = (cw - 8) // 10                                   # places along a cell
    wave = list(range(K)) + list(range(K - 2, 0, -1))
    frames = []
    for t in range(n):
        g = back.copy()
        for r in range(rects):
            y0, x0 = (r // cols) * ch + 4, (r % cols) * cw + 4 + 10 * wave[(t + 3 * r) % len(wave)]
            g[y0:y0 + min(24 + 2 * (r % 5), ch - 8), x0:x0 + 10] = 200
        frames.append(g)
    return frames


def measure_motion(a):
    """``--stream-boxes motion``: the scorer that finds its own boxes next to the scorer that is given the same boxes, alternating in
    one process on the same frames.  The tree is trained as for the other legs; then the test video is replaced by ``moving_frames``
    and its boxes are what the batch route finds for them (``foreground._motion_bboxes``, no detector boxes)."""
    import torch
    import foreground as FG
    import train as T
    from PIL import Image
    from FlowNet2_src import FlowNet2
    work = tempfile.mkdtemp(prefix='stream_tree_')
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes, flow=True)
        cfg = open(os.path.join(ROOT, 'config.cfg')).read()
        cfg = cfg.replace('epochs = 10', 'epochs = 1').replace('save_score_masks = True', 'save_score_masks = False')
        open('config.cfg', 'w').write(cfg)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=dict(os.environ, PYTHONPATH=ROOT),
                       stdout=subprocess.DEVNULL, timeout=600)
        shutil.rmtree(os.path.join('optical_flow', 'UCSDped2', 'Test'))
        os.remove(os.path.join('raw_datasets', 'UCSDped2', 'bboxes_test_obj_det_with_motion.npy'))
        grey = moving_frames(a.frames, a.boxes)
        for k, g in enumerate(grey):
            Image.fromarray(g).save(os.path.join('raw_datasets', 'UCSDped2', 'Test', 'Test001', '%04d.tif' % (k + 1)))
        c = T.read_config('config.cfg')
        boxes = FG._motion_bboxes(c, 'test', os.path.join('raw_datasets', 'UCSDped2', 'bboxes_test_obj_det.npy'), 'cuda', lambda *m: None)
        frames = [np.repeat(g[..., None], 3, axis=2) for g in grey]
        torch.manual_seed(0)
        net = FlowNet2().cuda().eval()
        res = {'useFlow': True, 'stream_boxes': 'motion', 'given': [], 'motion': [],
               'boxes_found_per_frame_mean': float(np.mean([len(b) for b in boxes])), 'boxes_found_per_frame_max': max(len(b) for b in boxes)}
        for _ in range(a.reps):
            g, sg = stream_leg(net, a.warm, frames, boxes, 'given')
            m, sm = stream_leg(net, a.warm, frames, None, 'motion')
            res['given'].append(g)
            res['motion'].append(m)
            res['largest_score_difference'] = float(np.abs(sg - sm).max())
        return res
    finally:
        os.chdir(ROOT)
        shutil.rmtree(work)


def measure(a, use_flow):
    import torch
    from FlowNet2_src import FlowNet2
    work = tempfile.mkdtemp(prefix='stream_tree_')
    os.chdir(work)
    try:
        make_tree({'train': (6, 6), 'test': (a.frames,)}, a.boxes, flow=True)
        cfg = open(os.path.join(ROOT, 'config.cfg')).read()
        cfg = cfg.replace('epochs = 10', 'epochs = 1').replace('save_score_masks = True', 'save_score_masks = False')
        if not use_flow:
            cfg = cfg.replace('useFlow = True', 'useFlow = False')
        open('config.cfg', 'w').write(cfg)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=dict(os.environ, PYTHONPATH=ROOT),
                       stdout=subprocess.DEVNULL, timeout=600)
        shutil.rmtree(os.path.join('optical_flow', 'UCSDped2', 'Test'))      # neither leg may need a flow file of the test split
        cfg = cfg.replace('direct_test = False', 'direct_test = True').replace('direct_flow = False', 'direct_flow = True')
        cfg = cfg.replace('direct_flow_pairs = 4', 'direct_flow_pairs = 1').replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 1')
        open('config.cfg', 'w').write(cfg)
        torch.manual_seed(0)
        net = FlowNet2().cuda().eval()
        res = {'useFlow': use_flow, 'batch': [], 'stream': []}
        pixels = dict(masks=a.masks, smooth=a.smooth, render=a.render) if (a.masks or a.smooth or a.render) else None
        if pixels:
            res['stream_pixels'] = []
        if a.tracks:
            res['stream_tracks'] = []
        if a.maps:
            res['stream_maps'] = []
        for _ in range(a.reps):
            if not a.no_batch:
                b, sb = batch_leg(net, a.frames)
                res['batch'].append(b)
            s, ss = stream_leg(net, a.warm)
            res['stream'].append(s)
            if not a.no_batch:
                res['largest_score_difference'] = float(np.abs(sb - ss).max())
            if a.maps:
                m, sm = stream_leg(net, a.warm, maps=True)
                res['stream_maps'].append(m)
                res['maps_change_a_score'] = bool((sm != ss).any())
            if pixels:
                p, sp = stream_leg(net, a.warm, pixels=pixels)
                res['stream_pixels'].append(p)
                res['pixels_change_a_score'] = bool((sp != ss).any())
            if a.tracks:
                t, st = stream_leg(net, a.warm, tracks=True)
                res['stream_tracks'].append(t)
                res['tracks_change_a_score'] = bool((st != ss).any())
        return res
    finally:
        os.chdir(ROOT)
        shutil.rmtree(work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=200)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--warm', type=int, default=20)
    ap.add_argument('--no-flow-branch', action='store_true')
    ap.add_argument('--stream-boxes', choices=('given', 'motion'), default='given')
    ap.add_argument('--masks', action='store_true')
    ap.add_argument('--smooth', action='store_true')
    ap.add_argument('--render', action='store_true')
    ap.add_argument('--tracks', action='store_true')
    ap.add_argument('--maps', action='store_true')
    ap.add_argument('--no-batch', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    from vec_vad_amd import build as B
    out_path = os.path.abspath(a.out) if a.out else None
    res = {'frames': a.frames, 'boxes_per_frame': a.boxes, 'library_hash': B.wanted()[1][:16]}
    res['runs'] = [measure_motion(a) if a.stream_boxes == 'motion' else measure(a, True)]
    if a.no_flow_branch and a.stream_boxes != 'motion':
        print(json.dumps(res), flush=True)               # the first tree's figures, should the second one fail
        res['runs'].append(measure(a, False))
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
