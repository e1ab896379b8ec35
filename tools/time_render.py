#!/usr/bin/env python
"""Time the render stage (``[mi355x] render = True``): the two kernels on one chunk next to their numpy restatement
(``tests/render_restatement.py``) and the PNG encoding on the host, and ``test.main`` with the key off and on.

  chunk leg: ``--chunk`` frames of 240x360 -- random BGR frames, masks of 12 random boxes of normal-distributed scores per frame, the
    boxes themselves, a ground-truth blob on every other frame, random flow fields.  ``vv_render_overlay`` and ``vv_flow_color`` (per
    image and with a fixed radius) through the bare ABI on buffers kept between calls, and ``render.overlay`` / ``render.flow_color``
    (checks, tables to the device, outputs from the caching allocator), are timed with device events after a warm-up.  The restatement
    runs once on the host -- the overlay on the first ``--host-frames`` frames only (it walks pixels in Python) -- and must equal the
    device's overlay bit for bit and its flow image within one level outside the band at ``rad = 1``.  The pictures of the chunk, with
    and without the flow panel, are encoded to PNG in memory with Pillow at its default settings, as the stage does.
  main legs: the synthetic UCSDped2-shaped tree of ``tools/synthetic_tree.py``; the cube files are extracted once, outside the timed
    runs, then ``test.main`` is timed with the key off, on, and on with ``render_flow`` (``save_score_masks`` off in all three); inside
    the stage the decoding, the two device calls and the PNG writes are timed on the host clock between device synchronisations.

Every GPU step runs in a child process of its own under its own time limit, one GPU process at a time.  Prints one JSON line; needs
the GPU.

    timeout 1500 python tools/time_render.py --frames 400 [--boxes 12] [--chunk 64] [--reps 200] [--host-frames 4] [--work DIR] [--out render.json]
"""
import argparse
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
H, W = 240, 360


def stats(ms):
    return {'median': float(np.median(ms)), 'min': float(min(ms)), 'max': float(max(ms))}


def chunk_leg(chunk, reps, host_frames):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch
    from PIL import Image
    from vec_vad_amd import render, _lib
    import render_restatement as R
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (chunk, H, W, 3), dtype=np.uint8)
    mask = np.full((chunk, H, W), -100000.0)
    gt = np.zeros((chunk, H, W), np.uint8)
    gt[1::2, 100:120, 100:130] = 255
    rects, scores = [], []
    for f in range(chunk):
        for _ in range(12):
            y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            y1, x1 = min(H, y0 + int(rng.integers(8, 65))), min(W, x0 + int(rng.integers(8, 65)))
            s = float(rng.standard_normal())
            mask[f, y0:y1, x0:x1] = np.maximum(mask[f, y0:y1, x0:x1], s)
            rects.append((y0, y1, x0, x1))
            scores.append(s)
    rects, scores = np.array(rects, np.int32), np.array(scores)
    off = (12 * np.arange(chunk + 1)).astype(np.int32)
    lo, hi, alpha = float(scores.min()), float(scores.max()), 128
    flow = (2 * rng.standard_normal((chunk, H, W, 2))).astype(np.float32)
    lut = render.colormap()
    d = {k: torch.from_numpy(v).cuda() for k, v in dict(frames=frames, mask=mask, gt=gt, rects=rects, scores=scores, off=off, flow=flow,
                                                       lut=lut).items()}

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

    l = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    img = torch.empty((chunk, H, W, 3), dtype=torch.uint8, device='cuda')
    fimg = torch.empty((chunk, H, W, 3), dtype=torch.uint8, device='cuda')
    work = torch.empty(int(l.vv_flow_color_work(chunk, H, W)), dtype=torch.uint8, device='cuda')

    def bare_overlay():
        _lib.check(l.vv_render_overlay(d['frames'].data_ptr(), 3, 1, d['mask'].data_ptr(), d['gt'].data_ptr(), d['rects'].data_ptr(),
                                       d['scores'].data_ptr(), d['off'].data_ptr(), len(scores), d['lut'].data_ptr(), lo, hi, alpha, chunk, H, W,
                                       img.data_ptr(), st), 'vv_render_overlay')

    def bare_flow(maxrad):
        _lib.check(l.vv_flow_color(d['flow'].data_ptr(), chunk, H, W, maxrad, fimg.data_ptr(), work.data_ptr(), st), 'vv_flow_color')

    res = {'chunk_frames': chunk, 'reps': reps, 'boxes_per_frame': 12, 'painted_fraction': float((mask != -100000.0).mean()),
           'vv_render_overlay_ms': stats(events(bare_overlay)),
           'overlay_ms': stats(events(lambda: render.overlay(d['frames'], d['mask'], d['rects'], d['scores'], off, lo, hi, alpha, gt=d['gt']))),
           'vv_flow_color_fixed_radius_ms': stats(events(lambda: bare_flow(8.0))),
           'vv_flow_color_per_image_ms': stats(events(lambda: bare_flow(0.0))),
           'flow_color_ms': stats(events(lambda: render.flow_color(d['flow'])))}
    bare_overlay()
    bare_flow(0.0)
    got, fgot = img.cpu().numpy(), fimg.cpu().numpy()
    k = min(host_frames, chunk)
    t0 = time.perf_counter()
    want = R.overlay(frames[:k], mask[:k], rects, scores, off[:k + 1], lo, hi, alpha, gt=gt[:k], lut=lut)
    res['host_overlay_ms_per_frame'] = 1e3 * (time.perf_counter() - t0) / k
    res['host_overlay_frames'] = k
    res['overlay_restatement_equals_device'] = bool(np.array_equal(want, got[:k]))
    t0 = time.perf_counter()
    parts = [R.flow_parts(f) for f in flow]
    res['host_flow_color_ms_per_frame'] = 1e3 * (time.perf_counter() - t0) / chunk
    worst, left_out = 0, 0
    for (fw, rad, _), fg in zip(parts, fgot):
        band = np.abs(rad - 1) < 1e-5
        left_out = max(left_out, int(band.sum()))
        worst = max(worst, int(np.abs(fw.astype(int) - fg.astype(int)).max(axis=2)[~band].max()))
    res['flow_color_largest_difference_outside_band'] = worst
    res['flow_color_band_pixels_per_image_max'] = left_out
    for key, pics in (('png_encode_ms_per_frame', got), ('png_encode_with_flow_panel_ms_per_frame', np.concatenate([got, fgot], axis=2))):
        t0, size = time.perf_counter(), 0
        for p in pics:
            buf = io.BytesIO()
            Image.fromarray(p).save(buf, format='PNG')
            size += buf.tell()
        res[key] = 1e3 * (time.perf_counter() - t0) / chunk
        res[key.replace('_ms_per_frame', '_bytes_per_frame')] = size // chunk
    print(json.dumps(res))


def main_leg():
    sys.path.insert(0, ROOT)
    import torch
    from PIL import Image
    import test as S
    import vad_datasets
    from vec_vad_amd import render, scoring
    sync = torch.cuda.synchronize
    times = {k: [] for k in ('stage', 'decode', 'paint', 'overlay', 'flow_color', 'png')}

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

    stage = S._render_stage

    def in_stage(*a, **k):      # the patched functions also serve other stages: only the calls of this one are counted
        keep = vad_datasets.get_inputs, scoring.paint_masks, render.overlay, render.flow_color, Image.Image.save
        vad_datasets.get_inputs, scoring.paint_masks = timed(keep[0], 'decode'), timed(keep[1], 'paint')
        render.overlay, render.flow_color = timed(keep[2], 'overlay'), timed(keep[3], 'flow_color')
        Image.Image.save = timed(keep[4], 'png')
        try:
            return stage(*a, **k)
        finally:
            vad_datasets.get_inputs, scoring.paint_masks, render.overlay, render.flow_color, Image.Image.save = keep

    S._render_stage = timed(in_stage, 'stage')
    sync()
    t0 = time.perf_counter()
    S.main('config.cfg')
    sync()
    res = {'wall_s': time.perf_counter() - t0}
    if times['stage']:
        res.update(stage_ms=1e3 * times['stage'][0], pictures=len(times['png']))
        for key in ('decode', 'paint', 'overlay', 'flow_color', 'png'):
            res[key + '_calls'] = len(times[key])
            res[key + '_ms_total'] = 1e3 * sum(times[key])
        if len(times['overlay']) > 2:
            res['overlay_median_ms'] = 1e3 * float(np.median(times['overlay'][1:-1]))      # the first call is cold, the last chunk may be short
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=400)
    ap.add_argument('--boxes', type=int, default=12)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--host-frames', type=int, default=4)
    ap.add_argument('--work', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--leg', choices=('chunk', 'main'), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg == 'chunk':
        return chunk_leg(a.chunk, a.reps, a.host_frames)
    if a.leg == 'main':
        return main_leg()
    sys.path.insert(0, ROOT)
    own = a.work is None
    work = tempfile.mkdtemp(prefix='render_tree_') if own else os.path.abspath(a.work)
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
        res['chunk'] = child(me + ['--leg', 'chunk', '--chunk', str(a.chunk), '--reps', str(a.reps), '--host-frames', str(a.host_frames)], 300)
        make_tree({'train': (6, 6), 'test': (a.frames // 2, a.frames - a.frames // 2)}, a.boxes)
        stock = open(os.path.join(ROOT, 'config.cfg')).read().replace('epochs = 10', 'epochs = 1')
        for key in ('save_score_masks = True', 'render = False', 'render_flow = False', 'direct_frames_per_chunk = 64'):
            assert key in stock, key
        stock = stock.replace('save_score_masks = True', 'save_score_masks = False').replace('direct_frames_per_chunk = 64',
                                                                                             'direct_frames_per_chunk = %d' % a.chunk)
        open('config.cfg', 'w').write(stock)
        print('training and extracting the cube files', file=sys.stderr, flush=True)
        subprocess.run([sys.executable, os.path.join(ROOT, 'train.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=600)
        subprocess.run([sys.executable, os.path.join(ROOT, 'test.py')], check=True, env=env, stdout=subprocess.DEVNULL, timeout=900)   # cube files
        saved = stock.replace('test_foreground_saved = False', 'test_foreground_saved = True')
        on = saved.replace('render = False', 'render = True')
        for tag, text in (('off', saved), ('on', on), ('on_flow', on.replace('render_flow = False', 'render_flow = True'))):
            shutil.rmtree('results', ignore_errors=True)
            open('config.cfg', 'w').write(text)
            res['main_' + tag] = child(me + ['--leg', 'main'], 900)
        res['pictures_written'] = len(os.listdir('results/UCSDped2/render'))
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
