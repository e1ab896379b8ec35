#!/usr/bin/env python
"""``python stream.py`` -- the configured test split scored frame by frame, as a camera would deliver it.

Every video of the split is pushed through a ``vec_vad_amd.stream.StreamScorer`` one frame at a time (one scorer per scene for
ShanghaiTech): boxes from ``foreground.load_bboxes``, videos from the split's frame indexer, the models and statistics ``train.py``
wrote.  The score of a frame comes back one push later (the flow of a frame needs the next frame; the last frame of a video comes
back at its end).  Writes ``results/<ds>/stream_scores_<fg>_<method>.npy`` and, when the split has frame labels, the frame-level ROC
``results/<ds>/<modality>_<fg>_<method>_stream_results.npz`` (per scene for ShanghaiTech, as ``test.py`` evaluates it) and prints its
AUROC.  ``main`` returns the score vector.  Nothing under ``optical_flow/`` and no cube file is read or written.

With ``[mi355x] stream_boxes = motion`` no ``bboxes_test_*`` file is loaded or written either: every push hands over the frame and the
rows of ``bboxes_test_obj_det.npy`` for it (when that file exists; none otherwise), and the scorer finds the motion boxes itself, so
the boxes are those of ``test_bbox_saved = False`` in mode ``obj_det_with_motion`` (another ``foreground_extraction_mode`` is refused:
the models and statistics are loaded by that mode).  The number of motion boxes that found no free
slot is printed when it is not 0.

``[mi355x] stream_smooth`` also writes ``results/<ds>/stream_scores_smooth_<fg>_<method>.npy`` -- per frame the maximum of the score mask's
mean over the last ``smooth_frames`` frames and ``smooth_pixels`` pixels -- and, with frame labels, its ROC
``..._stream_smooth_results.npz`` and AUROC line.  ``[mi355x] stream_render`` writes ``results/<ds>/stream_render/<frame>.png`` (Pillow,
lossless), the picture of ``test.py``'s render stage without the ground truth.  With either, or ``stream_masks``, a frame's result is
taken one push after it was issued instead of at the end, so that its pinned buffers go back to the scorer's pool.
``stream_scores_*.npy`` is the same file whatever these switches say.

``[mi355x] stream_tracks`` also writes ``results/<ds>/stream_scores_track_<fg>_<method>.npy`` -- per frame the largest mean score of a
track seen ``track_min_hits`` times or more (``StreamResult.track_score``) -- and, with frame labels, its ROC
``..._stream_track_results.npz`` and AUROC line; every other file is the one written without the key.

``[mi355x] stream_maps`` also writes ``results/<ds>/stream_scores_fine_<fg>_<method>.npy`` -- per frame the maximum of the frame's
per-pixel error mask (``StreamResult.fine_score``) -- and, with frame labels, its ROC ``..._stream_fine_results.npz`` and AUROC line;
every other file is the one written without the key, and no mask file is written.  Like the masks above it makes a frame's result
be taken one push after it was issued.

``[mi355x] stream_cameras = N`` (default 1: exactly the run above).  With N > 1 the videos of the split (of each scene for
ShanghaiTech, the scenes one after the other, one ``vec_vad_amd.multistream.MultiStreamScorer`` of N cameras each) are dealt to the
cameras in split order, video ``v`` to camera ``v mod N``, and every camera plays its videos in order.  The cameras run in lockstep
(``camera_ticks``): a tick pushes the next frame of every camera that still has one, in one ``push``; the cameras whose video ended
with that frame are then ended together in one ``end_video([...])`` and start their next video at the next tick; a camera that has
run out of videos passes ``None``.  The schedule depends on the split alone.  The files are those above (``stream_scores_*.npy`` and
``*_stream_results.npz``); a score differs from the run at N = 1 only through the launch sizes.  ``stream_boxes = motion`` and the
``stream_masks`` / ``stream_smooth`` / ``stream_render`` / ``stream_tracks`` / ``stream_maps`` switches are single-camera features: with N > 1 each is
refused with a one-line ``ValueError`` before any GPU work.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from train import read_config, build_network  # noqa: E402
from utils import save_roc_pr_curve_data  # noqa: E402


def results_path(c, scene=None, smooth=False, track=False, fine=False):
    return os.path.join('results', c['dataset_name'], '{}_{}_{}_stream{}_results{}.npz'.format(
        c['modality'], c['mode_fg'], c['method'], '_smooth' if smooth else ('_track' if track else ('_fine' if fine else '')),
        '' if scene is None else '_scene_{}'.format(scene)))


def scores_path(c, smooth=False, track=False, fine=False):
    return os.path.join('results', c['dataset_name'], 'stream_scores{}_{}_{}.npy'.format(
        '_smooth' if smooth else ('_track' if track else ('_fine' if fine else '')), c['mode_fg'], c['method']))


def render_dir(c):
    return os.path.join('results', c['dataset_name'], 'stream_render')


def _evaluate(c, scores, labels, scene_idx, shanghai, smooth=False, track=False, fine=False):
    """The frame-level ROC of a score vector of the stream, written and printed as ``test.py`` does for its own."""
    what = 'smoothed stream' if smooth else ("stream's tracks" if track else ("stream's error maps" if fine else 'stream'))
    if shanghai:
        auc = float(np.mean([save_roc_pr_curve_data(scores[scene_idx == si], labels[scene_idx == si],
                                                    results_path(c, si, smooth, track, fine)) for si in sorted(set(scene_idx))]))
        print('Average frame-level AUC of the {} is {}'.format(what, auc))
    else:
        print('Results written to {}:'.format(results_path(c, smooth=smooth, track=track, fine=fine)))
        auc = save_roc_pr_curve_data(scores, labels, results_path(c, smooth=smooth, track=track, fine=fine))
        print('Frame-level AUC of the {} is {}'.format(what, auc))


def _detector_boxes(c, n, mode='test'):
    """``[mi355x] stream_boxes = motion``: the appearance boxes of every test frame as ``foreground._motion_bboxes`` reads them -- the
    first four columns of the rows of ``bboxes_test_obj_det.npy`` when that file exists (it must hold ``n`` frames), none otherwise.
    ``mode='train'``: those of the training split (``bboxes_train_obj_det.npy``; stream_train.py)."""
    path = os.path.join(c['raw_dataset_dir'], c['dataset_name'], 'bboxes_{}_obj_det.npy'.format(mode))
    if not os.path.exists(path):
        print('no {}: motion boxes only (no appearance boxes)'.format(path))
        return [np.zeros((0, 4), np.float32) for _ in range(n)]
    ap_all = np.load(path, allow_pickle=True)
    if len(ap_all) != n:
        raise ValueError('{} holds boxes of {} frames, the dataset has {}'.format(path, len(ap_all), n))
    return [np.asarray(b)[:, :4] if np.asarray(b).ndim == 2 else np.zeros((0, 4), np.float32) for b in ap_all]


def camera_ticks(videos, cameras):
    """The schedule of ``[mi355x] stream_cameras = N``, pure: ``videos`` (a list of lists of frame indices, in split order) dealt to
    ``cameras`` cameras, video ``v`` to camera ``v % cameras``, each camera playing its videos in order.  Yields the calls of the run in
    order: ``('push', frames)`` with one frame index or None per camera, then, when the frame just pushed was the last of its video for
    some cameras, ``('end', [those cameras])``; a camera that was ended starts its next video with the next push."""
    queues = [videos[k::cameras] for k in range(cameras)]
    vid, pos = [0] * cameras, [0] * cameras
    while True:
        frames = [queues[k][vid[k]][pos[k]] if vid[k] < len(queues[k]) else None for k in range(cameras)]
        if all(f is None for f in frames):
            return
        yield 'push', frames
        ends = []
        for k in range(cameras):
            if frames[k] is not None:
                pos[k] += 1
                if pos[k] == len(queues[k][vid[k]]):
                    ends.append(k)
                    vid[k], pos[k] = vid[k] + 1, 0
        if ends:
            yield 'end', ends


def _main_cameras(c, flownet2):
    """``main`` with ``[mi355x] stream_cameras = N > 1``: per scene one ``MultiStreamScorer`` of N cameras, driven by ``camera_ticks``."""
    from vec_vad_amd.multistream import MultiStreamScorer, check_single_camera_keys, check_stream_maps
    check_single_camera_keys(c)                       # motion boxes, masks, smoothing, overlays, tracks: refused before any GPU work
    check_stream_maps(c)                              # ... and the per-pixel error maps
    import foreground as FG
    from test import BIG, load_artifacts
    from vad_datasets import get_inputs
    ds, cameras = c['dataset_name'], c['stream_cameras']
    shanghai = ds == 'ShanghaiTech'
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(device)
    base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
    st = FG._stage(c, 'test', direct_flow=True)
    scene_idx, labels = FG._write_frame_index(st, ds, 'test')
    indexer, n = st.raw_ds, len(st.raw_ds)
    net_set, st_r, st_o = load_artifacts(base, c['mode_fg'], c['method'], shanghai, lambda: build_network(c), device, c['h_block'],
                                         c['w_block'])
    if flownet2 is None:
        from calc_optical_flow import load_flownet2
        flownet2 = load_flownet2(c['flownet2_checkpoint'], device=device, fp16=c['direct_flow_fp16'])
    scores = np.full(n, -float(BIG), np.float64)
    scenes = {}                                       # scene -> its videos (lists of test frames), both in split order
    for i in range(n):
        if i == 0 or indexer.frame_video_idx[i] != indexer.frame_video_idx[i - 1]:
            video = []
            scenes.setdefault(int(scene_idx[i]) - 1 if shanghai else None, []).append(video)
        video.append(i)
    for key, videos in scenes.items():
        scorer, pushed, results = None, [[] for _ in range(cameras)], []
        for kind, arg in camera_ticks(videos, cameras):
            if kind == 'end':
                results += scorer.end_video(arg)
                continue
            frames = [get_inputs(indexer.all_frame_addr[i]) if i is not None else None for i in arg]
            if scorer is None:
                shape = next(f.shape for f in frames if f is not None)
                scorer = MultiStreamScorer(c, net_set, st_r, st_o, shape, cameras, flownet2=flownet2, scene=key, device=device)
            for k, i in enumerate(arg):
                if i is not None:
                    pushed[k].append(i)
            results += scorer.push(frames, [st.boxes[i] if i is not None else None for i in arg])
        for r in results:
            scores[pushed[r.camera][r.frame]] = r.wait()[0]
    os.makedirs(os.path.join('results', ds), exist_ok=True)
    np.save(scores_path(c), scores)
    if labels is None:
        print('no frame labels for {} -> frame-level evaluation of the stream skipped'.format(ds))
        return scores
    print('Evaluating the stream of {} by frame-criterion:'.format(ds))
    _evaluate(c, scores, labels, scene_idx, shanghai)
    return scores


def main(config_path='config.cfg', flownet2=None):
    c = read_config(config_path)                      # a bad [mi355x] stream_max_boxes / stream_boxes raises here, before any GPU work
    if c['stream_cameras'] > 1:
        return _main_cameras(c, flownet2)
    if c['stream_boxes'] == 'motion' and c['mode_fg'] != 'obj_det_with_motion':
        # the boxes would be obj_det_with_motion's while the models and statistics are loaded by mode_fg
        raise ValueError("[mi355x] stream_boxes = motion scores the boxes of mode obj_det_with_motion; the configured mode is "
                         "{!r}".format(c['mode_fg']))
    from vad_datasets import frame_size
    from vec_vad_amd.stream import check_pixel_settings
    nominal = frame_size[c['dataset_name']][:2]
    check_pixel_settings(c, None, None, None, nominal, nominal)      # what the keys alone can get wrong is refused here, before any GPU work
    import foreground as FG
    from test import BIG, load_artifacts
    from vad_datasets import get_inputs
    from vec_vad_amd.stream import StreamScorer
    ds = c['dataset_name']
    shanghai = ds == 'ShanghaiTech'
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(device)
    motion = c['stream_boxes'] == 'motion'
    base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
    if motion:                                        # the frame indexer alone: no bboxes_test_* file is loaded or written
        from types import SimpleNamespace
        os.makedirs(os.path.join(c['data_root_dir'], c['modality']), exist_ok=True)
        st = SimpleNamespace(raw_ds=FG._datasets(c, 'test', None, direct_flow=True)[0], base=base)
        st.boxes = _detector_boxes(c, len(st.raw_ds))
    else:
        st = FG._stage(c, 'test', direct_flow=True)   # boxes and the frame indexer over the raw tree; no flow file is globbed
    scene_idx, labels = FG._write_frame_index(st, ds, 'test')
    indexer, n = st.raw_ds, len(st.raw_ds)
    net_set, st_r, st_o = load_artifacts(base, c['mode_fg'], c['method'], shanghai, lambda: build_network(c), device, c['h_block'],
                                         c['w_block'])
    if flownet2 is None:
        from calc_optical_flow import load_flownet2
        flownet2 = load_flownet2(c['flownet2_checkpoint'], device=device, fp16=c['direct_flow_fp16'])
    scores = np.full(n, -float(BIG), np.float64)
    pixels = c['stream_masks'] or c['stream_smooth'] or c['stream_render'] or c['stream_maps']
    smooth_scores = np.full(n, -float(BIG), np.float64) if c['stream_smooth'] else None
    track_scores = np.full(n, -float(BIG), np.float64) if c['stream_tracks'] else None
    fine_scores = np.full(n, -float(BIG), np.float64) if c['stream_maps'] else None
    if c['stream_render']:
        from PIL import Image
        os.makedirs(render_dir(c), exist_ok=True)
    scorers, pushed, results = {}, {}, []             # per scene: the scorer, the test frames it was given in push order
    dropped = 0

    def take(upto):
        """The results ``results[:upto]``, waited for and filed; they leave the list."""
        nonlocal dropped
        for key, r in results[:upto]:
            f = pushed[key][r.frame]
            scores[f] = r.wait()[0]
            dropped += r.dropped
            if smooth_scores is not None:
                smooth_scores[f] = r.smooth_score
            if track_scores is not None:
                track_scores[f] = r.track_score
            if fine_scores is not None:
                fine_scores[f] = r.fine_score
            if r.picture is not None:
                Image.fromarray(r.picture).save(os.path.join(render_dir(c), '{}.png'.format(f)))
        del results[:upto]

    last = None                                       # the scene of the frame before
    for i in range(n):
        frame = get_inputs(indexer.all_frame_addr[i])
        key = int(scene_idx[i]) - 1 if shanghai else None
        if i > 0 and indexer.frame_video_idx[i] != indexer.frame_video_idx[i - 1]:
            results += [(last, r) for r in scorers[last].end_video()]
        if key not in scorers:
            scorers[key] = StreamScorer(c, net_set, st_r, st_o, frame.shape, flownet2=flownet2, scene=key, device=device)
            pushed[key] = []
        pushed[key].append(i)
        results += [(key, r) for r in scorers[key].push(frame, st.boxes[i])]
        last = key
        if pixels:                                    # all but the newest: the device stays one frame ahead of the host
            take(len(results) - 1)
    if n:
        results += [(last, r) for r in scorers[last].end_video()]
    take(len(results))
    if dropped:
        print('{} motion boxes found no free slot and were dropped: raise [mi355x] stream_max_boxes ({})'.format(
            dropped, c['stream_max_boxes']))
    os.makedirs(os.path.join('results', ds), exist_ok=True)
    np.save(scores_path(c), scores)
    if smooth_scores is not None:
        np.save(scores_path(c, smooth=True), smooth_scores)
    if track_scores is not None:
        np.save(scores_path(c, track=True), track_scores)
    if fine_scores is not None:
        np.save(scores_path(c, fine=True), fine_scores)
    if labels is None:
        print('no frame labels for {} -> frame-level evaluation of the stream skipped'.format(ds))
        return scores
    print('Evaluating the stream of {} by frame-criterion:'.format(ds))
    _evaluate(c, scores, labels, scene_idx, shanghai)
    if smooth_scores is not None:
        _evaluate(c, smooth_scores, labels, scene_idx, shanghai, smooth=True)
    if track_scores is not None:
        _evaluate(c, track_scores, labels, scene_idx, shanghai, track=True)
    if fine_scores is not None:
        _evaluate(c, fine_scores, labels, scene_idx, shanghai, fine=True)
    return scores


if __name__ == '__main__':
    main()
