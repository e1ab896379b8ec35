"""Frame-by-frame scoring on the GPU: one frame and its boxes in, that frame's anomaly score out (``StreamScorer``).

Every other route through this code base scores a finished test split.  A stream is a sequence of videos of one camera; for frame ``t``
of a video the scorer builds the cubes ``test.py`` builds for it -- the raw window ``context_range(t, 'predict', context_frame_num)``
inside the video (the first frame repeated at its start), the flow window the same over ``context_of_num``, the flow field of a frame
computed from the pair ``calc_optical_flow.flow_pairs`` names for it -- and scores them with the models, statistics, weights, motion
threshold and block grid of the configuration, exactly as ``test.py`` does.

Look-ahead.  The pair of a frame that is not the last of its video contains the NEXT frame, so the score of frame ``t`` is issued when
frame ``t + 1`` is pushed, and the last frame of a video when ``end_video()`` is called: a latency floor of one frame.  A video that
ends after one frame has no pair the batch route accepts next to another video; ``end_video()`` raises a one-line ``ValueError``.

Rings.  The last ``ring_frames(context_frame_num) = context_frame_num + 2`` frames live in a device ring: the ``context_frame_num + 1``
frames of the raw window of the frame that is being issued plus the one frame of look-ahead behind it.  The flow fields live in a second
ring of ``flow_ring_frames(context_of_num) = context_of_num + 1`` slots -- the flow window of the frame being issued, whose own field is
written in place when it is issued (``vv_flow_pairs_prep`` -> FlowNet2's captured graph at one pair per launch -> ``vv_flow_resize_back``:
the launches of ``calc_optical_flow.chunk_flows``, so the fields are those of ``direct_flow_pairs = 1``).  ``RingSchedule`` is that
bookkeeping as a pure class.

No host decision between upload and read-back.  ``push`` copies the frame into its ring slot and sends ONE small descriptor per issued
frame through a pinned staging buffer: the box rectangles as ``boxes_to_crops`` forms them, their number, the ring slots of the two
windows, the flow pair and the per-block masks.  Everything else is enqueued on the current stream: ``vv_stream_cut`` cuts the cubes of
the boxes into slots ``0..n-1`` of a fixed store of ``max_boxes`` cubes and applies the motion test; every block of the grid that has a
model scores the WHOLE store in its own fixed-size launch (the eval-mode graph of ``FusedTrainer.score_cubes``), and
``vv_stream_scores`` turns the error sums into box scores and max-accumulates the frame score under ``keep`` and the block's mask, with
no compaction.  The scores go to pinned host memory behind an event; ``StreamResult.wait()`` waits on that event and on nothing else.
A frame with more boxes than ``max_boxes`` takes ``ceil(n / max_boxes)`` rounds of the same launches, max-accumulated on the device.

Boxes found on the device (``boxes='motion'``, ``[mi355x] stream_boxes = motion``).  ``push`` then takes the frame alone, and
optionally the frame's detector boxes.  The boxes of a frame are those of ``test_bbox_saved = False`` in mode ``obj_det_with_motion``:
the detector's, followed by the motion boxes of the window ``context_range(t, 'hard', 1)`` = the frame and its two neighbours inside
the video -- the look-ahead frame the flow pair already waits for, so nothing is added to the latency floor (the raw ring holds
``max(ring_frames, 3)`` frames).  Behind the flow launches ``vv_motion_mask`` (one window, read from the descriptor, which also carries
the detector boxes as the table the mask erases) and ``vv_mask_boxes`` (through the C ABI into buffers allocated once; count and boxes
stay on the device) find the boxes, and ``vv_stream_boxes`` does for them what ``push`` does on the host for given boxes: crops, the
painted-rectangle test and the per-block masks, written behind the detector boxes' slots.  The host learns the number of boxes only
with the scores (``StreamResult.boxes`` / ``.dropped`` after ``wait()``), and that has two prices.  A frame is ONE round: motion boxes
beyond the slots the detector boxes leave free of ``max_boxes`` are dropped, in ``vv_mask_boxes``' emission order, and counted.  And
EVERY block of the ``h_block x w_block`` grid is scored for every frame -- a scoring launch of ``max_boxes`` cubes per block that has
a model -- since the host cannot know which blocks the motion boxes fall into.  Frames larger than the dataset's nominal frame are
refused in this mode: a motion box could then lie outside the block grid, which the host refuses for given boxes and cannot see here.

Where in the frame (``masks`` / ``smooth`` / ``render``; ``[mi355x] stream_masks`` / ``stream_smooth`` / ``stream_render``, all off by
default -- then nothing more is allocated, launched or copied).  Behind the frame's last ``vv_stream_scores`` the tables that are on
the device anyway -- the box-score rows, the box count, the boxes -- become pixels, with no word to the host in between.
``vv_stream_paint`` (one launch) paints the frame's score mask over the dataset's nominal frame, the mask ``test.paint_frame`` paints
from the box scores and boxes ``wait()`` returns: rectangles of given boxes ride in the descriptor as ``scoring.box_rects`` resolves
them, those of motion boxes are resolved by the kernel.  ``vv_stream_smooth`` is the filter of ``[mi355x] smooth_masks`` made causal:
the stream counts ``smooth_frames`` BACKWARDS from the frame (the frames ``max(0, t - smooth_frames + 1) .. t`` of the video), where
``test.py`` centres its window, so the values are those of the centred filter of ``2 smooth_frames - 1`` frames on a split that ends
at the frame, not those of ``score_mask_smooth``.  The masks live in a ring of ``smooth_frames`` slots next to their X/Y sums, so a
frame costs one frame's spatial passes.  ``vv_render_overlay`` then draws the picture of ``[mi355x] render`` from the frame as it lies
in the raw ring (no ground truth; ``render_range`` must be two numbers, since ``auto`` needs the whole run).  Masks and picture reach
the host in pooled pinned buffers behind the event ``wait()`` already waits on, which copies them out.

Which object, and for how long (``tracks``; ``[mi355x] stream_tracks``, off by default -- then nothing more is allocated, launched or
copied).  One more launch over the same tables, ``vv_stream_tracks``, links the frame's boxes to the tracks of the video's earlier
frames: greedy matching by IoU in integers, best pair first, in a table of ``stream_max_tracks`` slots that stays on the device and is
emptied at the first frame of a video (``RingSchedule`` says which that is).  A track keeps the scores of its last ``track_window``
matches; a box's track score is their mean, the frame's the largest over tracks matched ``track_min_hits`` times or more, so that one
badly reconstructed cube of an object seen once cannot raise the alarm, and a track that finds no box coasts ``track_max_age`` frames.
It needs the descriptor's tail (the count and the host's rectangles) but no mask; its outputs and the table ride to pinned memory in
one copy behind the same event (``StreamResult.track_ids`` / ``.track_hits`` / ``.track_scores`` / ``.track_score`` /
``.tracks_dropped`` / ``.tracks``).  The defaults of its keys are untuned picks; no accuracy is claimed for them.

Where inside a box (``maps``; ``[mi355x] stream_maps``, off by default -- then nothing more is allocated, launched or copied).  A
score mask is constant over every rectangle.  With ``maps`` every scoring launch is the one that also stores its reconstructions
(``FusedTrainer.score_cubes(maps=True)``, a captured graph of its own, warmed at construction; its error sums are the bits of the
plain launch, so score, box scores and keep flags do not change), and behind each block's ``vv_stream_scores`` one
``vv_stream_zpaint`` paints that launch's per-pixel errors into the frame's error mask: for every box that counts -- the same count on
the device, keep flags and mask row -- the 32 x 32 map of z-scores, stretched over the box's rectangle, max-combined over boxes,
blocks and rounds.  It is ``scoring.error_zmaps`` + ``scoring.paint_error_masks`` of the batch route in one launch, bit for bit, for
boxes the host may not even know: rectangles of motion boxes are resolved by the kernel.  The frame's first launch writes the mask
whole (a frame without a box gets one background launch), so there is no fill.  ``StreamResult.error_mask`` arrives in a pooled
pinned buffer behind the event ``wait()`` already waits on, ``StreamResult.fine_score`` is its maximum.  It needs the descriptor's
tail but neither the score mask nor the tracks; smoothing and overlays keep working on the score mask, not on this one.

What is not here: the mmdet detector (detector boxes are the caller's), decoding, a centred (delayed) smoothing window, smoothing or
rendering of the error mask, the pixel and region criteria of ``test.py``, and for the tracks motion prediction, assignment by the
Hungarian method, re-identification and ids drawn into the picture.  Several cameras in one scorer are
``vec_vad_amd.multistream.MultiStreamScorer`` (one frame shape and one model set, given boxes, scores only): the motion boxes, masks,
smoothing, overlays, tracks and error maps described above stay features of this single-camera class.  The models and statistics a
scorer is built from can come from pushed frames too (``vec_vad_amd.stream_train.StreamCollector``).  All three classes derive from
``vec_vad_amd.stream_front.StreamFront``, which owns everything up to and including ``vv_stream_cut`` -- the refusals, rings and
stores, ``RingSchedule``, the host side of a frame, the descriptor (``tick_descriptor`` at one camera, with the motion tables and this
class's tail behind its first round), the flow and the motion front; the names that used to be defined here are re-imported from
there.  This module holds what stands behind the cut: the score, paint, smooth, track and map stages and ``StreamResult``.
"""
import numpy as np
import torch

from . import _lib
from .scoring import BIG
from .stream_front import (RingSchedule, StreamFront, _Staging, _dev, check_frame, check_max_boxes, check_stream_boxes,  # noqa: F401
                           flow_ring_frames, motion_ring_frames, ring_frames, stream_boxes, stream_cut)


def stream_scores(raw, of, stats, w_raw, w_of, keep, n, mask, box_scores, frame_score):
    """``vv_stream_scores``: one block's share of a frame score.  raw / of: float32 ``[cap]`` error sums of a scoring launch over the
    store (``of`` None drops the flow term; ``raw`` may be None with ``stats`` None); stats: float64 ``[4]`` device tensor ``(mu_r, sd_r,
    mu_o, sd_o)`` or None for a block without a model; keep uint8 ``[cap]``, n int32 ``[1]``, mask uint8 ``[cap]`` = the boxes of the
    block, all on the device; box_scores float64 ``[cap]`` and frame_score float64 ``[1]`` are written in place: box ``b < n[0]`` gets
    the score of ``scoring.cube_scores`` when ``keep[b]`` and ``mask[b]`` (``+BIG`` without a model) and enters ``frame_score[0] =
    max(frame_score[0], ...)``, else ``-BIG``; slots ``>= n[0]`` are not written and nothing they hold is read."""
    cap = _dev('box_scores', box_scores, torch.float64).numel()
    _dev('frame_score', frame_score, torch.float64, 1), _dev('keep', keep, torch.uint8, cap), _dev('mask', mask, torch.uint8, cap)
    _dev('n', n, torch.int32, 1)
    if stats is not None:
        _dev('stats', stats, torch.float64, 4), _dev('raw', raw, torch.float32, cap)
        if of is not None:
            _dev('of', of, torch.float32, cap)
    _lib.check(_lib.lib().vv_stream_scores(raw.data_ptr() if stats is not None else None,
                                           of.data_ptr() if (stats is not None and of is not None) else None,
                                           stats.data_ptr() if stats is not None else None, float(w_raw), float(w_of), float(BIG),
                                           keep.data_ptr(), n.data_ptr(), mask.data_ptr(), cap, box_scores.data_ptr(),
                                           frame_score.data_ptr(), torch.cuda.current_stream(box_scores.device).cuda_stream),
               'vv_stream_scores')


PAINT_STAGE = 256      # boxes ``vv_stream_paint`` stages in LDS per pass (VV_STREAM_PAINT_STAGE)
SMOOTH_MAX = 33        # VV_SMOOTH_MAX: the widest window of ``vv_stream_smooth``, in frames and in pixels


def stream_paint(scores, n, n_host, rects, boxes, mask, box_max, frame_off):
    """``vv_stream_paint``: the score mask of one issued frame.  scores float64 ``[rows,width]`` (the box-score rows of
    ``vv_stream_scores``), n int32 ``[1]``, rects int32 ``[width,4]`` rows ``(y0, y1, x0, x1)`` (16-byte aligned; rows below
    ``n_host`` resolved by the host with ``scoring.box_rects``), boxes int32 ``[width,4]`` rows ``(x1, y1, x2, y2)`` or None, all on
    the device.  Written in place: mask float64 ``[h,w]`` whole (``-BIG`` where no box reaches), box_max float64 ``[width]`` below
    ``n[0]``, rows ``n_host..n[0]-1`` of rects (Python's slicing of the device's boxes) and frame_off int32 ``[2] = (0, n)``.  Slots
    at or above ``n[0]`` are neither read nor written."""
    _dev('scores', scores, torch.float64), _dev('mask', mask, torch.float64), _dev('n', n, torch.int32, 1)
    if scores.dim() != 2 or mask.dim() != 2:
        raise ValueError('scores must be a [rows,width] and mask an [h,w] tensor')
    rows, width = scores.shape
    _dev('rects', rects, torch.int32, 4 * width), _dev('box_max', box_max, torch.float64, width), _dev('frame_off', frame_off, torch.int32, 2)
    if boxes is not None:
        _dev('boxes', boxes, torch.int32, 4 * width)
    _lib.check(_lib.lib().vv_stream_paint(scores.data_ptr(), rows, width, n.data_ptr(), int(n_host), rects.data_ptr(),
                                          boxes.data_ptr() if boxes is not None else None, mask.shape[0], mask.shape[1], mask.data_ptr(),
                                          box_max.data_ptr(), frame_off.data_ptr(), torch.cuda.current_stream(mask.device).cuda_stream),
               'vv_stream_paint')


def stream_zpaint(e_raw, e_of, stats, w_raw, w_of, keep, mask, n, slot0, rects, n_host, boxes, out, first):
    """``vv_stream_zpaint``: one block's share of one round of a frame's per-pixel error mask.  e_raw / e_of: float32 ``[cap,32,32]``,
    the per-pixel errors of a scoring launch over the store (``FusedTrainer.score_cubes(maps=True)``; ``e_of`` None drops the flow term;
    both may be None with ``stats`` None); stats, w_raw, w_of, keep uint8 ``[cap]``, n int32 ``[1]`` and mask uint8 ``[cap]`` as for
    ``stream_scores`` (``cap`` is ``keep``'s length); rects int32 ``[width,4]`` rows ``(y0, y1, x0, x1)`` of the FRAME, of which the
    round's are rows ``slot0 .. slot0 + cap - 1``; rows below ``n_host`` are the host's (``scoring.box_rects``), the others are resolved
    from boxes int32 ``[width,4]`` rows ``(x1, y1, x2, y2)`` as ``stream_paint`` resolves them (None: every rectangle is the host's).
    out float64 ``[h,w]`` is written in place: pixel ``(y, x)`` of the rectangle of a slot ``b < n[0]`` with ``keep[b]`` and ``mask[b]``
    is max-combined with the value ``scoring.error_zmaps`` + ``scoring.paint_error_masks`` give it (``+BIG`` without a model).
    ``first``: the mask is written whole over a background of ``-BIG`` and what ``out`` held is not read; else the launch accumulates.
    The maps of a slot that does not count are not read."""
    _dev('out', out, torch.float64), _dev('keep', keep, torch.uint8), _dev('n', n, torch.int32, 1)
    if out.dim() != 2:
        raise ValueError('out must be an [h,w] tensor')
    cap, slot0 = keep.numel(), int(slot0)
    if slot0 < 0:
        raise ValueError('slot0 must not be negative, got {}'.format(slot0))
    _dev('mask', mask, torch.uint8, cap), _dev('rects', rects, torch.int32, 4 * (slot0 + cap))
    if boxes is not None:
        _dev('boxes', boxes, torch.int32, 4 * (slot0 + cap))
    if stats is not None:
        _dev('stats', stats, torch.float64, 4), _dev('e_raw', e_raw, torch.float32, 1024 * cap)
        if e_of is not None:
            _dev('e_of', e_of, torch.float32, 1024 * cap)
    _lib.check(_lib.lib().vv_stream_zpaint(e_raw.data_ptr() if stats is not None else None,
                                           e_of.data_ptr() if (stats is not None and e_of is not None) else None,
                                           stats.data_ptr() if stats is not None else None, float(w_raw), float(w_of), float(BIG),
                                           keep.data_ptr() if cap else None, mask.data_ptr() if cap else None, n.data_ptr(), cap, slot0,
                                           rects.data_ptr(), int(n_host), boxes.data_ptr() if boxes is not None else None, out.shape[0],
                                           out.shape[1], out.data_ptr(), int(bool(first)),
                                           torch.cuda.current_stream(out.device).cuda_stream), 'vv_stream_zpaint')


def stream_smooth(ring, win, kt, ks, Bsum, bcnt, out, partial):
    """``vv_stream_smooth``: the trailing-window mean of the issued frame's mask.  ring float64 ``[K,h,w]`` (a ``stream_paint`` mask
    per slot), win int32 ``[1+kt]`` on the device (the number of frames of the window, then their ring slots in ascending frame order,
    the issued frame last), Bsum float64 ``[K,h,w]`` and bcnt int16 ``[K,h,w]`` (16-bit counts; the X/Y sums of every slot, kept from
    frame to frame: only the issued frame's are formed), out float64 ``[h,w]`` and partial float64 ``[ceil(h*w/256)]``, written in
    place: the smoothed mask and one maximum per 256 pixels, whose maximum is the smoothed frame score."""
    _dev('ring', ring, torch.float64), _dev('win', win, torch.int32, 1 + int(kt))
    if ring.dim() != 3:
        raise ValueError('ring must be a [K,h,w] tensor')
    K, h, w = ring.shape
    _dev('Bsum', Bsum, torch.float64, K * h * w), _dev('bcnt', bcnt, torch.int16, K * h * w), _dev('out', out, torch.float64, h * w)
    _dev('partial', partial, torch.float64, (h * w + 255) // 256)
    _lib.check(_lib.lib().vv_stream_smooth(ring.data_ptr(), K, h, w, win.data_ptr(), int(kt), int(ks), Bsum.data_ptr(), bcnt.data_ptr(),
                                           out.data_ptr(), partial.data_ptr(), torch.cuda.current_stream(ring.device).cuda_stream),
               'vv_stream_smooth')


TRACK_STAGE = 256      # detections ``vv_stream_tracks`` stages in LDS per pass (VV_STREAM_TRACK_STAGE)
MAX_TRACKS = 1024      # VV_STREAM_MAX_TRACKS: the largest table of ``vv_stream_tracks``
TRACK_WINDOW = 32      # VV_STREAM_TRACK_WINDOW: the longest score history of a track


def stream_tracks(t_meta, t_hist, next_id, scores, n, n_host, rects, boxes, h, w, reset, iou_pct, max_age, min_hits, box_track,
                  box_track_score, frame_track_score, counts):
    """``vv_stream_tracks``: the boxes of one issued frame linked to the tracks of the frames before (include/vecvad_hip.h states the
    steps).  The state is the caller's, on the device, and is updated in place: t_meta int32 ``[max_tracks,8]`` rows ``(id, age, hits,
    y0, y1, x0, x1, 0)``, t_hist float64 ``[max_tracks,window]``, next_id int32 ``[1]`` (started at 1).  scores, n, n_host, rects and
    boxes as for ``stream_paint`` (rects is only read); ``h x w``: the mask the rectangles lie in; ``reset``: the first frame of a
    video.  Written in place below ``n[0]``: box_track int32 ``[width,2]`` rows ``(id, hits)`` and box_track_score float64 ``[width]``
    (the mean of the track's last ``min(hits, window)`` scores; ``-BIG`` for id 0); frame_track_score float64 ``[1]``, the largest of
    them over tracks with ``hits >= min_hits``; counts int32 ``[3] = (live, dropped, next_id)``."""
    _dev('t_meta', t_meta, torch.int32), _dev('t_hist', t_hist, torch.float64), _dev('scores', scores, torch.float64)
    if t_meta.dim() != 2 or t_meta.shape[1] != 8 or t_hist.dim() != 2 or t_hist.shape[0] != t_meta.shape[0] or scores.dim() != 2:
        raise ValueError('t_meta must be a [max_tracks,8], t_hist a [max_tracks,window] and scores a [rows,width] tensor')
    rows, width = scores.shape
    _dev('next_id', next_id, torch.int32, 1), _dev('n', n, torch.int32, 1), _dev('rects', rects, torch.int32, 4 * width)
    _dev('box_track', box_track, torch.int32, 2 * width), _dev('box_track_score', box_track_score, torch.float64, width)
    _dev('frame_track_score', frame_track_score, torch.float64, 1), _dev('counts', counts, torch.int32, 3)
    if boxes is not None:
        _dev('boxes', boxes, torch.int32, 4 * width)
    _lib.check(_lib.lib().vv_stream_tracks(t_meta.data_ptr(), t_hist.data_ptr(), next_id.data_ptr(), t_meta.shape[0], scores.data_ptr(), rows,
                                           width, n.data_ptr(), int(n_host), rects.data_ptr(),
                                           boxes.data_ptr() if boxes is not None else None, int(h), int(w), int(bool(reset)), int(iou_pct),
                                           int(max_age), t_hist.shape[1], int(min_hits), float(BIG), box_track.data_ptr(),
                                           box_track_score.data_ptr(), frame_track_score.data_ptr(), counts.data_ptr(),
                                           torch.cuda.current_stream(t_meta.device).cuda_stream), 'vv_stream_tracks')


TRACK_KEYS = (('track_iou_percent', 30, 1, 100), ('track_max_age', 5, 0, 2 ** 31 - 2), ('track_window', 8, 1, TRACK_WINDOW),
              ('track_min_hits', 3, 1, 2 ** 31 - 1), ('stream_max_tracks', 128, 1, MAX_TRACKS))      # key, default, smallest, largest


def check_track_settings(c, tracks):
    """The switch of the tracks of a stream and their settings, checked on the host whatever the switch says: ``(tracks, iou_percent,
    max_age, window, min_hits, max_tracks)``.  ``tracks`` None reads ``stream_tracks``.  One-line ``ValueError`` for a setting that
    is no integer of its range."""
    out = [bool(c.get('stream_tracks', False) if tracks is None else tracks)]
    for key, default, lo, hi in TRACK_KEYS:
        v = c.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError('[mi355x] {} must be an integer in {}..{}, got {!r}'.format(key, lo, hi, v))
        out.append(int(v))
    return tuple(out)


def check_pixel_settings(c, masks, smooth, render, frame_hw, grid_hw):
    """The switches of the pixel-level stages of a stream and what they need, checked on the host: ``(masks, smooth, render, kt, ks,
    source, boxes, lo, hi, alpha)``.  ``smooth`` and ``render`` imply the mask.  One-line ``ValueError``: windows outside 1..33 (an
    even ``smooth_pixels``), ``render_source = smooth`` without the smoothing, ``render_range = auto`` (it needs the whole run) and
    frames that are not of the dataset's nominal size (the mask's)."""
    smooth = bool(c.get('stream_smooth', False) if smooth is None else smooth)
    render = bool(c.get('stream_render', False) if render is None else render)
    masks = bool(c.get('stream_masks', False) if masks is None else masks) or smooth or render
    kt, ks = c.get('smooth_frames', 5), c.get('smooth_pixels', 9)
    if smooth:
        if isinstance(kt, bool) or int(kt) != kt or not 1 <= kt <= SMOOTH_MAX:
            raise ValueError('[mi355x] smooth_frames must be an integer in 1..{} for a stream, got {!r}'.format(SMOOTH_MAX, kt))
        if isinstance(ks, bool) or int(ks) != ks or not 1 <= ks <= SMOOTH_MAX or ks % 2 == 0:
            raise ValueError('[mi355x] smooth_pixels must be an odd integer in 1..{}, got {!r}'.format(SMOOTH_MAX, ks))
    source, lo, hi, alpha = c.get('render_source', 'score'), 0.0, 1.0, 0
    if render:
        if source not in ('score', 'smooth'):
            raise ValueError("[mi355x] render_source must be 'score' or 'smooth', got {!r}".format(source))
        if source == 'smooth' and not smooth:
            raise ValueError('[mi355x] render_source = smooth needs stream_smooth = True: only that stage forms the smoothed mask of a stream')
        rng = c.get('render_range', 'auto')
        if isinstance(rng, str):
            raise ValueError('[mi355x] render_range = {} needs the scores of the whole run; a stream takes two numbers lo,hi'.format(rng))
        lo, hi = float(rng[0]), float(rng[1])
        if not lo < hi:
            raise ValueError('[mi355x] render_range must have lo < hi, got {!r}'.format(rng))
        if tuple(frame_hw) != tuple(grid_hw):
            raise ValueError('stream_render draws the {}x{} score mask over the frame: {}x{} frames are refused'.format(
                grid_hw[0], grid_hw[1], frame_hw[0], frame_hw[1]))
        alpha = (256 * int(c.get('render_alpha', 50)) + 50) // 100          # as test.py's render stage reads the percent
    return masks, smooth, render, int(kt), int(ks), source, bool(c.get('render_boxes', True)), lo, hi, alpha


class StreamResult:
    """The scores of one frame, on their way to the host.  ``frame``: the running index of the frame (pushes are counted from 0 across
    videos).  ``wait()`` blocks until the frame's copy has landed and returns ``(score, box_scores, kept)``: the frame score (float64;
    ``-BIG`` when no box was kept), the score of every box (float64 ``[n]``: the largest over the blocks the box belongs to, ``+BIG`` in
    a block without a model, ``-BIG`` for a box that was not kept or paints no pixel) and the motion test's flags (bool ``[n]``).
    After ``wait()``: ``boxes``, float64 ``[n,4]``, the boxes the three refer to, and ``dropped``, an int.  With given boxes these are
    the pushed boxes and 0 (set from the start).  With ``boxes='motion'`` the host learns ``n`` only here: the appearance boxes of the
    push first, then the motion boxes that were found, and the number of motion boxes that found no free slot.

    With the scorer's pixel-level switches, also after ``wait()`` (None for a switch that is off): ``mask``, float64 ``[gh,gw]``, the
    frame's score mask as ``test.paint_frame`` paints it from ``box_scores`` and ``boxes`` (its maximum is the frame score);
    ``smooth_mask`` and ``smooth_score``, its trailing-window mean and that mean's maximum; ``picture``, uint8 ``[H,W,3]`` RGB.

    With the scorer's ``tracks``, also after ``wait()`` (all None with the switch off): ``track_ids`` and ``track_hits``, int32 ``[n]``,
    the identity of every box's track (0: the box is no detection -- it scored ``-BIG`` or paints no pixel -- or found no free slot)
    and the frames that track was matched in; ``track_scores``, float64 ``[n]``, the mean of the track's last ``track_window`` scores
    (``-BIG`` for id 0); ``track_score``, their maximum over tracks with ``track_min_hits`` matches or more (``-BIG`` without one);
    ``tracks_dropped``, the detections that found no free slot; ``tracks``, int32 ``[L,7]``, the live slots of the table in slot
    order as ``(id, age, hits, y0, y1, x0, x1)``.

    With the scorer's ``maps``, also after ``wait()`` (both None with the switch off): ``error_mask``, float64 ``[gh,gw]``, the
    frame's per-pixel error mask -- inside the rectangle of every box that counts the box's map of z-scores, ``-BIG`` elsewhere (its
    support is that of ``mask``) -- and ``fine_score``, a float, exactly ``error_mask.max()``."""

    def __init__(self, frame, n, rows, width, host, host_keep, event, boxes, host_found=None, pixels=None, tracks=None):
        self.frame, self._n, self._rows, self._width = frame, n, rows, width
        self._host, self._host_keep, self._event = host, host_keep, event
        self._given, self._host_found = np.asarray(boxes, np.float64).reshape(-1, 4), host_found      # host_found: n, dropped, boxes_out
        self.boxes, self.dropped = (self._given, 0) if host_found is None else (None, None)
        self._pixels = pixels or {}          # name -> pooled pinned buffer, held until wait() has copied it out
        self.mask = self.smooth_mask = self.smooth_score = self.picture = self.error_mask = self.fine_score = None
        self._tracks = tracks                # (pinned copy of the scorer's track buffer, max_tracks, width) | None
        self.track_ids = self.track_hits = self.track_scores = self.track_score = self.tracks_dropped = self.tracks = None

    def _copy_tracks(self, n):
        """The track outputs out of the frame's copy of the track buffer (``StreamScorer._init_tracks`` has the layout)."""
        host, mt, width = self._tracks
        a, o = host.numpy(), 8 * mt
        meta = a[:o].reshape(mt, 8)
        self.tracks = meta[meta[:, 0] > 0][:, :7].copy()
        self.tracks_dropped = int(a[o + 1])
        self.track_score = float(a[o + 4:o + 6].view(np.float64)[0])
        self.track_scores = a[o + 6:o + 6 + 2 * width].view(np.float64)[:n].copy()
        pairs = a[o + 6 + 2 * width:o + 6 + 4 * width].reshape(width, 2)[:n]
        self.track_ids, self.track_hits = pairs[:, 0].copy(), pairs[:, 1].copy()

    def _copy_out(self):
        """The pixel-level results out of their pooled pinned buffers, which go back to the pool."""
        px, self._pixels = self._pixels, {}
        for name, it in px.items():
            a = it[0].numpy()
            if name == 'partial':             # one maximum per workgroup; a maximum does not round
                self.smooth_score = float(a.max()) if a.size else -float(BIG)
            else:
                setattr(self, name, a.copy())
                if name == 'error_mask':      # a maximum does not round
                    self.fine_score = float(self.error_mask.max())
            it[1] = None

    def __del__(self):                        # a result that was never waited for gives its buffers back once its copies have landed
        for it in self._pixels.values():
            it[1] = self._event

    def wait(self):
        self._event.synchronize()
        self._copy_out()
        a = self._host.numpy()
        if self._host_found is not None:
            f = self._host_found.numpy()
            self._n, self.dropped = int(f[0]), int(f[1])
            self.boxes = np.concatenate([self._given, f[2:].reshape(-1, 4)[len(self._given):self._n].astype(np.float64)])
        n = self._n
        if self._tracks is not None:
            self._copy_tracks(n)
        box = np.full(n, -float(BIG), np.float64)
        if self._rows and n:
            box = a[1:].reshape(self._rows, self._width)[:, :n].max(axis=0)
        return float(a[0]), box.copy(), self._host_keep.numpy()[:n].astype(bool)


class StreamScorer(StreamFront):
    """``StreamScorer(c, net_set, stats_raw, stats_of, frame_shape, flownet2=None, scene=None, max_boxes=None, device='cuda', boxes=None,
    masks=None, smooth=None, render=None, tracks=None, maps=None)``.

    ``c``: the dict of ``train.read_config``; ``net_set`` / ``stats_raw`` / ``stats_of``: what ``test.load_artifacts`` returns;
    ``frame_shape``: ``(H, W, C)`` of the uint8 frames that will be pushed (C = 1 or 3); ``flownet2``: the network (None loads
    ``[mi355x] flownet2_checkpoint``, in fp16 mode with ``direct_flow_fp16``); ``scene``: ShanghaiTech's per-scene model set, 0-based
    like ``foreground.block_groups``, None for the other datasets; ``max_boxes``: cubes per scoring launch (None: ``[mi355x]
    stream_max_boxes``).  ``useFlow``, ``context_of_num`` 0 and 4, ``w_raw`` / ``w_of``, ``motionThr``, ``precision`` and the ``h_block x
    w_block`` grid are honoured as ``test.py`` honours them; like there, the grid cells and the painted-rectangle test are those of the
    dataset's nominal frame size (``vad_datasets.frame_size``).

    ``boxes``: ``'given'`` (the caller hands every frame's boxes to ``push``) or ``'motion'`` (the scorer finds the motion boxes on the
    device; the dataset must have ``motion.CONSTANTS`` and the frames must not be larger than its nominal frame, else a one-line
    ``ValueError``); None reads ``[mi355x] stream_boxes``.

    ``push(frame_u8 [H,W,C], boxes float [n,>=4])`` -> a list with 0 or 1 ``StreamResult`` (the previous frame of the video);
    ``end_video()`` -> a list with the video's last frame, and the rings start over.  Neither synchronises the host with the device.
    With ``boxes='motion'``: ``push(frame_u8, ap_boxes=None)``, where ``ap_boxes`` float ``[k,>=4]`` are the frame's detector boxes (the
    rows ``bboxes_<mode>_obj_det.npy`` would hold for it), at most ``max_boxes`` of them.  They take slots ``0..k-1`` and are erased
    from the motion mask, truncated to integers as ``motion._ap_table`` does; the motion boxes follow.  A frame is one round there: motion
    boxes that find no free slot are dropped in ``vv_mask_boxes``' emission order and counted in ``StreamResult.dropped``.

    ``masks`` / ``smooth`` / ``render`` (None reads ``[mi355x] stream_masks`` / ``stream_smooth`` / ``stream_render``; all off by
    default, and then nothing below is allocated or launched): the frame's score mask, its trailing-window mean over the last
    ``smooth_frames`` frames of the video and ``smooth_pixels`` pixels, and its picture (``render_source``, ``render_range`` -- two
    numbers; ``auto`` is refused --, ``render_alpha``, ``render_boxes``), formed behind the frame's last ``vv_stream_scores`` and
    delivered with the scores (``StreamResult.mask`` / ``.smooth_mask`` / ``.smooth_score`` / ``.picture``).  ``smooth`` and ``render``
    imply the mask; a picture needs frames of the dataset's nominal size.  Every refusal is a one-line ``ValueError`` before any GPU
    work.

    ``tracks`` (None reads ``[mi355x] stream_tracks``; off by default, and then nothing of it is allocated, launched or copied): one
    more launch behind the frame's last ``vv_stream_scores``, ``vv_stream_tracks``, links the frame's boxes to the tracks of the
    video's earlier frames by IoU (``track_iou_percent``; greedy, best pair first), in a table of ``stream_max_tracks`` slots that
    lives on the device and is emptied at the first frame of a video.  A track that finds no box coasts for ``track_max_age`` frames;
    its score is the mean of its last ``track_window`` box scores, and the frame's track score the largest over tracks seen
    ``track_min_hits`` times or more (``StreamResult.track_ids`` / ``.track_hits`` / ``.track_scores`` / ``.track_score`` /
    ``.tracks_dropped`` / ``.tracks``).  The box scores are those of the frame's score mask: a box that paints no pixel of the
    nominal frame or scored ``-BIG`` has no track.  Needs no mask: with ``masks`` off nothing of the mask ring exists.

    ``maps`` (None reads ``[mi355x] stream_maps``; off by default, and then nothing of it is allocated, launched or copied): every
    scoring launch also stores its reconstructions (the ``'eval_maps'`` graph of ``FusedTrainer``, warmed and captured here, so that a
    ``push`` only replays), and one ``vv_stream_zpaint`` per scored block and round paints the per-pixel errors of the boxes that count
    into the frame's error mask (``StreamResult.error_mask`` / ``.fine_score``).  Score, box scores and keep flags keep their bits."""

    def __init__(self, c, net_set, stats_raw, stats_of, frame_shape, flownet2=None, scene=None, max_boxes=None, device='cuda',
                 boxes=None, masks=None, smooth=None, render=None, tracks=None, maps=None):
        self.cap = check_max_boxes(c.get('stream_max_boxes', 64) if max_boxes is None else max_boxes)      # before any GPU work
        self.motion = check_stream_boxes(c.get('stream_boxes', 'given') if boxes is None else boxes) == 'motion'
        self._refuse(c, frame_shape)
        from vad_datasets import frame_size
        cp, ds, method = c['cp'], c['dataset_name'], c['method']
        (self.masks, self.smooth, self.render, self.kt, self.ks, self.render_source, self.render_boxes, self.render_lo, self.render_hi,
         self.render_alpha) = check_pixel_settings(c, masks, smooth, render, (self.H, self.W), frame_size[ds][:2])      # before any GPU work
        self.tracks, self.trk_iou, self.trk_age, self.trk_window, self.trk_hits, self.trk_max = check_track_settings(c, tracks)
        self.maps = bool(c.get('stream_maps', False) if maps is None else maps)
        self.tail = self.masks or self.tracks or self.maps      # the stages that read the descriptor's tail
        super().__init__(c, RingSchedule(cp.getint(method, 'context_frame_num'), cp.getint(method, 'context_of_num'), motion=self.motion,
                                         mask_frames=self.kt if self.smooth else 1), flownet2, device)
        self._block_table(c, net_set, stats_raw, stats_of, scene)
        dev = self.device
        if self.tail:
            self._init_tail()
        if self.masks:
            self._init_pixels()
        if self.tracks:
            self._init_tracks()
        if self.maps:                         # the frame's error mask: every block's vv_stream_zpaint of every round accumulates into it
            self.zmask = torch.empty((self.grid_h, self.grid_w), dtype=torch.float64, device=dev)
            self.zfirst = True                # the frame being issued has had no vv_stream_zpaint launch yet
        self.held = None          # (boxes, crops, blocks, appearance table | None) of the frame that waits for its look-ahead
        self.frames = 0           # frames pushed so far, across videos
        self._warm_blocks(self.maps)

    def _init_tail(self):
        """Behind the descriptor, for the stages that read the frame's box count and rectangles (pixels, tracks, maps): the tail ``n, 3 unused |
        window [1 + K], padded to 4 words | rects [width][4]``."""
        dev, K = self.device, self.sched.K
        self.t_win = 4
        self.t_rects = self.t_win + (1 + K + 3) // 4 * 4
        if self.motion:                       # one round: the tail has its place behind the descriptor for good
            self.t_base = (self.words_motion + 3) // 4 * 4
            self.desc = torch.zeros(self.t_base + self.t_rects + 4 * self.cap, dtype=torch.int32, device=dev)
        else:                                 # room for one round and its tail from the start; more rounds grow it as before
            self.desc = torch.zeros((self.lay.words(1) + 3) // 4 * 4 + self.t_rects + 4 * self.cap, dtype=torch.int32, device=dev)

    def _init_pixels(self):
        """The device state of the pixel-level stages, allocated once: the mask ring (``smooth_frames`` slots, 1 without smoothing),
        the X/Y sums and counts of every slot, the smoothed mask and its partial maxima, the picture, the colour table and the table of
        box maxima (it grows with the rounds of a frame)."""
        from .render import colormap
        dev, gh, gw, K = self.device, self.grid_h, self.grid_w, self.sched.K
        self.mask_ring = torch.full((K, gh, gw), -float(BIG), dtype=torch.float64, device=dev)
        self.box_max = torch.zeros(self.cap, dtype=torch.float64, device=dev)
        self.frame_off = torch.zeros(2, dtype=torch.int32, device=dev)
        if self.smooth:
            self.Bsum = torch.zeros((K, gh, gw), dtype=torch.float64, device=dev)
            self.bcnt = torch.zeros((K, gh, gw), dtype=torch.int16, device=dev)
            self.S = torch.empty((gh, gw), dtype=torch.float64, device=dev)
            self.partial = torch.empty(int(_lib.lib().vv_stream_smooth_partials(gh, gw)), dtype=torch.float64, device=dev)
        if self.render:
            self.picture = torch.empty((self.H, self.W, 3), dtype=torch.uint8, device=dev)
            self.lut = torch.from_numpy(colormap()).to(dev)

    def _init_tracks(self):
        """The track table of the camera, on the device for good: the history, the id counter and ONE int32 buffer that holds what a
        frame's read-back wants, so that it is one copy: ``t_meta [max_tracks][8] | counts [3], 1 unused | frame track score (float64)
        | box track scores (float64) [width] | box (id, hits) [width][2]``.  It grows with the rounds of a frame."""
        dev, mt = self.device, self.trk_max
        self.t_hist = torch.zeros((mt, self.trk_window), dtype=torch.float64, device=dev)
        self.next_id = torch.ones(1, dtype=torch.int32, device=dev)
        self.trk = torch.zeros(8 * mt + 6 + 4 * self.cap, dtype=torch.int32, device=dev)

    def _tracks(self, issue, tail, scores, n_dev, n_host, boxes_dev):
        """``vv_stream_tracks`` behind a frame's last ``vv_stream_scores``, on the current stream; the arguments of ``_pixels``.
        Returns the part of the track buffer the frame's read-back copies."""
        width, o = scores.shape[1], 8 * self.trk_max
        used = o + 6 + 4 * width
        if self.trk.numel() < used:
            grown = torch.zeros(used, dtype=torch.int32, device=self.device)
            grown[:o].copy_(self.trk[:o])
            self.trk = grown
        t = self.trk
        stream_tracks(t[:o].view(self.trk_max, 8), self.t_hist, self.next_id, scores, n_dev, n_host,
                      tail[self.t_rects:self.t_rects + 4 * max(width, 1)], boxes_dev, self.grid_h, self.grid_w, issue['reset'], self.trk_iou,
                      self.trk_age, self.trk_hits, t[o + 6 + 2 * width:used].view(width, 2), t[o + 6:o + 6 + 2 * width].view(torch.float64),
                      t[o + 4:o + 6].view(torch.float64), t[o:o + 4])
        return t[:used]

    def _fill_tail(self, d, issue, n, boxes):
        """The tail of the descriptor on the host: the total number of boxes, the trailing window and the host's rectangles."""
        from .scoring import box_rects
        d[0] = n
        d[self.t_win] = len(issue['mask_slots'])
        d[self.t_win + 1:self.t_win + 1 + len(issue['mask_slots'])] = issue['mask_slots']
        d[self.t_rects:self.t_rects + 4 * len(boxes)] = box_rects(boxes, self.grid_h, self.grid_w).reshape(-1)

    def _pixels(self, issue, tail, scores, n_dev, n_host, boxes_dev):
        """The launches of the pixel-level stages behind a frame's last ``vv_stream_scores`` and their copies to pooled pinned buffers,
        all on the current stream: the caller's event behind them covers them.  tail: the descriptor's tail on the device; scores:
        the ``[rows,width]`` box-score rows; n_dev: the frame's box count on the device; ``n_host`` rectangles are the host's, the
        others the kernel resolves from ``boxes_dev``."""
        width = scores.shape[1]
        if self.box_max.numel() < width:
            self.box_max = torch.zeros(width, dtype=torch.float64, device=self.device)
        rects = tail[self.t_rects:self.t_rects + 4 * max(width, 1)]
        mask = self.mask_ring[issue['mask_slot']]
        stream_paint(scores, n_dev, n_host, rects, boxes_dev, mask, self.box_max, self.frame_off)
        out = {'mask': mask}
        if self.smooth:
            stream_smooth(self.mask_ring, tail[self.t_win:self.t_win + 1 + self.sched.K], self.kt, self.ks, self.Bsum, self.bcnt, self.S,
                          self.partial)
            out['smooth_mask'], out['partial'] = self.S, self.partial
        if self.render:
            shown = self.S if self.render_source == 'smooth' else mask
            draw = self.render_boxes and width > 0
            _lib.check(_lib.lib().vv_render_overlay(
                self.raw_ring[issue['raw_slots'][-1]].data_ptr(), self.C, 1, shown.data_ptr(), None, rects.data_ptr() if draw else None,
                self.box_max.data_ptr() if draw else None, self.frame_off.data_ptr() if draw else None, width if draw else 0,
                self.lut.data_ptr(), self.render_lo, self.render_hi, self.render_alpha, 1, self.H, self.W, self.picture.data_ptr(),
                torch.cuda.current_stream(self.device).cuda_stream), 'vv_render_overlay')
            out['picture'] = self.picture
        held = {}
        for name, t in out.items():
            held[name] = self.staging.hold(name, t.shape, t.dtype)
            held[name][0].copy_(t, non_blocking=True)
        return held

    @classmethod
    def from_config(cls, config_path='config.cfg', frame_shape=None, flownet2=None, scene=None):
        """The scorer of a configuration: the artifacts ``train.py`` wrote under ``<data_root_dir>/<modality>/`` are loaded as ``test.py``
        loads them.  ``frame_shape`` None: the dataset's nominal frame size with 3 channels.  A bad ``stream_max_boxes`` raises before
        any GPU work."""
        c, net_set, st_r, st_o, frame_shape, device = cls.load(config_path, frame_shape)
        return cls(c, net_set, st_r, st_o, frame_shape, flownet2=flownet2, scene=scene, device=device)

    def push(self, frame_u8, boxes=None, ap_boxes=None):
        issue, held = self._take(frame_u8, boxes, ap_boxes)
        out = [self._issue(issue, self.held)] if issue is not None else []
        self.held = held
        self.frames += 1
        return out

    def end_video(self):
        held, self.held = self.held, None
        issue = self.sched.end_video()
        return [self._issue(issue, held)] if issue is not None else []

    def _score_block(self, cell, keep, n, masks, box_scores, frame_score, zp=None):
        """One block's share of a round: its model scores the whole store in its own fixed-size launch (no launch for a block without a
        model), ``vv_stream_scores`` reduces under ``keep`` and the block's mask row.  With ``maps`` the launch is the one that stores
        the reconstructions (same sums), and ``vv_stream_zpaint`` paints its per-pixel errors into the frame's error mask behind it;
        ``zp = (slot0, rects, n_host, boxes_dev)``: the round's first row of the frame's rectangle table and who resolves which row."""
        hh, ww = cell
        ent = self.blocks[cell]
        raw = of = stats = e_raw = e_of = None
        if ent is not None:
            raw, of, *maps = ent[0].score_cubes(self.store_raw, self.store_flow, self.idx, maps=self.maps)
            if self.maps:
                e_raw, e_of = maps[0], (maps[1] if self.use_flow else None)
            raw = raw.to(torch.float32).contiguous()
            of = of.to(torch.float32).contiguous() if (of is not None and self.use_flow) else None
            stats = ent[1]
        m0 = (hh * self.wb + ww) * self.cap
        stream_scores(raw, of, stats, self.w_raw, self.w_of, keep, n, masks[m0:m0 + self.cap], box_scores, frame_score)
        if self.maps:
            slot0, rects, n_host, boxes_dev = zp
            stream_zpaint(e_raw, e_of, stats, self.w_raw, self.w_of, keep, masks[m0:m0 + self.cap], n, slot0, rects, n_host, boxes_dev,
                          self.zmask, self.zfirst)
            self.zfirst = False

    def _maps_out(self, n_dev, rects):
        """The frame's error mask on its way to a pooled pinned buffer, on the current stream (the caller's event behind it covers the
        copy).  A frame that had no ``vv_stream_zpaint`` launch -- no box, or no block with a box -- gets its one background launch."""
        if self.zfirst:
            none = self.idx[:0].to(torch.uint8)
            stream_zpaint(None, None, None, self.w_raw, self.w_of, none, none, n_dev, 0, rects, 0, None, self.zmask, True)
        self.zfirst = True                    # for the next frame
        it = self.staging.hold('error_mask', self.zmask.shape, self.zmask.dtype)
        it[0].copy_(self.zmask, non_blocking=True)
        return {'error_mask': it}

    def _read_back(self, *tensors):
        """Non-blocking copies to fresh pinned memory and the event behind them."""
        hosts = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in tensors]
        for h, t in zip(hosts, tensors):
            h.copy_(t, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return hosts, event

    def _issue(self, issue, held):
        if self.motion:
            return self._issue_motion(issue, held)
        boxes, crops, blocks, _ = held
        cap, lay = self.cap, self.lay
        n = len(crops)
        rounds = (n + cap - 1) // cap
        width = rounds * cap
        words = lay.words(rounds)
        t_base = (words + 3) // 4 * 4                                          # the tail of the pixel-level stages, 16-byte aligned
        if self.tail:
            words = t_base + self.t_rects + 4 * max(width, 1)
        st, d, _, rows, used = self._describe([(0, issue, crops, blocks)], words - lay.words(rounds))  # rows: the blocks of the frame's boxes
        if self.tail:
            self._fill_tail(d[t_base:], issue, n, boxes)
        desc = self._start(st)
        out = torch.full((1 + len(rows) * width,), -float(BIG), dtype=torch.float64, device=self.device)
        keep = torch.zeros(max(width, 1), dtype=torch.uint8, device=self.device)
        tail = desc[t_base:words] if self.tail else None
        zrects = tail[self.t_rects:self.t_rects + 4 * max(width, 1)] if self.maps else None
        for r in range(rounds):
            rnd, n_dev, masks = self._round(desc, r)
            k = keep[r * cap:(r + 1) * cap]
            self._cut(rnd, n_dev, k)
            for i in used[r]:
                self._score_block(rows[i], k, n_dev, masks, out[1 + i * width + r * cap:1 + i * width + (r + 1) * cap], out[0:1],
                                  (r * cap, zrects, n, None))
        pixels, trk = None, []
        if self.tail:
            if self.tracks:
                trk = [self._tracks(issue, tail, out[1:].view(len(rows), width), tail[0:1], n, None)]
            if self.masks:
                pixels = self._pixels(issue, tail, out[1:].view(len(rows), width), tail[0:1], n, None)
            if self.maps:
                pixels = dict(pixels or {}, **self._maps_out(tail[0:1], zrects))
        (host, host_keep, *host_trk), event = self._read_back(out, keep, *trk)
        return StreamResult(self.frames - 1, n, len(rows), width, host, host_keep, event, boxes, pixels=pixels,
                            tracks=(host_trk[0], self.trk_max, width) if host_trk else None)

    def _issue_motion(self, issue, held):
        """A frame whose motion boxes the device finds: ONE round, the appearance boxes in slots ``0..k-1`` as ``_issue`` files them, the
        motion boxes behind them by ``vv_stream_boxes``, and every block of the grid scored, since the host does not know where a motion
        box lands."""
        boxes, cap, k, found = held[0], self.cap, len(held[1]), self.found
        desc, rnd, n, masks = self._motion_front(issue, held)
        keep = torch.zeros(cap, dtype=torch.uint8, device=self.device)
        self._cut(rnd, n, keep)
        cells = [(hh, ww) for hh in range(self.hb) for ww in range(self.wb)]
        out = torch.full((1 + len(cells) * cap,), -float(BIG), dtype=torch.float64, device=self.device)
        zrects = desc[self.t_base + self.t_rects:self.t_base + self.t_rects + 4 * cap] if self.maps else None
        for i, cell in enumerate(cells):
            self._score_block(cell, keep, n, masks, out[1 + i * cap:1 + (i + 1) * cap], out[0:1], (0, zrects, k, found[2:]))
        pixels, trk = None, []
        if self.tracks:
            trk = [self._tracks(issue, desc[self.t_base:], out[1:].view(len(cells), cap), n, k, found[2:])]
        if self.masks:
            pixels = self._pixels(issue, desc[self.t_base:], out[1:].view(len(cells), cap), n, k, found[2:])
        if self.maps:
            pixels = dict(pixels or {}, **self._maps_out(n, zrects))
        (host, host_keep, host_found, *host_trk), event = self._read_back(out, keep, found, *trk)
        return StreamResult(self.frames - 1, None, len(cells), cap, host, host_keep, event, boxes, host_found, pixels=pixels,
                            tracks=(host_trk[0], self.trk_max, cap) if host_trk else None)
