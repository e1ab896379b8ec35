"""The front half of a stream, once: everything between ``push`` and the cubes of a frame's boxes in their store slots (``StreamFront``).

``vec_vad_amd.stream.StreamScorer`` (one camera, scores), ``vec_vad_amd.multistream.MultiStreamScorer`` (several cameras, scores) and
``vec_vad_amd.stream_train.StreamCollector`` (one camera, a training store) differ in what stands BEHIND ``vv_stream_cut``.  In front of
it they are one thing, and derive it from here:

  the refusals of a configuration and a frame shape, all before any GPU call;
  the geometry of the block grid, the device, FlowNet2's captured graph at ``cameras`` pairs per launch;
  the rings ``[cameras*R,...]`` / ``[cameras*Rf,...]`` and the stores ``[cameras*cap,...]`` (camera ``k`` owns slots ``k*R ..``,
    ``k*Rf ..`` and ``k*cap ..``; a single-camera class is ``cameras = 1``);
  the host side of a frame (``check_frame``, ``boxes_to_crops``, ``box_cells``) and its upload into a ring slot;
  ONE descriptor format (``TickLayout`` / ``tick_descriptor``), written straight into a pinned staging buffer (``fill_tick``), and the
    flow launches that read their tables from its header;
  the motion front (``vv_motion_mask`` -> ``vv_mask_boxes`` -> ``vv_stream_boxes``), whose tables lie behind the one round of a frame;
  the cut of a round (``vv_stream_cut_multi`` at ``cameras`` cameras).

The ring bookkeeping (``RingSchedule``, ``MultiSchedule``), the pinned staging pool and the wrappers of the three launches live here
too, as do the integer checks of the ``[mi355x]`` keys the three classes read.  This module imports none of the three.
"""
import os

import numpy as np
import torch

from . import _lib
from .extract import boxes_to_crops
from .scoring import box_paints


def ring_frames(context_frame_num):
    """Frames the raw ring holds: the ``context_frame_num + 1`` frames of the 'predict' window of the frame being issued, plus the
    frame pushed behind it (the second frame of its flow pair)."""
    return int(context_frame_num) + 2


def motion_ring_frames(context_frame_num):
    """Frames the raw ring holds when the scorer finds its own motion boxes: the motion window of the frame being issued is the frame
    before it, the frame and the look-ahead frame, so never fewer than 3."""
    return max(ring_frames(context_frame_num), 3)


def flow_ring_frames(context_of_num):
    """Flow fields the flow ring holds: the ``context_of_num + 1`` fields of the flow window of the frame being issued (its own field
    is computed when it is issued, into the slot of the field that left the window)."""
    return int(context_of_num) + 1


def check_count(key, v):
    """``[mi355x] <key>`` as an integer >= 1, else a one-line ``ValueError``; no GPU is touched."""
    if isinstance(v, str):
        try:
            v = int(v.strip())
        except ValueError:
            pass
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError('[mi355x] {} must be an integer >= 1, got {!r}'.format(key, v))
    return int(v)


def check_max_boxes(v):
    """``stream_max_boxes`` as an integer >= 1, else a one-line ``ValueError``; no GPU is touched."""
    return check_count('stream_max_boxes', v)


def check_cameras(v):
    """``stream_cameras`` as an integer >= 1, else a one-line ``ValueError``; no GPU is touched."""
    return check_count('stream_cameras', v)


def check_max_cubes(v):
    """``collect_max_cubes`` as an integer >= 1, else a one-line ``ValueError``; no GPU is touched."""
    return check_count('collect_max_cubes', v)


def check_stream_boxes(v):
    """``stream_boxes`` as ``'given'`` or ``'motion'``, else a one-line ``ValueError``; no GPU is touched."""
    w = v.strip().lower() if isinstance(v, str) else v
    if w not in ('given', 'motion'):
        raise ValueError("[mi355x] stream_boxes must be 'given' or 'motion', got {!r}".format(v))
    return w


def _dev(name, t, dtype, numel=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() < numel):
        raise ValueError('{} must be a contiguous CUDA {} tensor{}'.format(name, dtype, '' if numel is None else ' of at least %d elements' % numel))
    return t


def check_frame(frame_u8, boxes, H, W, C):
    """What ``push`` is handed, checked on the host: the frame as a uint8 ``[H,W,C]`` array (a ``[H,W]`` one passes for ``C`` = 1) and
    the first four columns of its boxes as float64 ``[n,4]``; a frame of another type or shape is a one-line ``ValueError``."""
    frame = np.asarray(frame_u8)
    if frame.ndim == 2 and C == 1:
        frame = frame[:, :, None]
    if frame.dtype != np.uint8 or tuple(frame.shape) != (H, W, C):
        raise ValueError('push takes uint8 frames of shape {}, got {} {}'.format((H, W, C), frame.dtype, tuple(frame.shape)))
    boxes = np.asarray(boxes, np.float64)
    boxes = boxes.reshape(-1, boxes.shape[-1])[:, :4] if boxes.ndim == 2 and boxes.shape[0] else np.zeros((0, 4), np.float64)
    return frame, boxes


def box_cells(boxes, grid_h, grid_w, hb, wb, h_step, w_step, block_mode, painted_only):
    """Per box ``(x1, y1, x2, y2)`` the sorted cells ``(h, w)`` of the ``hb x wb`` block grid it belongs to, each once: those of
    ``utils.calc_block_idx`` under ``block_mode``; pure.  ``painted_only`` is the test rule -- a box that paints no pixel of the
    ``grid_h x grid_w`` mask (``scoring.box_paints``) belongs to no cell; without it every box keeps its cells, the training rule.
    A box with a cell outside the grid is an ``IndexError`` under both."""
    from utils import calc_block_idx
    paints = box_paints(boxes, grid_h, grid_w) if painted_only else np.ones(len(boxes), bool)
    out = []
    for b, bb in enumerate(boxes):
        cells = calc_block_idx(bb[0], bb[2], bb[1], bb[3], h_step, w_step, mode=block_mode)
        if any(not (0 <= hi < hb and 0 <= wi < wb) for hi, wi in cells):
            raise IndexError('box {} falls outside the {}x{} block grid'.format(b, hb, wb))
        out.append(sorted(set(cells)) if paints[b] else [])
    return out


def stream_cut(raw_ring, flow_ring, n, crops, raw_win, flow_win, thr, raw_store, flow_store, keep, energy=None):
    """``vv_stream_cut``: the cubes of the ``n[0]`` boxes of one frame from the two rings into slots ``0..n-1`` of a fixed store, and the
    motion test.  raw_ring uint8 ``[R,H,W,C]``, flow_ring float32 ``[Rf,H,W,2]``; the tables are DEVICE tensors that the kernel reads
    (int32: ``n`` ``[1]``, ``crops`` ``[cap,4]`` as ``boxes_to_crops`` forms them, ``raw_win`` ``[T]`` and ``flow_win`` ``[Tf]`` ring
    slots), so nothing here looks at their values; raw_store uint8 ``[cap,T,P,P,C]``, flow_store float32 ``[cap,Tf,P,P,2]``, keep uint8
    ``[cap]``, energy float64 ``[cap]`` or None.  Written: slots below ``n[0]`` -- the bytes of ``extract.cube_cut`` and the values of
    ``extract.cube_energy`` for the same frames, crops and windows; everything else keeps what it holds."""
    _dev('raw_ring', raw_ring, torch.uint8), _dev('flow_ring', flow_ring, torch.float32)
    if raw_ring.dim() != 4 or flow_ring.dim() != 4 or tuple(flow_ring.shape[1:]) != tuple(raw_ring.shape[1:3]) + (2,):
        raise ValueError('the rings must be [R,H,W,C] frames and [Rf,H,W,2] flow fields of one frame size')
    R, H, W, C = raw_ring.shape
    _dev('raw_store', raw_store, torch.uint8), _dev('flow_store', flow_store, torch.float32)
    if raw_store.dim() != 5 or flow_store.dim() != 5:
        raise ValueError('the stores must be [cap,T,P,P,C] and [cap,Tf,P,P,2] tensors')
    cap, T, P = raw_store.shape[0], raw_store.shape[1], raw_store.shape[2]
    Tf = flow_store.shape[1]
    if tuple(raw_store.shape) != (cap, T, P, P, C) or tuple(flow_store.shape) != (cap, Tf, P, P, 2):
        raise ValueError('the stores must be [cap,T,P,P,%d] and [cap,Tf,P,P,2] tensors of one cap and P' % C)
    _dev('n', n, torch.int32, 1), _dev('crops', crops, torch.int32, 4 * cap)
    _dev('raw_win', raw_win, torch.int32, T), _dev('flow_win', flow_win, torch.int32, Tf), _dev('keep', keep, torch.uint8, cap)
    if energy is not None:
        _dev('energy', energy, torch.float64, cap)
    _lib.check(_lib.lib().vv_stream_cut(raw_ring.data_ptr(), R, flow_ring.data_ptr(), flow_ring.shape[0], H, W, C, n.data_ptr(),
                                        crops.data_ptr(), raw_win.data_ptr(), flow_win.data_ptr(), cap, T, Tf, P, float(thr),
                                        raw_store.data_ptr(), flow_store.data_ptr(), keep.data_ptr(),
                                        energy.data_ptr() if energy is not None else None,
                                        torch.cuda.current_stream(raw_ring.device).cuda_stream), 'vv_stream_cut')


def stream_cut_multi(raw_ring, flow_ring, cams, n, crops, raw_win, flow_win, thr, raw_store, flow_store, keep, energy=None):
    """``vv_stream_cut_multi``: ``stream_cut`` for ``cams`` cameras in one launch.  raw_ring uint8 ``[cams*R,H,W,C]``, flow_ring
    float32 ``[cams*Rf,H,W,2]``; DEVICE tables the kernel reads (int32: ``n`` ``[cams]``, ``crops`` ``[cams,cap,4]``, ``raw_win``
    ``[cams,T]`` and ``flow_win`` ``[cams,Tf]`` absolute ring slots), so nothing here looks at their values; raw_store uint8
    ``[cams*cap,T,P,P,C]``, flow_store float32 ``[cams*cap,Tf,P,P,2]``, keep uint8 ``[cams*cap]``, energy float64 ``[cams*cap]`` or None.
    Written: slots ``k*cap + b`` with ``b < n[k]`` -- what ``stream_cut`` writes for camera ``k`` alone; everything else keeps what it
    holds."""
    cams = int(cams)
    _dev('raw_ring', raw_ring, torch.uint8), _dev('flow_ring', flow_ring, torch.float32)
    if raw_ring.dim() != 4 or flow_ring.dim() != 4 or tuple(flow_ring.shape[1:]) != tuple(raw_ring.shape[1:3]) + (2,):
        raise ValueError('the rings must be [cams*R,H,W,C] frames and [cams*Rf,H,W,2] flow fields of one frame size')
    if cams < 1 or raw_ring.shape[0] % cams or flow_ring.shape[0] % cams:
        raise ValueError('cams must be at least 1 and divide the slots of both rings, got {}'.format(cams))
    _, H, W, C = raw_ring.shape
    R, Rf = raw_ring.shape[0] // cams, flow_ring.shape[0] // cams
    _dev('raw_store', raw_store, torch.uint8), _dev('flow_store', flow_store, torch.float32)
    if raw_store.dim() != 5 or flow_store.dim() != 5 or raw_store.shape[0] % cams:
        raise ValueError('the stores must be [cams*cap,T,P,P,C] and [cams*cap,Tf,P,P,2] tensors')
    slots, T, P = raw_store.shape[0], raw_store.shape[1], raw_store.shape[2]
    cap, Tf = slots // cams, flow_store.shape[1]
    if tuple(raw_store.shape) != (slots, T, P, P, C) or tuple(flow_store.shape) != (slots, Tf, P, P, 2):
        raise ValueError('the stores must be [cams*cap,T,P,P,%d] and [cams*cap,Tf,P,P,2] tensors of one cap and P' % C)
    _dev('n', n, torch.int32, cams), _dev('crops', crops, torch.int32, 4 * slots)
    _dev('raw_win', raw_win, torch.int32, cams * T), _dev('flow_win', flow_win, torch.int32, cams * Tf), _dev('keep', keep, torch.uint8, slots)
    if energy is not None:
        _dev('energy', energy, torch.float64, slots)
    _lib.check(_lib.lib().vv_stream_cut_multi(raw_ring.data_ptr(), R, flow_ring.data_ptr(), Rf, H, W, C, cams, n.data_ptr(),
                                              crops.data_ptr(), raw_win.data_ptr(), flow_win.data_ptr(), cap, T, Tf, P, float(thr),
                                              raw_store.data_ptr(), flow_store.data_ptr(), keep.data_ptr(),
                                              energy.data_ptr() if energy is not None else None,
                                              torch.cuda.current_stream(raw_ring.device).cuda_stream), 'vv_stream_cut_multi')


def stream_boxes(count, boxes, n_ap, H, W, grid_h, grid_w, hb, wb, h_step, w_step, block_mode, n, dropped, crops, masks, boxes_out):
    """``vv_stream_boxes``: what ``StreamScorer._prepare`` forms on the host, for motion boxes that exist only on the device.  count
    int32 ``[1]`` and boxes int32 ``[mcap,4]`` as ``vv_mask_boxes`` leaves them for one window; ``n_ap``: slots ``0..n_ap-1`` of the
    tables hold the host's appearance boxes and are not touched.  Written in place, all on the device: n int32 ``[1]`` = ``n_ap + m``
    with ``m = min(count, mcap, cap - n_ap)``; dropped int32 ``[1]`` = ``count - m``; crops int32 ``[cap,4]`` (``boxes_to_crops``) and
    boxes_out int32 ``[cap,4]`` in slots ``n_ap..n-1``; masks uint8 ``[hb*wb,cap]``: columns ``n_ap..cap-1`` get 1 in the cells of
    ``utils.calc_block_idx`` of a box that paints a pixel of the ``grid_h x grid_w`` mask (``scoring.box_paints``), else 0."""
    _dev('count', count, torch.int32, 1), _dev('boxes', boxes, torch.int32)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or crops.dim() != 2 or crops.shape[1] != 4:
        raise ValueError('boxes and crops must be [mcap,4] and [cap,4] tensors')
    cap = crops.shape[0]
    _dev('crops', crops, torch.int32), _dev('boxes_out', boxes_out, torch.int32, 4 * cap), _dev('n', n, torch.int32, 1)
    _dev('dropped', dropped, torch.int32, 1), _dev('masks', masks, torch.uint8, int(hb) * int(wb) * cap)
    _lib.check(_lib.lib().vv_stream_boxes(count.data_ptr(), boxes.data_ptr(), boxes.shape[0], int(n_ap), cap, int(H), int(W), int(grid_h),
                                          int(grid_w), int(hb), int(wb), float(h_step), float(w_step), int(block_mode), n.data_ptr(),
                                          dropped.data_ptr(), crops.data_ptr(), masks.data_ptr(), boxes_out.data_ptr(),
                                          torch.cuda.current_stream(crops.device).cuda_stream), 'vv_stream_boxes')


class RingSchedule:
    """The ring bookkeeping of one camera, pure (no GPU).  ``push()`` -> ``(slot, issue | None)``: the raw ring slot the new frame goes
    into, and the frame that can now be issued (the previous frame of the video).  ``end_video()`` -> the issue of the video's last
    frame (None for a video without frames; ``ValueError`` for a video of one frame), after which the next push starts a video.

    An issue is a dict with video-local frame numbers and ring slots: ``frame``; ``raw_frames`` / ``raw_slots`` (the raw window);
    ``flow_frames`` / ``flow_slots`` (the flow window); ``pair_frames`` / ``pair_slots`` (the two frames FlowNet2 sees for the flow of
    ``frame``) and ``flow_slot`` (where that flow is written before the window is read); ``motion_frames`` / ``motion_slots`` (the
    three-frame window of the motion stage, ``context_range(i, 'hard', 1)``: the frame between its two neighbours, itself in place of
    a neighbour the video does not have).  Frame ``k`` of a video lives in raw slot ``k % R``, its flow in flow slot ``k % Rf``.
    ``motion``: the raw ring holds ``motion_ring_frames`` frames, never fewer than the three of the motion window; without it the
    motion slots mean something only where ``ring_frames`` is 3 or more already.  ``mask_frames`` = K, the slots of the score-mask ring
    (the trailing smoothing window in frames; 1 without smoothing): ``mask_slot`` = ``frame % K`` is where the issued frame's mask
    goes, ``mask_frames`` / ``mask_slots`` the frames ``max(0, frame - K + 1) .. frame`` of the video and their slots, ascending.
    ``reset``: the issue is the first of its video (what a tracker frees its table for)."""

    def __init__(self, context_frame_num=4, context_of_num=0, motion=False, mask_frames=1):
        self.T, self.Tf, self.K = int(context_frame_num) + 1, int(context_of_num) + 1, int(mask_frames)
        self.R = motion_ring_frames(context_frame_num) if motion else ring_frames(context_frame_num)
        self.Rf = flow_ring_frames(context_of_num)
        self.count = 0            # frames of the current video pushed so far

    def _issue(self, t, last):
        raw = [max(t - self.T + 1 + i, 0) for i in range(self.T)]            # 'predict': up to and including t, first frame repeated
        flow = [max(t - self.Tf + 1 + i, 0) for i in range(self.Tf)]
        pair = (t - 1, t) if last else ((t, t) if t == 0 else (t, t + 1))     # calc_optical_flow.flow_pairs
        motion = (max(t - 1, 0), t, t if last else t + 1)                     # 'hard' at one frame of context: clipped to the video
        trail = list(range(max(0, t - self.K + 1), t + 1))                    # the trailing window of the mask smoothing
        return dict(frame=t, reset=t == 0, mask_slot=t % self.K, mask_frames=trail, mask_slots=[f % self.K for f in trail], raw_frames=raw, raw_slots=[f % self.R for f in raw], flow_frames=flow,
                    flow_slots=[f % self.Rf for f in flow], pair_frames=pair, pair_slots=(pair[0] % self.R, pair[1] % self.R),
                    flow_slot=t % self.Rf, motion_frames=motion, motion_slots=tuple(f % self.R for f in motion))

    def push(self):
        k = self.count
        self.count += 1
        return k % self.R, (self._issue(k - 1, False) if k >= 1 else None)

    def end_video(self):
        k, self.count = self.count, 0
        if k == 0:
            return None
        if k == 1:
            raise ValueError('a video that ends after one frame cannot be scored: the flow of a frame needs a second frame of its video')
        return self._issue(k - 1, True)


class MultiSchedule:
    """The ring bookkeeping of ``cameras`` cameras, pure (no GPU): ``cameras`` independent ``RingSchedule``s over shared rings.  An issue
    of camera ``k`` is the ``RingSchedule`` issue with ``camera = k`` and ABSOLUTE slots: its raw slots (``raw_slots``, ``pair_slots``,
    ``motion_slots``) offset by ``k*R``, its flow slots (``flow_slots``, ``flow_slot``) by ``k*Rf``.

    ``push(present)`` (a sequence of ``cameras`` flags) -> ``[(k, slot, issue | None)]`` for the cameras that got a frame, ascending:
    the absolute raw slot of the new frame and the frame that can now be issued.  ``end_video(cameras=None)`` -> ``[(k, issue)]`` for
    the named cameras (None: all) that hold a frame, ascending; a camera without frames is skipped.  A camera whose video has one
    frame raises the ``ValueError`` of ``RingSchedule.end_video`` BEFORE any camera's schedule is changed."""

    def __init__(self, cameras, context_frame_num=4, context_of_num=0):
        self.cameras = int(cameras)
        self.cams = [RingSchedule(context_frame_num, context_of_num) for _ in range(self.cameras)]
        one = self.cams[0]
        self.T, self.Tf, self.R, self.Rf = one.T, one.Tf, one.R, one.Rf

    def _absolute(self, k, issue):
        ro, fo = k * self.R, k * self.Rf
        out = dict(issue, camera=k, flow_slot=issue['flow_slot'] + fo)
        out['raw_slots'] = [s + ro for s in issue['raw_slots']]
        out['flow_slots'] = [s + fo for s in issue['flow_slots']]
        out['pair_slots'] = tuple(s + ro for s in issue['pair_slots'])
        out['motion_slots'] = tuple(s + ro for s in issue['motion_slots'])
        return out

    def push(self, present):
        if len(present) != self.cameras:
            raise ValueError('one flag per camera: {} for {} cameras'.format(len(present), self.cameras))
        out = []
        for k, here in enumerate(present):
            if here:
                slot, issue = self.cams[k].push()
                out.append((k, k * self.R + slot, self._absolute(k, issue) if issue is not None else None))
        return out

    def end_video(self, cameras=None):
        ks = sorted(set(range(self.cameras) if cameras is None else (int(k) for k in cameras)))
        if any(not 0 <= k < self.cameras for k in ks):
            raise ValueError('cameras must lie in 0..{}, got {!r}'.format(self.cameras - 1, list(cameras)))
        for k in ks:
            if self.cams[k].count == 1:
                raise ValueError('camera {}: a video that ends after one frame cannot be scored: the flow of a frame needs a second '
                                 'frame of its video'.format(k))
        out = []
        for k in ks:
            issue = self.cams[k].end_video()
            if issue is not None:
                out.append((k, self._absolute(k, issue)))
        return out


class TickLayout:
    """Where the parts of a tick's int32 descriptor lie, in words; pure.  Header ``rounds, cameras, 2 unused | pairs [cameras][2] | rows
    [cameras]``, padded to 4 words (``head``); then per round ``D`` words: ``n [cameras]``, padded to 4 | ``crops [cameras][cap][4]`` |
    ``raw_win [cameras][T]`` | ``flow_win [cameras][Tf]``, padded to 4 | ``masks [hb*wb][cameras*cap]`` bytes."""

    def __init__(self, cameras, cap, T, Tf, hb, wb):
        self.cameras, self.cap, self.T, self.Tf, self.hb, self.wb = (int(v) for v in (cameras, cap, T, Tf, hb, wb))
        cams = self.cameras
        self.h_pairs = 4
        self.h_rows = self.h_pairs + 2 * cams
        self.head = (self.h_rows + cams + 3) // 4 * 4
        self.w_crops = (cams + 3) // 4 * 4
        self.w_rwin = self.w_crops + 4 * cams * self.cap
        self.w_fwin = self.w_rwin + cams * self.T
        self.w_mask = (self.w_fwin + cams * self.Tf + 3) // 4 * 4
        self.D = self.w_mask + (self.hb * self.wb * cams * self.cap + 3) // 4

    def rounds(self, items):
        """The rounds of a tick of ``items`` (``tick_descriptor``): ``max ceil(n / cap)`` over the issuing cameras' box counts."""
        return max((len(it[2]) + self.cap - 1) // self.cap for it in items)

    def words(self, rounds):
        return self.head + max(int(rounds), 1) * self.D


def tick_descriptor(lay, items):
    """The descriptor of one tick, pure (no GPU).  ``items``: ``(camera, issue, crops, blocks)`` per issuing camera in ascending camera
    order -- the ``MultiSchedule`` issue, int32 ``[n,4]`` crops (``boxes_to_crops``) and per box the sorted list of grid cells
    ``(h, w)`` it belongs to (empty for a box that paints no pixel).  Returns ``(d, rounds, rows, used)``: the int32 words in the
    layout of ``TickLayout``; the rounds, ``lay.rounds(items)``; the sorted cells that any box belongs to; per round the indices into
    ``rows`` of the cells with a box of that round.  The words are those of ``fill_tick``, which ``StreamFront`` calls on its pinned
    staging buffer; this function checks the items and makes the array."""
    ks = [it[0] for it in items]
    if ks != sorted(set(ks)) or any(not 0 <= k < lay.cameras for k in ks) or not ks:
        raise ValueError('a tick takes one item per issuing camera, in ascending camera order, got cameras {!r}'.format(ks))
    rounds = lay.rounds(items)
    d = np.zeros(lay.words(rounds), np.int32)
    return (d, rounds) + fill_tick(lay, items, rounds, d)


def fill_tick(lay, items, rounds, d):
    """The words of ``tick_descriptor`` written into ``d``, a ZEROED int32 array of at least ``lay.words(rounds)`` words; ``items`` as
    there and taken as given, ``rounds`` = ``lay.rounds(items)``.  Returns ``(rows, used)``.

    The pair and row tables are ``calc_optical_flow.launch_tables(pair_slots, flow_slot, cameras)[0]`` of the issuing cameras: absolute
    ring slots, the tail repeating the last pair at row -1.  Box ``b`` of round ``r`` of camera ``k`` has its crop at ``crops[k][b]`` of
    that round and its mask bytes at ``masks[h*wb + w][k*cap + b]``; a camera that does not issue, or has no box left for a round, has
    ``n = 0`` there.  A tick without a box still has the words of one round, and the issuing cameras' windows in them: the motion front
    files boxes there that only the device knows."""
    cams, cap = lay.cameras, lay.cap
    idle = cams - len(items)
    pairs = [s for it in items for s in it[1]['pair_slots']]
    d[0], d[1] = rounds, cams
    d[lay.h_pairs:lay.h_rows] = pairs + pairs[-2:] * idle
    d[lay.h_rows:lay.h_rows + cams] = [it[1]['flow_slot'] for it in items] + [-1] * idle
    rows = sorted({cell for it in items for cells in it[3] for cell in cells})
    used = []
    for r in range(max(rounds, 1)):
        rnd = d[lay.head + r * lay.D:lay.head + (r + 1) * lay.D]
        masks = rnd[lay.w_mask:].view(np.uint8)
        here = set()
        for k, issue, crops, blocks in items:
            lo, hi = r * cap, min(len(crops), (r + 1) * cap)
            rnd[lay.w_rwin + k * lay.T:lay.w_rwin + (k + 1) * lay.T] = issue['raw_slots']
            rnd[lay.w_fwin + k * lay.Tf:lay.w_fwin + (k + 1) * lay.Tf] = issue['flow_slots']
            if hi <= lo:
                continue
            rnd[k] = hi - lo
            o = lay.w_crops + 4 * k * cap
            rnd[o:o + 4 * (hi - lo)] = np.asarray(crops[lo:hi], np.int32).reshape(-1)
            for b, cells in enumerate(blocks[lo:hi]):
                for (hh, ww) in cells:
                    masks[(hh * lay.wb + ww) * cams * cap + k * cap + b] = 1
                    here.add((hh, ww))
        if r < rounds:
            used.append([i for i, cell in enumerate(rows) if cell in here])
    return rows, used


class _Staging:
    """Pinned host buffers for uploads that are still in flight when the host moves on: a buffer is handed out again only once the
    event recorded behind its last copy has completed (asked, never waited for); otherwise a new one is made."""

    def __init__(self):
        self.items = {}

    def get(self, key, shape, dtype):
        pool = self.items.setdefault((key, tuple(shape), dtype), [])
        for it in pool:
            if it[1] is None or it[1].query():
                it[1] = None
                return it
        it = [torch.empty(tuple(shape), dtype=dtype, pin_memory=True), None]
        pool.append(it)
        return it

    def hold(self, key, shape, dtype):
        """A buffer for a read-back: it stays out of the pool until its reader (``StreamResult``) hands it back."""
        it = self.get(key, shape, dtype)
        it[1] = _HELD
        return it


class _Held:
    """In place of an event on a pooled buffer that a ``StreamResult`` still has to read: never 'completed'."""

    @staticmethod
    def query():
        return False


_HELD = _Held()


class StreamFront:
    """What ``StreamScorer``, ``MultiStreamScorer`` and ``StreamCollector`` share: a frame from ``push`` to its cubes in the store.

    A subclass checks the arguments that are its own, calls ``_refuse`` (the shared refusals of the configuration and the frame shape),
    builds its schedule -- a ``RingSchedule``, or a ``MultiSchedule`` for several cameras -- and hands it to ``__init__``, which refuses
    what is left to refuse and only then touches the GPU.  Behind it the subclass keeps what it puts behind the cut.  What differs in
    the front half itself is stated here, as class attributes; ``motion`` and ``cameras`` may be set per instance before ``_refuse``."""

    verb = 'scores'                          # what the class does with a stream, in the border_mode refusal
    block_mode_key = 'test_block_mode'       # the dataset's key of calc_block_idx's mode ...
    painted_only = True                      # ... and box_cells' rule: the test rules
    motion = False                           # the boxes are given
    cameras = 1
    tail = False                             # True: the subclass keeps words of its own behind the motion tables, see _fill_tail

    def _refuse(self, c, frame_shape):
        """The refusals every stream shares, on the host: a dataset without motion constants, a centred window, a frame that is no
        image.  Leaves ``H``, ``W``, ``C``."""
        from vec_vad_amd.motion import CONSTANTS
        cp, ds, method = c['cp'], c['dataset_name'], c['method']
        if self.motion and ds not in CONSTANTS:
            raise ValueError("stream_boxes = motion: the motion stage has no constants for dataset {!r}".format(ds))
        if cp.get(method, 'border_mode') != 'predict':
            raise ValueError("a stream {} with border_mode = predict only (a centred window needs frames that have not arrived), got "
                             "{!r}".format(self.verb, cp.get(method, 'border_mode')))
        H, W, C = (int(v) for v in frame_shape)
        if C not in (1, 3):
            raise ValueError('frames must have 1 or 3 channels, got frame_shape {!r}'.format(tuple(frame_shape)))
        self.H, self.W, self.C = H, W, C

    def __init__(self, c, sched, flownet2=None, device='cuda'):
        from vad_datasets import frame_size
        cp, ds = c['cp'], c['dataset_name']
        H, W, C, cams, cap = self.H, self.W, self.C, self.cameras, self.cap
        self.sched = sc = sched
        self.P = P = cp.getint(ds, 'patch_size')
        self.thr = cp.getfloat(ds, 'motionThr')
        self.hb, self.wb = c['h_block'], c['w_block']
        self.grid_h, self.grid_w = frame_size[ds][0], frame_size[ds][1]
        if self.motion and (H > self.grid_h or W > self.grid_w):
            raise ValueError('stream_boxes = motion: {}x{} frames are larger than the nominal {}x{} frame of {}, so a motion box could '
                             'fall outside the block grid'.format(H, W, self.grid_h, self.grid_w, ds))
        self.h_step, self.w_step = self.grid_h / self.hb, self.grid_w / self.wb
        self.block_mode = cp.getint(ds, self.block_mode_key)
        dev = torch.device(device)
        self.device = dev = dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())
        if flownet2 is None:
            from calc_optical_flow import load_flownet2
            flownet2 = load_flownet2(c['flownet2_checkpoint'], device=dev, fp16=c['direct_flow_fp16'])
        from calc_optical_flow import FLOW_H, FLOW_W
        self.flow_h, self.flow_w = FLOW_H, FLOW_W
        self.flow_in, self.flow_out, self.flow_graph = flownet2.graph_entry((cams, 3, 2, FLOW_H, FLOW_W))
        self.flownet2 = flownet2
        self.raw_ring = torch.zeros((cams * sc.R, H, W, C), dtype=torch.uint8, device=dev)
        self.flow_ring = torch.zeros((cams * sc.Rf, H, W, 2), dtype=torch.float32, device=dev)
        self.store_raw = torch.zeros((cams * cap, sc.T, P, P, C), dtype=torch.uint8, device=dev)
        self.store_flow = torch.zeros((cams * cap, sc.Tf, P, P, 2), dtype=torch.float32, device=dev)
        self.lay = lay = TickLayout(cams, cap, sc.T, sc.Tf, self.hb, self.wb)
        self.desc = torch.zeros(lay.words(1), dtype=torch.int32, device=dev)       # grows with the rounds of a frame or tick
        if self.motion:
            # behind the one round of a frame: motion window [3], 1 unused | appearance table [cap][5] = window 0, x1, y1, x2, y2
            from vec_vad_amd.motion import CONSTANTS
            self.w_mwin = lay.words(1)
            self.w_ap = self.w_mwin + 4
            self.words_motion = self.w_ap + 5 * cap
            self.desc = torch.zeros(self.words_motion, dtype=torch.int32, device=dev)
            self.mt = CONSTANTS[ds]
            self.mt_mask = torch.zeros((1, H, W), dtype=torch.uint8, device=dev)
            self.mt_work = torch.empty((_lib.lib().vv_mask_boxes_workspace_bytes(1, H, W),), dtype=torch.uint8, device=dev)
            self.mt_count = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.mt_boxes = torch.zeros((cap, 4), dtype=torch.int32, device=dev)                          # mcap = cap
            self.found = torch.zeros((2 + 4 * cap,), dtype=torch.int32, device=dev)                       # n, dropped, boxes_out [cap][4]
        self.staging = _Staging()

    @staticmethod
    def load(config_path, frame_shape=None, refuse=()):
        """The loading half of a ``from_config``: the configuration is read, every check of ``refuse`` is called with it (what the
        class refuses of a configuration, before any GPU work), and the artifacts ``train.py`` wrote under
        ``<data_root_dir>/<modality>/`` are loaded as ``test.py`` loads them.  ``frame_shape`` None: the dataset's nominal frame size
        with 3 channels.  Returns ``(c, net_set, stats_raw, stats_of, frame_shape, device)``."""
        from train import build_network, read_config
        c = read_config(config_path)
        for check in refuse:
            check(c)
        from test import load_artifacts
        from vad_datasets import frame_size
        ds = c['dataset_name']
        device = torch.device('cuda', torch.cuda.current_device())
        base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
        net_set, st_r, st_o = load_artifacts(base, c['mode_fg'], c['method'], ds == 'ShanghaiTech', lambda: build_network(c), device,
                                             c['h_block'], c['w_block'])
        if frame_shape is None:
            frame_shape = (frame_size[ds][0], frame_size[ds][1], 3)
        return c, net_set, st_r, st_o, frame_shape, device

    def _block_table(self, c, net_set, stats_raw, stats_of, scene):
        """``blocks``: per block of the grid ``(trainer, device statistics)``, or None for a block without a model -- built as
        ``test._group_scorer`` does -- with the weights the scores are formed under, and ``idx``, the whole store as a scoring launch
        names it."""
        from vec_vad_amd.trainer import FusedTrainer
        self.w_raw, self.w_of, self.use_flow = float(c['w_raw']), float(c['w_of']), bool(c['useFlow'])
        self.idx = torch.arange(self.cameras * self.cap, dtype=torch.long, device=self.device)
        nets = net_set[scene] if scene is not None else net_set
        s_raw = stats_raw[scene] if scene is not None else stats_raw
        s_of = stats_of[scene] if scene is not None else stats_of
        trainers, self.blocks = {}, {}
        for hh in range(self.hb):
            for ww in range(self.wb):
                models = nets[hh][ww]
                if len(models) == 0:
                    self.blocks[(hh, ww)] = None
                    continue
                net = models[0]
                if id(net) not in trainers:
                    trainers[id(net)] = FusedTrainer(net)
                st_r = s_raw[hh][ww]
                st_o = s_of[hh][ww] if self.use_flow else (0.0, 1.0)
                stats = torch.from_numpy(np.array([st_r[0], st_r[1], st_o[0], st_o[1]], np.float64)).to(self.device)
                self.blocks[(hh, ww)] = (trainers[id(net)], stats)

    def _warm_blocks(self, maps=False):
        """Every engine runs its eager launches and captures its graph, so that a push only replays."""
        for ent in self.blocks.values():
            if ent is not None:
                for _ in range(3):
                    ent[0].score_cubes(self.store_raw, self.store_flow, self.idx, maps=maps)
        torch.cuda.synchronize(self.device)

    # ---- host side of a frame: everything that can be refused is refused before a ring is touched
    def _prepare(self, frame_u8, boxes):
        """-> the checked frame and what is held for it until its look-ahead arrives: ``(boxes, crops, blocks, ap)``."""
        frame, boxes = check_frame(frame_u8, boxes, self.H, self.W, self.C)
        ap = None
        if self.motion:                                   # the given boxes are the frame's appearance boxes: one round holds them all
            from .motion import _ap_table
            if len(boxes) > self.cap:
                raise ValueError('{} appearance boxes, stream_max_boxes holds {} (with stream_boxes = motion a frame is one '
                                 'round)'.format(len(boxes), self.cap))
            ap = _ap_table([boxes], 1)                    # what vv_motion_mask erases: truncated to int32, x2 < 0 refused
        crops = boxes_to_crops(boxes, self.H, self.W)
        blocks = box_cells(boxes, self.grid_h, self.grid_w, self.hb, self.wb, self.h_step, self.w_step, self.block_mode, self.painted_only)
        return frame, (boxes, crops, blocks, ap)

    def _take(self, frame_u8, boxes, ap_boxes):
        """The front of a single-camera ``push``: the argument rule, the refusals, the schedule's step and the frame on its way into
        its ring slot.  Returns ``(issue | None, held)``: the frame that can now be issued, and what to hold for the new one."""
        if self.motion:
            boxes = ap_boxes if ap_boxes is not None else (boxes if boxes is not None else np.zeros((0, 4), np.float64))
        elif boxes is None or ap_boxes is not None:
            raise ValueError('push takes the frame and its boxes; ap_boxes and a push without boxes belong to stream_boxes = motion')
        frame, held = self._prepare(frame_u8, boxes)
        slot, issue = self.sched.push()
        self._upload(frame, slot)
        return issue, held

    def _upload(self, frame, slot):
        """A checked frame into its raw ring slot, through a pooled pinned buffer."""
        st = self.staging.get('frame', frame.shape, torch.uint8)
        st[0].numpy()[...] = frame
        self._copy(st, self.raw_ring[slot])

    def _copy(self, st, dst):
        """The pooled pinned buffer ``st`` into the device tensor ``dst``, with the event that frees the buffer."""
        dst.copy_(st[0], non_blocking=True)
        st[1] = torch.cuda.Event()
        st[1].record()

    # ---- device side: descriptor, flow, motion boxes, cut
    def _describe(self, items, behind=0):
        """``fill_tick`` of ``items`` (one per issuing camera, ascending, as the schedule yields them) on a pooled pinned buffer that has
        ``behind`` zeroed words behind the descriptor for the caller's own tables.  Returns ``(st, d, rounds, rows, used)``: the
        buffer, for ``_start``, its words as the host fills them, and what ``tick_descriptor`` returns."""
        lay = self.lay
        rounds = lay.rounds(items)
        st = self.staging.get('desc', (lay.words(rounds) + behind,), torch.int32)
        d = st[0].numpy()
        d[:] = 0
        return (st, d, rounds) + fill_tick(lay, items, rounds, d)

    def _start(self, st):
        """The first launches of an issue: the descriptor in the buffer of ``_describe`` to the device (its copy there grows to the
        longest one seen) and the flow that reads its header.  Returns the device words."""
        words = st[0].numel()
        if self.desc.numel() < words:
            self.desc = torch.zeros(words, dtype=torch.int32, device=self.device)
        self._copy(st, self.desc[:words])
        self._flow(self.desc.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        return self.desc

    def _flow(self, base, stream):
        """The flow fields of the issued frames, in place in the flow ring: the launches of ``calc_optical_flow.chunk_flows`` at
        ``cameras`` pairs, their tables read from the header of the descriptor at ``base``."""
        lib, sc, cams, lay = _lib.lib(), self.sched, self.cameras, self.lay
        _lib.check(lib.vv_flow_pairs_prep(self.raw_ring.data_ptr(), cams * sc.R, self.H, self.W, self.C, base + 4 * lay.h_pairs, cams,
                                          self.flow_h, self.flow_w, self.flow_in.data_ptr(), stream), 'vv_flow_pairs_prep')
        self.flow_graph.replay()
        _lib.check(lib.vv_flow_resize_back(self.flow_out.data_ptr(), cams, self.flow_h, self.flow_w, base + 4 * lay.h_rows, self.H, self.W,
                                           self.flow_ring.data_ptr(), cams * sc.Rf, stream), 'vv_flow_resize_back')

    def _round(self, desc, r):
        """Round ``r`` of the descriptor on the device: ``(rnd, n, masks)`` -- its words, the box counts ``[cameras]`` and the mask rows
        ``[hb*wb][cameras*cap]`` as bytes."""
        lay = self.lay
        rnd = desc[lay.head + r * lay.D:lay.head + (r + 1) * lay.D]
        return rnd, rnd[0:self.cameras], rnd[lay.w_mask:].view(torch.uint8)

    def _motion_front(self, issue, held):
        """The front half of a frame whose motion boxes the device finds, up to the tables ``vv_stream_cut`` reads: the descriptor of
        the ONE round (the appearance boxes in slots ``0..k-1``, as given boxes are filed), the flow, and ``vv_motion_mask`` ->
        ``vv_mask_boxes`` -> ``vv_stream_boxes``, which files the motion boxes behind them.  Returns ``(desc, rnd, n, masks)``: the
        descriptor and its round on the device, the box count on the device and the ``[hb*wb][cap]`` mask rows."""
        boxes, crops, blocks, ap = held
        lib, cap, sc, lay, k = _lib.lib(), self.cap, self.sched, self.lay, len(crops)
        st, d = self._describe([(0, issue, crops, blocks)], self.desc.numel() - lay.words(1))[:2]
        d[self.w_mwin:self.w_mwin + 3] = issue['motion_slots']
        d[self.w_ap:self.w_ap + 5 * len(ap)] = ap.reshape(-1)
        if self.tail:                         # the count is the device's (found[0]); the appearance boxes' rectangles are the host's
            self._fill_tail(d[self.t_base:], issue, k, boxes)
        desc = self._start(st)
        stream, base, c = torch.cuda.current_stream(self.device).cuda_stream, desc.data_ptr(), self.mt
        _lib.check(lib.vv_motion_mask(self.raw_ring.data_ptr(), sc.R, self.H, self.W, self.C, base + 4 * self.w_mwin, 1, c['ksize'],
                                      c['binary_thr'], base + 4 * self.w_ap if len(ap) else None, len(ap), c['extend'],
                                      self.mt_mask.data_ptr(), stream), 'vv_motion_mask')
        _lib.check(lib.vv_mask_boxes(self.mt_mask.data_ptr(), 1, self.H, self.W, c['area_thr'], c['extend'], cap, self.mt_work.data_ptr(),
                                     self.mt_work.numel(), self.mt_count.data_ptr(), self.mt_boxes.data_ptr(), stream), 'vv_mask_boxes')
        rnd, _, masks = self._round(desc, 0)
        found = self.found
        n = found[0:1]
        stream_boxes(self.mt_count, self.mt_boxes, k, self.H, self.W, self.grid_h, self.grid_w, self.hb, self.wb, self.h_step, self.w_step,
                     self.block_mode, n, found[1:2], rnd[lay.w_crops:lay.w_rwin].view(cap, 4), masks, found[2:])
        return desc, rnd, n, masks

    def _fill_tail(self, d, issue, n, boxes):
        """The hook of a subclass that sets ``tail``: it sizes ``desc`` for its words, names their first as ``t_base`` (16-byte
        aligned, behind ``words_motion``) and fills them here -- ``d``: the host words from ``t_base`` on; ``n`` boxes of ``boxes`` are
        the host's.  ``_motion_front`` calls it before the descriptor leaves the host."""
        raise NotImplementedError

    def _cut(self, rnd, n, keep):
        """``vv_stream_cut_multi`` of one round: every camera's boxes of the round into the camera's store slots, ``keep`` = the motion
        test."""
        lay = self.lay
        stream_cut_multi(self.raw_ring, self.flow_ring, self.cameras, n, rnd[lay.w_crops:lay.w_rwin], rnd[lay.w_rwin:lay.w_fwin],
                         rnd[lay.w_fwin:lay.w_fwin + self.cameras * lay.Tf], self.thr, self.store_raw, self.store_flow, keep)
