"""Several cameras in one scorer (``MultiStreamScorer``): what ``vec_vad_amd.stream.StreamScorer`` does for one camera, for ``cameras``
cameras that share ONE launch set per tick.

Somebody with eight cameras can build eight ``StreamScorer``s; each then pays its own descriptor upload, its own FlowNet2 replay at one
pair per launch and its own scoring launches of ``max_boxes`` cubes, none of which fills the chip.  Here the cameras share one raw
ring ``[cameras*R,H,W,C]`` and one flow ring ``[cameras*Rf,H,W,2]`` (camera ``k`` owns slots ``k*R ..`` and ``k*Rf ..``), one cube store
of ``cameras*max_boxes`` slots (camera ``k`` owns slots ``k*max_boxes ..``), one FlowNet2 graph at ``cameras`` pairs per launch and one
descriptor.  A call of ``push`` or ``end_video`` is one TICK: every camera that can issue a frame does so in the same launches --

  one descriptor copy (``tick_descriptor``: header, the FlowNet2 launch tables, per round the box counts, crops, windows and masks);
  one ``vv_flow_pairs_prep``, one replay of the ``cameras``-pair graph, one ``vv_flow_resize_back`` -- the tables are those of
    ``calc_optical_flow.launch_tables`` for the issuing cameras, the tail repeating the last pair at row -1 (computed, not written),
    so a tick with fewer issues replays the same graph;
  per round one ``vv_stream_cut_multi`` over the whole store;
  per block that a box of the round belongs to, one ``FusedTrainer.score_cubes`` over the whole store and one
    ``vv_stream_scores_multi``;
  one read-back behind one event, shared by the tick's results.

A tick has ``max_k ceil(n_k / max_boxes)`` rounds; a camera with fewer has ``n = 0`` in the later ones, an idle camera in all.  The
values are those of ``StreamScorer`` up to the launch sizes: the flow of a frame is that of ``chunk_flows`` at ``cameras`` pairs per
launch, an error sum that of a scoring launch of ``cameras*max_boxes`` cubes; with ``cameras = 1`` they are ``StreamScorer``'s bit for bit.
No camera's values depend on another camera's frames or boxes.

Limits.  All cameras share one frame shape and one model set (for ShanghaiTech: one scene per scorer).  Boxes are given: the motion
boxes, masks, smoothing, overlays, tracks and per-pixel error maps of ``StreamScorer`` stay single-camera features and are refused
here when switched on in the configuration.  Cameras that tick at different rates pass ``None`` for the ticks they miss.

The front half -- refusals, rings and stores, ``MultiSchedule``, ``TickLayout`` / ``tick_descriptor``, the frame upload, the flow and
the cut -- is ``vec_vad_amd.stream_front.StreamFront`` at ``cameras`` cameras, shared with ``StreamScorer`` and ``StreamCollector``
(which are that class at one camera); its names are re-imported here.  This module holds the tick's back half: the scoring launches
per block, ``vv_stream_scores_multi`` and the one read-back.
"""
import numpy as np
import torch

from . import _lib
from .scoring import BIG
from .stream_front import (MultiSchedule, StreamFront, TickLayout, _dev, check_cameras, check_max_boxes, check_stream_boxes,  # noqa: F401
                           stream_cut_multi, tick_descriptor)

SINGLE_CAMERA_KEYS = ('stream_boxes', 'stream_masks', 'stream_smooth', 'stream_render', 'stream_tracks')


def check_single_camera_keys(c):
    """The keys of ``c`` that switch on a single-camera feature of the stream are refused, each with its one-line ``ValueError``; no GPU
    is touched."""
    for key in SINGLE_CAMERA_KEYS:
        on = check_stream_boxes(c.get(key, 'given')) == 'motion' if key == 'stream_boxes' else bool(c.get(key, False))
        if on:
            raise ValueError('[mi355x] {} = {} is a single-camera feature: several cameras in one scorer take given boxes and deliver '
                             'scores only (use stream_cameras = 1)'.format(key, 'motion' if key == 'stream_boxes' else 'on'))


def check_stream_maps(c):
    """``stream_maps`` switched on in ``c`` is refused with a one-line ``ValueError``: the per-pixel error mask is a single-camera
    feature like those of ``SINGLE_CAMERA_KEYS``; no GPU is touched."""
    if bool(c.get('stream_maps', False)):
        raise ValueError('[mi355x] stream_maps = on is a single-camera feature: several cameras in one scorer take given boxes and '
                         'deliver scores only (use stream_cameras = 1)')


def stream_scores_multi(raw, of, stats, w_raw, w_of, keep, n, mask, cams, cap, box_scores, box_stride, frame_score, frame_stride):
    """``vv_stream_scores_multi``: ``stream.stream_scores`` for ``cams`` cameras in one launch.  raw / of float32 ``[cams*cap]`` (``of``
    None drops the flow term; ``raw`` may be None with ``stats`` None), stats float64 ``[4]`` or None, keep and mask uint8 ``[cams*cap]``,
    n int32 ``[cams]``, all on the device.  Written in place: ``box_scores[k*box_stride + b]`` for ``b < n[k]`` and
    ``frame_score[k*frame_stride]`` (max-accumulated), with the rule of ``stream_scores`` per camera; strides in float64 elements.
    Slots at or above ``n[k]`` are neither read nor written; the cell of a camera with ``n[k] = 0`` keeps its value."""
    cams, cap, box_stride, frame_stride = int(cams), int(cap), int(box_stride), int(frame_stride)
    if cams < 1 or cap < 0 or box_stride < cap or frame_stride < 1:
        raise ValueError('cams >= 1, cap >= 0, box_stride >= cap and frame_stride >= 1 are required, got {} {} {} {}'.format(
            cams, cap, box_stride, frame_stride))
    slots = cams * cap
    _dev('box_scores', box_scores, torch.float64, (cams - 1) * box_stride + cap)
    _dev('frame_score', frame_score, torch.float64, (cams - 1) * frame_stride + 1)
    _dev('keep', keep, torch.uint8, slots), _dev('mask', mask, torch.uint8, slots), _dev('n', n, torch.int32, cams)
    if stats is not None:
        _dev('stats', stats, torch.float64, 4), _dev('raw', raw, torch.float32, slots)
        if of is not None:
            _dev('of', of, torch.float32, slots)
    _lib.check(_lib.lib().vv_stream_scores_multi(raw.data_ptr() if stats is not None else None,
                                                 of.data_ptr() if (stats is not None and of is not None) else None,
                                                 stats.data_ptr() if stats is not None else None, float(w_raw), float(w_of), float(BIG),
                                                 keep.data_ptr(), n.data_ptr(), mask.data_ptr(), cams, cap, box_scores.data_ptr(),
                                                 box_stride, frame_score.data_ptr(), frame_stride,
                                                 torch.cuda.current_stream(box_scores.device).cuda_stream), 'vv_stream_scores_multi')


class MultiStreamResult:
    """The scores of one frame of one camera, on their way to the host.  ``camera``; ``frame``: the running index of the frame among
    that camera's pushes (counted from 0 across videos); ``boxes``, float64 ``[n,4]``, the pushed boxes; ``dropped`` = 0.  ``wait()``
    blocks until the tick's copy has landed -- all results of a tick share one read-back and one event -- and returns ``(score,
    box_scores, kept)`` with the meaning of ``StreamResult.wait()``."""

    def __init__(self, camera, frame, boxes, n, rows, width, cap, rounds, stride, host, host_keep, event):
        self.camera, self.frame, self.dropped = camera, frame, 0
        self.boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        self._n, self._rows, self._width, self._cap, self._rounds, self._stride = n, rows, width, cap, rounds, stride
        self._host, self._host_keep, self._event = host, host_keep, event

    def wait(self):
        self._event.synchronize()
        k, n, cap = self.camera, self._n, self._cap
        a = self._host.numpy()[k * self._stride:(k + 1) * self._stride]
        box = np.full(n, -float(BIG), np.float64)
        if self._rows and n:
            box = a[1:].reshape(self._rows, self._width)[:, :n].max(axis=0)
        kept = self._host_keep.numpy()[:self._rounds, k * cap:(k + 1) * cap].reshape(-1)[:n].astype(bool)
        return float(a[0]), box.copy(), kept


class MultiStreamScorer(StreamFront):
    """``MultiStreamScorer(c, net_set, stats_raw, stats_of, frame_shape, cameras, flownet2=None, scene=None, max_boxes=None,
    device='cuda')``: the arguments of ``StreamScorer`` plus the number of cameras, which all deliver ``frame_shape`` frames and are scored
    by one model set (``scene``).  The same configuration is honoured (``border_mode = predict`` only, ``useFlow``, ``context_of_num``
    0 and 4, ``w_raw`` / ``w_of``, ``motionThr``, ``precision``, the block grid of the nominal frame); ``max_boxes`` is the store slots
    PER CAMERA.  Boxes are given; ``stream_boxes = motion``, ``stream_masks``, ``stream_smooth``, ``stream_render`` and ``stream_tracks``
    switched on in ``c`` are refused with a one-line ``ValueError`` before any GPU work.

    ``push(frames, boxes)``: two sequences of length ``cameras``; a ``None`` frame means that camera has no frame this tick (its boxes
    entry is ignored).  ``end_video(cameras=None)``: None ends every camera that holds a frame, a list the named ones (a camera without
    frames is skipped).  Each call is ONE tick: every camera that can issue -- the previous frame of every camera that got a frame;
    the last frame of every ended camera -- does so in the same launch set.  Both return the tick's ``MultiStreamResult``s in ascending
    camera order, and neither synchronises the host with the device.  Everything that can be refused (a wrong frame shape or dtype,
    a box outside the block grid, a video of one frame, a bad camera list) is refused for ALL cameras before any ring, schedule or
    counter is touched: a refused call leaves every camera as it was."""

    def __init__(self, c, net_set, stats_raw, stats_of, frame_shape, cameras, flownet2=None, scene=None, max_boxes=None, device='cuda'):
        self.cameras = check_cameras(cameras)                                                                # all before any GPU work
        self.cap = check_max_boxes(c.get('stream_max_boxes', 64) if max_boxes is None else max_boxes)
        check_single_camera_keys(c)
        check_stream_maps(c)
        self._refuse(c, frame_shape)
        cp, method = c['cp'], c['method']
        super().__init__(c, MultiSchedule(self.cameras, cp.getint(method, 'context_frame_num'), cp.getint(method, 'context_of_num')),
                         flownet2, device)
        self._block_table(c, net_set, stats_raw, stats_of, scene)
        self.held = [None] * self.cameras         # per camera: (boxes, crops, blocks, None) of the frame that waits for its look-ahead
        self.frames = [0] * self.cameras          # per camera: frames pushed so far, across videos
        self._warm_blocks()

    @classmethod
    def from_config(cls, config_path='config.cfg', cameras=None, frame_shape=None, flownet2=None, scene=None):
        """The scorer of a configuration, as ``StreamScorer.from_config``; ``cameras`` None reads ``[mi355x] stream_cameras``.  A bad
        key raises before any GPU work."""
        if cameras is not None:
            cameras = check_cameras(cameras)
        c, net_set, st_r, st_o, frame_shape, device = cls.load(config_path, frame_shape, (check_single_camera_keys, check_stream_maps))
        if cameras is None:
            cameras = c['stream_cameras']                 # read_config has checked it
        return cls(c, net_set, st_r, st_o, frame_shape, cameras, flownet2=flownet2, scene=scene, device=device)

    def push(self, frames, boxes):
        cams = self.cameras
        if len(frames) != cams or len(boxes) != cams:
            raise ValueError('push takes one frame (or None) and one box table per camera: {} and {} for {} cameras'.format(
                len(frames), len(boxes), cams))
        ready = {}
        for k in range(cams):                             # every camera's refusals first: nothing is touched before all have passed
            if frames[k] is not None:
                if boxes[k] is None:
                    raise ValueError('camera {}: push takes the frame and its boxes'.format(k))
                ready[k] = self._prepare(frames[k], boxes[k])
        issued = []
        for k, slot, issue in self.sched.push([k in ready for k in range(cams)]):
            self._upload(ready[k][0], slot)
            if issue is not None:
                issued.append((k, issue, self.held[k], self.frames[k] - 1))
        out = self._tick(issued)
        for k in ready:
            self.held[k] = ready[k][1]
            self.frames[k] += 1
        return out

    def end_video(self, cameras=None):
        issued = []
        for k, issue in self.sched.end_video(cameras):    # raises before any schedule is changed
            issued.append((k, issue, self.held[k], self.frames[k] - 1))
            self.held[k] = None
        return self._tick(issued)

    def _score_block(self, cell, keep, n, masks, box_scores, frame_score, stride):
        """One block's share of a round: its model scores the WHOLE store in one launch (no launch for a block without a model),
        ``vv_stream_scores_multi`` reduces per camera under ``keep`` and the block's mask row."""
        hh, ww = cell
        ent = self.blocks[cell]
        raw = of = stats = None
        if ent is not None:
            raw, of = ent[0].score_cubes(self.store_raw, self.store_flow, self.idx)
            raw = raw.to(torch.float32).contiguous()
            of = of.to(torch.float32).contiguous() if (of is not None and self.use_flow) else None
            stats = ent[1]
        slots = self.cameras * self.cap
        m0 = (hh * self.wb + ww) * slots
        stream_scores_multi(raw, of, stats, self.w_raw, self.w_of, keep, n, masks[m0:m0 + slots], self.cameras, self.cap, box_scores, stride,
                            frame_score, stride)

    def _tick(self, issued):
        """The launch set of one tick.  issued: ``(camera, issue, held, frame index)`` per issuing camera, ascending."""
        if not issued:
            return []
        cams, cap = self.cameras, self.cap
        st, _, rounds, rows, used = self._describe([(k, issue, held[1], held[2]) for k, issue, held, _ in issued])
        desc = self._start(st)
        width = rounds * cap
        stride = 1 + len(rows) * width                    # per camera: the frame's cell, then its [rows][width] box scores
        # the tick's results in ONE buffer, so that the read-back is one copy: float64 [cams][stride] | keep uint8 [rounds][cams*cap]
        nb = 8 * cams * stride
        buf = torch.empty(nb + max(rounds, 1) * cams * cap, dtype=torch.uint8, device=self.device)
        out, keep = buf[:nb].view(torch.float64), buf[nb:].view(max(rounds, 1), cams * cap)
        out.fill_(-float(BIG))
        keep.zero_()
        for r in range(rounds):
            rnd, n, masks = self._round(desc, r)
            self._cut(rnd, n, keep[r])
            for i in used[r]:
                self._score_block(rows[i], keep[r], n, masks, out[1 + i * width + r * cap:], out, stride)
        host_buf = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=True)
        host_buf.copy_(buf, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        host, host_keep = host_buf[:nb].view(torch.float64), host_buf[nb:].view(max(rounds, 1), cams * cap)
        return [MultiStreamResult(k, frame, held[0], len(held[1]), len(rows), width, cap, rounds, stride, host, host_keep, event)
                for k, _, held, frame in issued]
