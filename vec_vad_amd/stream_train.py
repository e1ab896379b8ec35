"""Training from pushed frames: a camera's normal footage in, models and training-score statistics out (``StreamCollector``).

``vec_vad_amd.stream.StreamScorer`` scores a camera frame by frame, but the models and statistics it is built from could only come
from ``train.py`` on a dataset tree.  A ``StreamCollector`` is the scorer's front half with no model behind it
(``vec_vad_amd.stream_front.StreamFront``, the base class of both): the same frame checks and refusals before any state is touched, the
same ``RingSchedule`` with its one frame of look-ahead, the same descriptor through a pinned staging buffer, the flow at one pair per
launch and the cut of every round into ``max_boxes`` fixed slots (``boxes='motion'``: ``vv_motion_mask`` -> ``vv_mask_boxes`` ->
``vv_stream_boxes`` in front of the one round of a frame).  Behind
every cut ONE ``vv_stream_append`` packs the round's kept cubes behind those of the rounds before into a training store of
``[mi355x] collect_max_cubes`` cubes, with the frame, the box index, the box and the block cells of every cube in three small tables
next to it.  The cursor lives on the device (two cells, alternated per launch): neither ``push`` nor ``end_video`` synchronises.

The training rules apply, not the test rules: the block cells of a box are ``calc_block_idx(...)`` under ``train_block_mode``, not
gated by the painted-rectangle test -- what ``foreground.extract_device(mode='train')`` files -- and a box outside the grid is an
``IndexError`` before anything is touched.  ``motionThr`` and ``border_mode = predict`` are honoured as in the scorer.

``finish()`` is the one host synchronisation: the cursor and the meta rows come to the host and become the dict of
``foreground.extract_train_device`` -- on the same frames and boxes the same store and index lists as ``train.py`` with
``direct_train``, ``direct_flow`` and one pair per launch, bit for bit.  ``train()`` hands it to ``train.train_store`` and returns
what ``test.load_artifacts`` returns, so that a ``StreamScorer`` can be built from it directly.

What is not here: several cameras in one collector, ShanghaiTech (one model per scene), data-parallel training from a collected
store, re-collection per epoch, incremental updates of a trained model, a validation split.
"""
import os

import numpy as np
import torch

from . import _lib
from .stream_front import RingSchedule, StreamFront, _dev, check_max_boxes, check_max_cubes, check_stream_boxes  # noqa: F401

COLLECT_MAX_CUBES = 65536      # [mi355x] collect_max_cubes default: 65536 x 56 320 B (5 raw uint8 + 5 flow float32 patches) = 3.7 GB


def stream_append(raw_slots, flow_slots, keep, n, masks, boxes, frame, slot0, cursor_in, cursor_out, raw_store, flow_store, meta,
                  meta_boxes, meta_cells):
    """``vv_stream_append``: the kept cubes of one ``stream_cut`` round appended to a training store, all on the device.  raw_slots
    uint8 ``[cap,...]`` and flow_slots float32 ``[cap,...]`` (the round's stores), keep uint8 ``[cap]``, n int32 ``[1]``; masks uint8
    ``[cells,cap]`` (the round's block rows; ``cells`` may be 0) and boxes int32 ``[cap,4]`` or None; ``frame``: the running frame
    index, ``slot0``: the box index of slot 0; cursor_in / cursor_out int32 ``[1]``, two different cells.  raw_store / flow_store: the
    training store, ``[capacity,...]`` cubes of the slots' shapes; meta int32 ``[capacity,2]``, meta_boxes int32 ``[capacity,4]``,
    meta_cells uint8 of at least ``max(capacity * cells, 1)`` elements.  The ``j``-th slot ``b < n[0]`` with ``keep[b]`` goes to cube
    ``d = cursor_in[0] + j`` when ``d < capacity`` -- its bytes, ``meta[d] = (frame, slot0 + b)``, ``meta_boxes[d] = boxes[b]`` (zeros
    without boxes), ``meta_cells[d] = masks[:, b]`` -- and ``cursor_out[0] = cursor_in[0] + kept``, not clamped.  Nothing else is
    written."""
    _dev('raw_slots', raw_slots, torch.uint8), _dev('flow_slots', flow_slots, torch.float32)
    _dev('raw_store', raw_store, torch.uint8), _dev('flow_store', flow_store, torch.float32)
    if raw_slots.dim() < 1 or raw_slots.shape[0] < 1 or flow_slots.shape[0] != raw_slots.shape[0]:
        raise ValueError('raw_slots and flow_slots must be [cap,...] tensors of one cap >= 1')
    cap, capacity = raw_slots.shape[0], raw_store.shape[0]
    if capacity < 1 or flow_store.shape[0] != capacity or tuple(raw_store.shape[1:]) != tuple(raw_slots.shape[1:]) \
            or tuple(flow_store.shape[1:]) != tuple(flow_slots.shape[1:]):
        raise ValueError('raw_store and flow_store must be [capacity,...] tensors of one capacity >= 1 and of the cubes of the slots')
    _dev('masks', masks, torch.uint8)
    if masks.dim() != 2 or masks.shape[1] != cap:
        raise ValueError('masks must be a [cells,%d] tensor' % cap)
    cells = masks.shape[0]
    _dev('keep', keep, torch.uint8, cap), _dev('n', n, torch.int32, 1)
    _dev('cursor_in', cursor_in, torch.int32, 1), _dev('cursor_out', cursor_out, torch.int32, 1)
    _dev('meta', meta, torch.int32, 2 * capacity), _dev('meta_boxes', meta_boxes, torch.int32, 4 * capacity)
    _dev('meta_cells', meta_cells, torch.uint8, max(capacity * cells, 1))
    if boxes is not None:
        _dev('boxes', boxes, torch.int32, 4 * cap)
    _lib.check(_lib.lib().vv_stream_append(raw_slots.data_ptr(), flow_slots.data_ptr(), keep.data_ptr(), n.data_ptr(), cap,
                                           raw_slots[0].numel(), 4 * flow_slots[0].numel(), masks.data_ptr() if cells else None, cells,
                                           boxes.data_ptr() if boxes is not None else None, int(frame), int(slot0), cursor_in.data_ptr(),
                                           cursor_out.data_ptr(), capacity, raw_store.data_ptr(), flow_store.data_ptr(), meta.data_ptr(),
                                           meta_boxes.data_ptr(), meta_cells.data_ptr(),
                                           torch.cuda.current_stream(raw_store.device).cuda_stream), 'vv_stream_append')


def meta_groups(meta, meta_cells, n_frames, wb):
    """The index lists of a collected store from its meta rows, pure (no GPU): meta int ``[n,2]`` rows ``(frame, box)`` in store
    order, meta_cells uint8 ``[n,hb*wb]`` (cell ``hi * wb + wi`` set: the cube's box lies in block ``(hi, wi)``).  Returns
    ``foreground.block_groups(cube_frame, cube_blocks, n_frames)``."""
    from foreground import block_groups
    meta, meta_cells = np.asarray(meta).reshape(-1, 2), np.asarray(meta_cells)
    if len(meta_cells) != len(meta) or meta_cells.ndim != 2:
        raise ValueError('meta_cells must hold one row of cells per meta row')
    cube_blocks = [[(int(k) // wb, int(k) % wb) for k in np.nonzero(row)[0]] for row in meta_cells]
    return block_groups([int(f) for f in meta[:, 0]], cube_blocks, n_frames)


class StreamCollector(StreamFront):
    """``StreamCollector(c, frame_shape, flownet2=None, max_boxes=None, max_cubes=None, boxes=None, device='cuda')``.

    ``c``: the dict of ``train.read_config``; ``frame_shape``: ``(H, W, C)`` of the uint8 frames that will be pushed (C = 1 or 3);
    ``flownet2``: the network (None loads ``[mi355x] flownet2_checkpoint``, in fp16 mode with ``direct_flow_fp16``); ``max_boxes``:
    slots per round (None: ``[mi355x] stream_max_boxes``); ``max_cubes``: cubes the training store holds (None: ``[mi355x]
    collect_max_cubes``); ``boxes``: ``'given'`` or ``'motion'`` as for ``StreamScorer`` (None: ``[mi355x] stream_boxes``; motion
    needs ``motion.CONSTANTS`` for the dataset and frames no larger than its nominal frame).  Every refusal is a one-line error
    before any GPU work; ShanghaiTech is a ``NotImplementedError``.

    ``push(frame_u8 [H,W,C], boxes float [n,>=4])`` and ``end_video()`` return None and do not synchronise the host with the device.
    With ``boxes='motion'``: ``push(frame_u8)`` or ``push(frame_u8, ap_boxes=rows)``; a frame is one round there, and the motion boxes
    that found no free slot are counted on the device.  ``finish()`` -- the one synchronisation -- returns the dict of
    ``foreground.extract_train_device``: ``raw`` / ``flow`` (the store, of which the first ``n`` cubes are valid, in frame and then box
    order), ``n``, ``n_frames``, ``groups`` (``meta_groups``), ``boxes`` (float64 ``[n,4]``: the pushed boxes or the device's motion
    boxes) and ``dropped_boxes``.  A run that kept more cubes than the store holds raises a one-line ``ValueError`` there that names
    the number needed and ``collect_max_cubes``; no partial set is returned.  After ``finish()`` the collector refuses further pushes.

    ``train(net=None, save=False)`` -> ``(net_set, stats_raw, stats_of)`` as ``test.load_artifacts`` returns them: ``finish()`` if
    needed, then ``train.train_store``; ``save`` also writes the three files where ``train.py`` writes them."""

    verb = 'collects'
    block_mode_key = 'train_block_mode'      # the training rules: every cell of calc_block_idx, no painted-rectangle test
    painted_only = False

    def __init__(self, c, frame_shape, flownet2=None, max_boxes=None, max_cubes=None, boxes=None, device='cuda'):
        self.cap = check_max_boxes(c.get('stream_max_boxes', 64) if max_boxes is None else max_boxes)      # before any GPU work
        self.capacity = check_max_cubes(c.get('collect_max_cubes', COLLECT_MAX_CUBES) if max_cubes is None else max_cubes)
        self.motion = check_stream_boxes(c.get('stream_boxes', 'given') if boxes is None else boxes) == 'motion'
        cp, method = c['cp'], c['method']
        if c['dataset_name'] == 'ShanghaiTech':
            from train import DIRECT_TRAIN_SHANGHAI
            raise NotImplementedError(DIRECT_TRAIN_SHANGHAI)
        self._refuse(c, frame_shape)
        self.c = c
        super().__init__(c, RingSchedule(cp.getint(method, 'context_frame_num'), cp.getint(method, 'context_of_num'), motion=self.motion),
                         flownet2, device)
        sc, P, C, cells, dev = self.sched, self.P, self.C, self.hb * self.wb, self.device
        self.keep = torch.zeros(self.cap, dtype=torch.uint8, device=dev)
        # the training store and its tables; state: cursor cells [2] (launch i reads cell i % 2 and writes the other), dropped boxes
        self.train_raw = torch.empty((self.capacity, sc.T, P, P, C), dtype=torch.uint8, device=dev)
        self.train_flow = torch.empty((self.capacity, sc.Tf, P, P, 2), dtype=torch.float32, device=dev)
        self.meta = torch.zeros((self.capacity, 2), dtype=torch.int32, device=dev)
        self.meta_boxes = torch.zeros((self.capacity, 4), dtype=torch.int32, device=dev)
        self.meta_cells = torch.zeros((self.capacity, cells), dtype=torch.uint8, device=dev)
        self.state = torch.zeros(3, dtype=torch.int32, device=dev)
        self.launches = 0         # vv_stream_append launches so far: the current cursor is cell launches % 2
        self.held = None          # (boxes, crops, blocks, appearance table | None) of the frame that waits for its look-ahead
        self.frames = 0           # frames pushed so far, across videos
        self.given = []           # per pushed frame: the boxes the host knows (given boxes, or the appearance boxes in motion mode)
        self.slots = 0            # an upper bound of the cubes appended so far, known without asking the device
        self.store = None         # what finish() returned
        self.finished = False
        torch.cuda.synchronize(dev)

    def push(self, frame_u8, boxes=None, ap_boxes=None):
        if self.finished:
            raise ValueError('this collector has finished: its store is handed over, start a new one for more frames')
        issue, held = self._take(frame_u8, boxes, ap_boxes)
        if issue is not None:
            self._issue(issue, self.held)
        self.held = held
        self.given.append(held[0])
        self.frames += 1

    def end_video(self):
        if self.finished:
            raise ValueError('this collector has finished: its store is handed over, start a new one for more frames')
        held, self.held = self.held, None
        issue = self.sched.end_video()
        if issue is not None:
            self._issue(issue, held)

    def _append(self, n, masks, boxes_dev, slot0):
        """One ``vv_stream_append`` behind a round's cut, on the current stream; the cursor cells change roles."""
        i = self.launches % 2
        stream_append(self.store_raw, self.store_flow, self.keep, n, masks.view(self.hb * self.wb, self.cap), boxes_dev, self.frames - 1,
                      slot0, self.state[i:i + 1], self.state[1 - i:2 - i], self.train_raw, self.train_flow, self.meta, self.meta_boxes,
                      self.meta_cells)
        self.launches += 1

    def _issue(self, issue, held):
        """The launches of one issued frame (the frame pushed before the newest, or a video's last): the descriptor, the flow, and per
        round of ``max_boxes`` boxes ``vv_stream_cut`` and ``vv_stream_append``.  A frame without boxes still gets its flow: later
        frames' flow windows name it."""
        if self.motion:
            desc, rnd, n, masks = self._motion_front(issue, held)
            self._cut(rnd, n, self.keep)
            self._append(n, masks[:self.hb * self.wb * self.cap], self.found[2:], 0)
            self.state[2:3].add_(self.found[1:2])         # the dropped boxes, accumulated where they are counted
            self.slots += self.cap
            return
        boxes, crops, blocks, _ = held
        st, _, rounds, _, _ = self._describe([(0, issue, crops, blocks)])
        desc = self._start(st)
        for r in range(rounds):
            rnd, n, masks = self._round(desc, r)
            self._cut(rnd, n, self.keep)
            self._append(n, masks[:self.hb * self.wb * self.cap], None, r * self.cap)
        self.slots += len(crops)

    def finish(self):
        """The one host synchronisation: the cursor, the dropped-box count and the meta rows come to the host (one event behind
        non-blocking copies to pinned memory), and the store becomes the dict of ``foreground.extract_train_device``.  A video that
        was not ended is ended here."""
        if self.store is not None:
            return self.store
        if self.finished:
            raise ValueError('this collector has finished without a store (collect_max_cubes was too small)')
        self.end_video()
        self.finished = True
        bound = min(self.slots, self.capacity)
        parts = [self.state, self.meta[:bound], self.meta_boxes[:bound], self.meta_cells[:bound]]
        hosts = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in parts]
        for h, t in zip(hosts, parts):
            h.copy_(t, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        event.synchronize()
        state, meta, meta_boxes, meta_cells = (h.numpy() for h in hosts)
        n, dropped = int(state[self.launches % 2]), int(state[2])
        if n > self.capacity:
            self.train_raw = self.train_flow = None
            raise ValueError('[mi355x] collect_max_cubes = {}: the pushed frames keep {} cubes, and training needs all of them in one '
                             'store (raise collect_max_cubes)'.format(self.capacity, n))
        meta, meta_boxes, meta_cells = meta[:n], meta_boxes[:n], meta_cells[:n]
        boxes = np.zeros((n, 4), np.float64)
        for s, (f, b) in enumerate(meta):
            host = self.given[f]
            boxes[s] = host[b] if b < len(host) else meta_boxes[s]
        self.store = dict(raw=self.train_raw, flow=self.train_flow, n=n, n_frames=self.frames, boxes=boxes, dropped_boxes=dropped,
                          groups=meta_groups(meta, meta_cells, self.frames, self.wb))
        return self.store

    def train(self, net=None, save=False, log=print):
        """Models and statistics from the collected store: ``train.train_store`` on ``finish()``'s dict with ``net`` (None:
        ``train.build_network(c)``), returned as ``test.load_artifacts`` returns them -- built by the same code from the same three
        nested lists.  ``save``: the lists are also written where ``train.py`` writes them."""
        from test import artifacts_from
        from train import build_network, save_outputs, train_store
        c = self.c
        store = self.finish()
        if net is None:
            net = build_network(c)
        model_set, raw_scores_set, of_scores_set = train_store(c, store, net, log=log)
        if save:
            os.makedirs(os.path.join(c['data_root_dir'], c['modality']), exist_ok=True)
            save_outputs(c, model_set, raw_scores_set, of_scores_set, log=log)
        return artifacts_from(model_set, raw_scores_set, of_scores_set, False, lambda: build_network(c), self.device)
