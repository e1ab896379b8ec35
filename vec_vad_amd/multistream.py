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
"""
import os

import numpy as np
import torch

from . import _lib
from .scoring import BIG
from .stream import RingSchedule, StreamScorer, _Staging, _dev, check_max_boxes, check_stream_boxes

SINGLE_CAMERA_KEYS = ('stream_boxes', 'stream_masks', 'stream_smooth', 'stream_render', 'stream_tracks')


def check_cameras(v):
    """``stream_cameras`` as an integer >= 1, else a one-line ``ValueError``; no GPU is touched."""
    if isinstance(v, str):
        try:
            v = int(v.strip())
        except ValueError:
            pass
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError('[mi355x] stream_cameras must be an integer >= 1, got {!r}'.format(v))
    return int(v)


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


def stream_cut_multi(raw_ring, flow_ring, cams, n, crops, raw_win, flow_win, thr, raw_store, flow_store, keep, energy=None):
    """``vv_stream_cut_multi``: ``stream.stream_cut`` for ``cams`` cameras in one launch.  raw_ring uint8 ``[cams*R,H,W,C]``, flow_ring
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

    def words(self, rounds):
        return self.head + max(int(rounds), 1) * self.D


def tick_descriptor(lay, items):
    """The descriptor of one tick, pure (no GPU).  ``items``: ``(camera, issue, crops, blocks)`` per issuing camera in ascending camera
    order -- the ``MultiSchedule`` issue, int32 ``[n,4]`` crops (``boxes_to_crops``) and per box the sorted list of grid cells
    ``(h, w)`` it belongs to (empty for a box that paints no pixel).  Returns ``(d, rounds, rows, used)``: the int32 words in the
    layout of ``TickLayout``; the rounds, ``max ceil(n / cap)``; the sorted cells that any box belongs to; per round the indices into
    ``rows`` of the cells with a box of that round.

    The pair and row tables are ``calc_optical_flow.launch_tables(pair_slots, flow_slot, cameras)[0]`` of the issuing cameras: absolute
    ring slots, the tail repeating the last pair at row -1.  Box ``b`` of round ``r`` of camera ``k`` has its crop at ``crops[k][b]`` of
    that round and its mask bytes at ``masks[h*wb + w][k*cap + b]``; a camera that does not issue, or has no box left for a round, has
    ``n = 0`` there."""
    from calc_optical_flow import launch_tables
    cams, cap = lay.cameras, lay.cap
    ks = [it[0] for it in items]
    if ks != sorted(set(ks)) or any(not 0 <= k < cams for k in ks) or not ks:
        raise ValueError('a tick takes one item per issuing camera, in ascending camera order, got cameras {!r}'.format(ks))
    rounds = max((len(it[2]) + cap - 1) // cap for it in items)
    d = np.zeros(lay.words(rounds), np.int32)
    d[0], d[1] = rounds, cams
    pairs, rows_tab = launch_tables([it[1]['pair_slots'] for it in items], [it[1]['flow_slot'] for it in items], cams)[0]
    d[lay.h_pairs:lay.h_rows] = pairs.reshape(-1)
    d[lay.h_rows:lay.h_rows + cams] = rows_tab
    rows = sorted({cell for it in items for cells in it[3] for cell in cells})
    used = []
    for r in range(rounds):
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
        used.append([i for i, cell in enumerate(rows) if cell in here])
    return d, rounds, rows, used


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


class MultiStreamScorer:
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

    motion = False                       # what StreamScorer._prepare asks: boxes are given
    _prepare = StreamScorer._prepare     # the host side of one camera's frame: the same checks, crops and cells

    def __init__(self, c, net_set, stats_raw, stats_of, frame_shape, cameras, flownet2=None, scene=None, max_boxes=None, device='cuda'):
        self.cameras = check_cameras(cameras)                                                                # all before any GPU work
        self.cap = check_max_boxes(c.get('stream_max_boxes', 64) if max_boxes is None else max_boxes)
        check_single_camera_keys(c)
        check_stream_maps(c)
        from vad_datasets import frame_size
        from vec_vad_amd.trainer import FusedTrainer
        cp, ds, method = c['cp'], c['dataset_name'], c['method']
        if cp.get(method, 'border_mode') != 'predict':
            raise ValueError("a stream scores with border_mode = predict only (a centred window needs frames that have not arrived), got "
                             "{!r}".format(cp.get(method, 'border_mode')))
        H, W, C = (int(v) for v in frame_shape)
        if C not in (1, 3):
            raise ValueError('frames must have 1 or 3 channels, got frame_shape {!r}'.format(tuple(frame_shape)))
        self.H, self.W, self.C = H, W, C
        self.sched = MultiSchedule(self.cameras, cp.getint(method, 'context_frame_num'), cp.getint(method, 'context_of_num'))
        self.P = cp.getint(ds, 'patch_size')
        self.thr = cp.getfloat(ds, 'motionThr')
        self.hb, self.wb = c['h_block'], c['w_block']
        self.grid_h, self.grid_w = frame_size[ds][0], frame_size[ds][1]
        self.h_step, self.w_step = self.grid_h / self.hb, self.grid_w / self.wb
        self.block_mode = cp.getint(ds, 'test_block_mode')
        self.w_raw, self.w_of, self.use_flow = float(c['w_raw']), float(c['w_of']), bool(c['useFlow'])
        dev = torch.device(device)
        self.device = dev = dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())
        if flownet2 is None:
            from calc_optical_flow import load_flownet2
            flownet2 = load_flownet2(c['flownet2_checkpoint'], device=dev, fp16=c['direct_flow_fp16'])
        from calc_optical_flow import FLOW_H, FLOW_W
        self.flow_h, self.flow_w = FLOW_H, FLOW_W
        self.flow_in, self.flow_out, self.flow_graph = flownet2.graph_entry((self.cameras, 3, 2, FLOW_H, FLOW_W))
        self.flownet2 = flownet2
        sc, cams, cap, P = self.sched, self.cameras, self.cap, self.P
        self.raw_ring = torch.zeros((cams * sc.R, H, W, C), dtype=torch.uint8, device=dev)
        self.flow_ring = torch.zeros((cams * sc.Rf, H, W, 2), dtype=torch.float32, device=dev)
        self.store_raw = torch.zeros((cams * cap, sc.T, P, P, C), dtype=torch.uint8, device=dev)
        self.store_flow = torch.zeros((cams * cap, sc.Tf, P, P, 2), dtype=torch.float32, device=dev)
        self.idx = torch.arange(cams * cap, dtype=torch.long, device=dev)
        # per block of the grid: (trainer, device statistics) or None for a block without a model -- built as StreamScorer does
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
                stats = torch.from_numpy(np.array([st_r[0], st_r[1], st_o[0], st_o[1]], np.float64)).to(dev)
                self.blocks[(hh, ww)] = (trainers[id(net)], stats)
        self.lay = TickLayout(cams, cap, sc.T, sc.Tf, self.hb, self.wb)
        self.desc = torch.zeros(self.lay.words(1), dtype=torch.int32, device=dev)       # grows with the rounds of a tick
        self.staging = _Staging()
        self.held = [None] * cams         # per camera: (boxes, crops, blocks, None) of the frame that waits for its look-ahead
        self.frames = [0] * cams          # per camera: frames pushed so far, across videos
        # warm-up: every engine runs its eager launches and captures its graph here, so that a tick only replays
        for ent in self.blocks.values():
            if ent is not None:
                for _ in range(3):
                    ent[0].score_cubes(self.store_raw, self.store_flow, self.idx)
        torch.cuda.synchronize(dev)

    @classmethod
    def from_config(cls, config_path='config.cfg', cameras=None, frame_shape=None, flownet2=None, scene=None):
        """The scorer of a configuration, as ``StreamScorer.from_config``; ``cameras`` None reads ``[mi355x] stream_cameras``.  A bad
        key raises before any GPU work."""
        from train import build_network, read_config
        c = read_config(config_path)
        cameras = check_cameras(c['stream_cameras'] if cameras is None else cameras)
        check_single_camera_keys(c)
        check_stream_maps(c)
        from test import load_artifacts
        from vad_datasets import frame_size
        ds = c['dataset_name']
        device = torch.device('cuda', torch.cuda.current_device())
        base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
        net_set, st_r, st_o = load_artifacts(base, c['mode_fg'], c['method'], ds == 'ShanghaiTech', lambda: build_network(c), device,
                                             c['h_block'], c['w_block'])
        if frame_shape is None:
            frame_shape = (frame_size[ds][0], frame_size[ds][1], 3)
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
            frame = ready[k][0]
            st = self.staging.get('frame', frame.shape, torch.uint8)
            st[0].numpy()[...] = frame
            self.raw_ring[slot].copy_(st[0], non_blocking=True)
            st[1] = torch.cuda.Event()
            st[1].record()
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

    def _flow(self, base, stream):
        """The flow fields of the issued frames, in place in the flow ring: the launches of ``calc_optical_flow.chunk_flows`` at
        ``cameras`` pairs, their tables read from the descriptor."""
        lib, sc, cams, lay = _lib.lib(), self.sched, self.cameras, self.lay
        _lib.check(lib.vv_flow_pairs_prep(self.raw_ring.data_ptr(), cams * sc.R, self.H, self.W, self.C, base + 4 * lay.h_pairs, cams,
                                          self.flow_h, self.flow_w, self.flow_in.data_ptr(), stream), 'vv_flow_pairs_prep')
        self.flow_graph.replay()
        _lib.check(lib.vv_flow_resize_back(self.flow_out.data_ptr(), cams, self.flow_h, self.flow_w, base + 4 * lay.h_rows, self.H, self.W,
                                           self.flow_ring.data_ptr(), cams * sc.Rf, stream), 'vv_flow_resize_back')

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
        cams, cap, lay = self.cameras, self.cap, self.lay
        d, rounds, rows, used = tick_descriptor(lay, [(k, issue, held[1], held[2]) for k, issue, held, _ in issued])
        words = len(d)
        if self.desc.numel() < words:
            self.desc = torch.zeros(words, dtype=torch.int32, device=self.device)
        st = self.staging.get('desc', (words,), torch.int32)
        st[0].numpy()[:] = d
        desc = self.desc
        desc[:words].copy_(st[0], non_blocking=True)
        st[1] = torch.cuda.Event()
        st[1].record()
        self._flow(desc.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream)
        width = rounds * cap
        stride = 1 + len(rows) * width                    # per camera: the frame's cell, then its [rows][width] box scores
        # the tick's results in ONE buffer, so that the read-back is one copy: float64 [cams][stride] | keep uint8 [rounds][cams*cap]
        nb = 8 * cams * stride
        buf = torch.empty(nb + max(rounds, 1) * cams * cap, dtype=torch.uint8, device=self.device)
        out, keep = buf[:nb].view(torch.float64), buf[nb:].view(max(rounds, 1), cams * cap)
        out.fill_(-float(BIG))
        keep.zero_()
        for r in range(rounds):
            rnd = desc[lay.head + r * lay.D:lay.head + (r + 1) * lay.D]
            masks = rnd[lay.w_mask:].view(torch.uint8)
            n = rnd[0:cams]
            stream_cut_multi(self.raw_ring, self.flow_ring, cams, n, rnd[lay.w_crops:lay.w_rwin], rnd[lay.w_rwin:lay.w_fwin],
                             rnd[lay.w_fwin:lay.w_fwin + cams * lay.Tf], self.thr, self.store_raw, self.store_flow, keep[r])
            for i in used[r]:
                self._score_block(rows[i], keep[r], n, masks, out[1 + i * width + r * cap:], out, stride)
        host_buf = torch.empty(buf.shape, dtype=torch.uint8, pin_memory=True)
        host_buf.copy_(buf, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        host, host_keep = host_buf[:nb].view(torch.float64), host_buf[nb:].view(max(rounds, 1), cams * cap)
        return [MultiStreamResult(k, frame, held[0], len(held[1]), len(rows), width, cap, rounds, stride, host, host_keep, event)
                for k, _, held, frame in issued]
