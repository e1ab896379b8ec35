#!/usr/bin/env python
"""``python train.py`` -- normal-event modelling stage of VEC_VAD on the MI355X UNet-bank engine.

Drop-in for the reference's train.py:239-437 ("Normal video event modeling"): same ``config.cfg`` keys, same input
artifacts (``<data_root>/<modality>/<ds>_foreground_train_<mode>-raw.npy / -flow.npy``, ShanghaiTech segment files)
and same outputs (``<ds>_model_<mode>_SelfComplete.npy`` = torch-pickled nested list of ``state_dict`` with the
DataParallel ``module.`` key prefix, ``<ds>_{raw,of}_training_scores_<mode>_SelfComplete.npy``).

What is different on purpose:
  * the cubes are uploaded once and stay on the GPU in their on-disk layout; batches are gathered by a HIP kernel
    (no DataLoader / ToTensor / H2D copy per step, reference train.py:372-381);
  * forward + backward + Adam are the fused HIP path (vec_vad_amd.trainer.FusedTrainer); no per-step ``.item()`` sync
    -- the running losses are accumulated on the device and fetched only when a log line is printed;
  * ``torchrun --nproc-per-node N train.py`` gives one process per GPU with RCCL gradient all-reduce instead of
    nn.DataParallel; plain ``python train.py`` stays valid (1 GPU);
  * the epoch permutation is seeded (``[mi355x] shuffle_seed``) -- the reference shuffles unseeded.
Cube extraction (train.py:102-226) runs through ``foreground.extract_train`` (crop + resize on the GPU) when
``train_foreground_saved = False``.  With ``train_bbox_saved = False`` the boxes of the detector-free modes are computed first
(``foreground.load_bboxes``: 'frame', 'simple_patch', and 'obj_det_with_motion' = the rows of ``bboxes_train_obj_det.npy``, if
that file exists, plus the motion boxes found on the GPU); the mmdet detector itself (train.py:44-67) is not part of this build,
so mode 'obj_det' needs its bbox file.

``[mi355x] direct_train = True`` (default False; UCSDped2 / avenue) trains straight from frames and boxes:
``foreground.extract_train_device`` cuts the kept cubes of the whole training split into ONE device-resident store
(``foreground.extract_device`` with ``mode='train'``: many frames per launch, every frame decoded once per chunk) and every (h, w)
block trains from ``(store_raw, store_flow, block_idx)`` -- its index list of ``foreground.block_groups`` -- through the same loop.
No ``foreground_train_*`` file is written or read; the three output files are, bit for bit, those of the staged route with the same
``shuffle_seed``.  With ``direct_flow = True`` as well the flow of every chunk is computed on the GPU and nothing under
``optical_flow/<ds>/Train...`` is read (``main(config_path, flownet2=None)`` takes the network; None loads
``[mi355x] flownet2_checkpoint``).  Under ``torchrun`` every rank runs that extraction itself and holds the full store: no
side-group barrier, no shared filesystem, but every rank decodes every frame (cost not measured).
"""
import os
import sys
from configparser import ConfigParser

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from model.unet import SelfCompleteNet4, SelfCompleteNetFull  # noqa: E402
from vad_datasets import CubeStore  # noqa: E402
from vec_vad_amd.trainer import FusedTrainer, shard_batch  # noqa: E402


class AverageMeter:
    """Running average of the per-batch losses (reference helper/misc.py AverageMeter; never reset, train.py:365)."""

    def __init__(self, device):
        self.sum = torch.zeros((), device=device, dtype=torch.float64)
        self.count = 0

    def update(self, val, n):
        self.sum += val.double() * n
        self.count += n

    @property
    def avg(self):
        return float(self.sum) / max(1, self.count)


# [mi355x] direct_max_cubes default.  A cube of the 5raw+5of bank is 5*32*32*3 B (uint8 raw) + 5*32*32*2*4 B (float32 flow) =
# 15 360 + 40 960 = 56 320 B; 524 288 cubes are 29.5e9 B (27.5 GiB), below 32 GB.  (5raw+1of: 23 552 B per cube, 12.3e9 B.)
DIRECT_MAX_CUBES = 524288
DIRECT_TRAIN_SHANGHAI = ('[mi355x] direct_train = True does not cover ShanghaiTech (one model per scene, training cubes in randomly '
                         'ordered saveSegNum segments): set it to False to train from the staged segment files')


def read_config(path='config.cfg'):
    cp = ConfigParser()
    if not cp.read(path):
        raise FileNotFoundError(path)
    method = cp.get('shared_parameters', 'method')
    ds = cp.get('shared_parameters', 'dataset_name')
    c = dict(cp=cp, dataset_name=ds, raw_dataset_dir=cp.get('shared_parameters', 'raw_dataset_dir'),
             mode_fg=cp.get('shared_parameters', 'foreground_extraction_mode'),
             data_root_dir=cp.get('shared_parameters', 'data_root_dir'), modality=cp.get('shared_parameters', 'modality'),
             method=method, h_block=cp.getint(ds, 'h_block'), w_block=cp.getint(ds, 'w_block'))
    if method != 'SelfComplete':
        raise NotImplementedError(method)
    border_mode = cp.get(method, 'border_mode')
    if border_mode == 'predict':                       # train.py:246-251
        tot_frame = cp.getint(method, 'context_frame_num') + 1
        tot_of = cp.getint(method, 'context_of_num') + 1
    else:
        tot_frame = 2 * cp.getint(method, 'context_frame_num') + 1
        tot_of = 2 * cp.getint(method, 'context_of_num') + 1
    raw_range = cp.getint(method, 'rawRange')
    if raw_range >= tot_frame:                         # train.py:252-254
        raw_range = None
    c.update(border_mode=border_mode, tot_frame_num=tot_frame, tot_of_num=tot_of, rawRange=raw_range,
             epochs=cp.getint(method, 'epochs'), batch_size=cp.getint(method, 'batch_size'),
             useFlow=cp.getboolean(method, 'useFlow'), padding=cp.getboolean(method, 'padding'),
             lambda_raw=cp.getfloat(method, 'lambda_raw'), lambda_of=cp.getfloat(method, 'lambda_of'),
             w_raw=cp.getfloat(method, 'w_raw'), w_of=cp.getfloat(method, 'w_of'), nf=cp.getint(method, 'nf'),
             shuffle_seed=cp.getint('mi355x', 'shuffle_seed', fallback=0),
             score_batch=cp.getint('mi355x', 'score_batch', fallback=2048),
             save_score_masks=cp.getboolean('mi355x', 'save_score_masks', fallback=True),
             overlap_wgrad=cp.getboolean('mi355x', 'overlap_wgrad', fallback=False),
             precision=cp.get('mi355x', 'precision', fallback='fp32').strip().lower(),
             direct_test=cp.getboolean('mi355x', 'direct_test', fallback=False),
             direct_train=cp.getboolean('mi355x', 'direct_train', fallback=False),
             direct_frames_per_chunk=cp.getint('mi355x', 'direct_frames_per_chunk', fallback=64),
             direct_max_cubes=cp.getint('mi355x', 'direct_max_cubes', fallback=DIRECT_MAX_CUBES),
             direct_flow=cp.getboolean('mi355x', 'direct_flow', fallback=False),
             direct_flow_pairs=cp.getint('mi355x', 'direct_flow_pairs', fallback=4),
             direct_flow_fp16=cp.getboolean('mi355x', 'direct_flow_fp16', fallback=False),
             flownet2_checkpoint=cp.get('mi355x', 'flownet2_checkpoint', fallback=None),
             pixel_criterion=cp.getboolean('mi355x', 'pixel_criterion', fallback=False),
             pixel_overlap_percent=cp.getint('mi355x', 'pixel_overlap_percent', fallback=40),
             device_score_masks=cp.getboolean('mi355x', 'device_score_masks', fallback=False),
             pixel_maps=cp.getboolean('mi355x', 'pixel_maps', fallback=False),
             region_criterion=cp.getboolean('mi355x', 'region_criterion', fallback=False),
             region_iou_percent=cp.getint('mi355x', 'region_iou_percent', fallback=10),
             track_percent=cp.getint('mi355x', 'track_percent', fallback=10),
             smooth_masks=cp.getboolean('mi355x', 'smooth_masks', fallback=False),
             smooth_frames=cp.getint('mi355x', 'smooth_frames', fallback=5),
             smooth_pixels=cp.getint('mi355x', 'smooth_pixels', fallback=9),
             auc_statistics=cp.getboolean('mi355x', 'auc_statistics', fallback=False),
             auc_bootstrap=cp.getint('mi355x', 'auc_bootstrap', fallback=1000),
             auc_bootstrap_unit=cp.get('mi355x', 'auc_bootstrap_unit', fallback='block').strip().lower(),
             auc_bootstrap_block=cp.getint('mi355x', 'auc_bootstrap_block', fallback=25),
             auc_bootstrap_seed=cp.getint('mi355x', 'auc_bootstrap_seed', fallback=0),
             auc_confidence=cp.getint('mi355x', 'auc_confidence', fallback=95),
             render=cp.getboolean('mi355x', 'render', fallback=False),
             render_source=cp.get('mi355x', 'render_source', fallback='score').strip().lower(),
             render_alpha=cp.getint('mi355x', 'render_alpha', fallback=50),
             render_range=cp.get('mi355x', 'render_range', fallback='auto').strip().lower(),
             render_every=cp.getint('mi355x', 'render_every', fallback=1),
             render_boxes=cp.getboolean('mi355x', 'render_boxes', fallback=True),
             render_flow=cp.getboolean('mi355x', 'render_flow', fallback=False),
             render_flow_max=cp.getfloat('mi355x', 'render_flow_max', fallback=0.0),
             stream_max_boxes=cp.get('mi355x', 'stream_max_boxes', fallback='64').strip(),
             stream_boxes=cp.get('mi355x', 'stream_boxes', fallback='given').strip().lower(),
             stream_cameras=cp.get('mi355x', 'stream_cameras', fallback='1').strip(),
             collect_max_cubes=cp.get('mi355x', 'collect_max_cubes', fallback='65536').strip(),
             stream_masks=cp.getboolean('mi355x', 'stream_masks', fallback=False),
             stream_smooth=cp.getboolean('mi355x', 'stream_smooth', fallback=False),
             stream_render=cp.getboolean('mi355x', 'stream_render', fallback=False),
             stream_tracks=cp.getboolean('mi355x', 'stream_tracks', fallback=False),
             stream_maps=cp.getboolean('mi355x', 'stream_maps', fallback=False),
             track_iou_percent=cp.getint('mi355x', 'track_iou_percent', fallback=30),
             track_max_age=cp.getint('mi355x', 'track_max_age', fallback=5),
             track_window=cp.getint('mi355x', 'track_window', fallback=8),
             track_min_hits=cp.getint('mi355x', 'track_min_hits', fallback=3),
             stream_max_tracks=cp.getint('mi355x', 'stream_max_tracks', fallback=128))
    for key in ('pixel_overlap_percent', 'region_iou_percent', 'track_percent'):
        if not 1 <= c[key] <= 100:
            raise ValueError('[mi355x] {} must be an integer in 1..100, got {}'.format(key, c[key]))
    for key in ('smooth_frames', 'smooth_pixels'):      # the windows of vv_smooth_masks (VV_SMOOTH_MAX), checked whatever the switch says
        if not 1 <= c[key] <= 33 or c[key] % 2 == 0:
            raise ValueError('[mi355x] {} must be an odd integer in 1..33, got {}'.format(key, c[key]))
    # the settings of scoring.auc_bootstrap ([mi355x] auc_statistics), checked whatever the switch says
    if c['auc_bootstrap'] < 0:
        raise ValueError('[mi355x] auc_bootstrap must be a number of replicates >= 0, got {}'.format(c['auc_bootstrap']))
    if c['auc_bootstrap_unit'] not in ('block', 'video'):
        raise ValueError("[mi355x] auc_bootstrap_unit must be 'block' or 'video', got {!r}".format(c['auc_bootstrap_unit']))
    if c['auc_bootstrap_block'] < 1:
        raise ValueError('[mi355x] auc_bootstrap_block must be a number of frames >= 1, got {}'.format(c['auc_bootstrap_block']))
    if not 0 <= c['auc_bootstrap_seed'] < 2 ** 64:
        raise ValueError('[mi355x] auc_bootstrap_seed must be an integer in 0..2^64-1, got {}'.format(c['auc_bootstrap_seed']))
    if not 50 <= c['auc_confidence'] <= 99:
        raise ValueError('[mi355x] auc_confidence must be an integer in 50..99, got {}'.format(c['auc_confidence']))
    # the settings of the render stage ([mi355x] render), checked whatever the switch says
    if c['render_source'] not in ('score', 'smooth'):
        raise ValueError("[mi355x] render_source must be 'score' or 'smooth', got {!r}".format(c['render_source']))
    if not 0 <= c['render_alpha'] <= 100:
        raise ValueError('[mi355x] render_alpha must be an integer percent in 0..100, got {}'.format(c['render_alpha']))
    if c['render_range'] != 'auto':
        try:
            lo, hi = (float(t) for t in c['render_range'].split(','))
        except ValueError:
            lo = hi = float('nan')
        if not lo < hi or not abs(lo) < float('inf') or not abs(hi) < float('inf'):
            raise ValueError("[mi355x] render_range must be 'auto' or two finite numbers lo,hi with lo < hi, got {!r}".format(c['render_range']))
        c['render_range'] = (lo, hi)
    if c['render_every'] < 1:
        raise ValueError('[mi355x] render_every must be a frame stride >= 1, got {}'.format(c['render_every']))
    if not c['render_flow_max'] >= 0 or c['render_flow_max'] == float('inf'):
        raise ValueError('[mi355x] render_flow_max must be a finite radius >= 0 (0: every image by its own), got {}'.format(c['render_flow_max']))
    if c['render'] and c['render_source'] == 'smooth' and not c['smooth_masks']:
        raise ValueError('[mi355x] render_source = smooth needs smooth_masks = True: only that stage forms the smoothed masks')
    # cubes per scoring launch of a streamed frame (stream.py), checked whatever route runs
    try:
        c['stream_max_boxes'] = int(c['stream_max_boxes'])
    except ValueError:
        pass
    if not isinstance(c['stream_max_boxes'], int) or c['stream_max_boxes'] < 1:
        raise ValueError('[mi355x] stream_max_boxes must be an integer >= 1, got {!r}'.format(c['stream_max_boxes']))
    # where a streamed frame's boxes come from: the caller, or the motion stage on the device
    from vec_vad_amd.stream import check_stream_boxes, check_track_settings
    c['stream_boxes'] = check_stream_boxes(c['stream_boxes'])
    check_track_settings(c, None)                      # the settings of a stream's tracks, checked whatever the switch says
    from vec_vad_amd.multistream import check_cameras
    c['stream_cameras'] = check_cameras(c['stream_cameras'])      # cameras per scorer of stream.py, checked whatever route runs
    from vec_vad_amd.stream_train import check_max_cubes
    c['collect_max_cubes'] = check_max_cubes(c['collect_max_cubes'])      # cubes a StreamCollector's store holds (stream_train.py)
    if c['flownet2_checkpoint'] is None:
        from calc_optical_flow import CHECKPOINT
        c['flownet2_checkpoint'] = CHECKPOINT
    assert c['modality'] == 'raw2flow'
    return c


def build_network(c):
    """train.py:261-268 / test.py:216-224."""
    os.environ['VV_PRECISION'] = c.get('precision', 'fp32')       # read by the UNet bank when it is built ([mi355x] precision)
    kw = dict(features_root=c['nf'], tot_raw_num=c['tot_frame_num'], tot_of_num=c['tot_of_num'],
              border_mode=c['border_mode'], rawRange=c['rawRange'], useFlow=c['useFlow'], padding=c['padding'])
    if c['tot_of_num'] == 1:
        net = SelfCompleteNet4(**kw)
    elif c['tot_of_num'] == 5:
        net = SelfCompleteNetFull(**kw)
    else:
        raise NotImplementedError('context_of_num must be 0 or 4 (config.cfg; the reference falls through at train.py:266)')
    assert c['tot_frame_num'] == 5
    return net


def _dist():
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1:
        return None, 0, 1
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
    return dist, dist.get_rank(), dist.get_world_size()


class StoreView:
    """The cubes ``idx`` (int64 list, repeats between views allowed) of a device-resident store, seen as a cube set of its own:
    ``len`` cubes, ``take(sel)`` = the store indices of the view's cubes ``sel``.  ``CubeStore`` is the view of a whole store."""

    def __init__(self, raw, flow, idx, device='cuda'):
        self.raw, self.flow = raw, flow
        idx = idx if torch.is_tensor(idx) else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
        self.idx = idx.to(device=device, dtype=torch.int64)
        if self.idx.numel() and not 0 <= int(self.idx.min()) <= int(self.idx.max()) < raw.shape[0]:
            raise IndexError('block index list names cube %d / %d of a store of %d cubes'
                             % (int(self.idx.min()), int(self.idx.max()), raw.shape[0]))

    def __len__(self):
        return int(self.idx.numel())

    def take(self, sel):
        return self.idx[sel]


def _extract_once(c, device, dist=None, timeout_h=48.0):
    """Rank 0 cuts the training cubes (train.py:102-226); every other rank of the job waits for it.

    The wait is a barrier on a gloo SIDE group with its own, long, explicit timeout -- cutting a large dataset takes longer than
    the default collective timeout, and the RCCL group must not carry a 48 h watchdog for its real collectives.  No marker
    files: nothing survives a crash or a ``torchrun --max-restarts`` restart that a later attempt could mistake for "done", and
    the .npy files are written atomically (foreground.save_nested: tmp + os.replace), so a rank that gets past the barrier reads
    complete files.  All ranks must see ``data_root_dir`` (one node, or a shared filesystem); the ranks check that after the
    barrier instead of assuming it."""
    rank = dist.get_rank() if dist is not None else 0
    if dist is None:
        from foreground import extract_train
        extract_train(c, device)
        return
    import datetime
    side = dist.new_group(backend='gloo', timeout=datetime.timedelta(hours=timeout_h))
    err = None
    try:
        if rank == 0:
            try:
                from foreground import extract_train
                extract_train(c, device)
            except BaseException as e:      # incl. KeyboardInterrupt / SystemExit: the other ranks must not wait 48 h for a rank that
                err = e                     # is on its way out (a SIGKILL cannot be announced: gloo then fails the peers' broadcast
                                            # when the socket closes)
        flag = torch.tensor([1 if err is not None else 0], dtype=torch.int32)
        dist.broadcast(flag, src=0, group=side)          # = the barrier; carries rank 0's verdict
    finally:
        dist.destroy_process_group(side)                 # also when the broadcast itself raised
    if err is not None:
        raise err
    if int(flag.item()):
        raise RuntimeError('rank 0 failed while extracting the training cubes')
    base = os.path.join(c['data_root_dir'], c['modality'], c['dataset_name'] + '_')
    fg = c['mode_fg']
    probe = base + ('foreground_train_{}_seg_0-raw.npy' if c['dataset_name'] == 'ShanghaiTech' else 'foreground_train_{}-raw.npy').format(fg)
    if not os.path.exists(probe):
        raise RuntimeError('rank %d cannot see %s: train.py under torchrun needs data_root_dir on a filesystem every rank mounts'
                           % (rank, probe))


def train_block(net, segments, epochs, batch_size, lambda_raw=1.0, lambda_of=1.0, shuffle_seed=0, device='cuda',
                log=print, tag='(0, 0)', dist=None, overlap=False):
    """The loop of train.py:375-427 for one (h, w) block.

    ``segments``: list of callables returning (raw uint8 [N,5,32,32,3], flow fp32 [N,(Tf,)32,32,2]) -- one entry for
    UCSDped2 / avenue, ``totSegNum`` entries for ShanghaiTech (train.py:292-299).  An entry may instead be a tuple
    ``(store_raw, store_flow, block_idx)``: the block's cubes are ``store[block_idx]`` of a device-resident store in ``CubeStore``
    layout (``[mi355x] direct_train``); ``block_idx`` (int64, numpy or device tensor) is uploaded once, the epoch permutation
    indexes it and the scoring pass walks it in order, so the steps see the cubes a callable returning ``store[block_idx]`` gives.
    Returns (state_dict with 'module.' prefixed keys, raw_scores [N_total], of_scores [N_total])."""
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist is not None else (0, 1)
    net = net.to(device)
    net.train()
    trainer = FusedTrainer(net, lr=1e-3, eps=1e-7, lambda_raw=lambda_raw, lambda_of=lambda_of,
                           process_group=dist.group.WORLD if dist is not None else None, overlap=overlap)
    raw_losses, of_losses = AverageMeter(device), AverageMeter(device)
    rng = np.random.default_rng(shuffle_seed) if shuffle_seed is not None and shuffle_seed >= 0 else None
    stores = [None] * len(segments)

    def store(i):
        if not callable(segments[i]):
            if stores[i] is None:
                stores[i] = StoreView(*segments[i], device=device)
            return stores[i]
        if stores[i] is None or len(segments) > 1:
            if len(segments) > 1:
                trainer.release_graphs()      # the captured steps pin the previous segment's store: free it before the next upload
            raw, flow = segments[i]()
            s = CubeStore(raw, flow, device)
            if len(segments) == 1:
                stores[i] = s
            return s
        return stores[i]

    for epoch in range(epochs):
        for si in range(len(segments)):
            st = store(si)
            n = len(st)
            perm = rng.permutation(n) if rng is not None else np.arange(n)
            perm = torch.from_numpy(perm).to(device)
            nb = (n + batch_size - 1) // batch_size
            for idx in range(nb):
                bidx = st.take(perm[idx * batch_size:(idx + 1) * batch_size])   # the last partial batch is kept (train.py:373)
                n_glob = int(bidx.numel())
                if world > 1:
                    if n_glob % world == 0:
                        bidx = shard_batch(bidx, rank, world)
                        ws = trainer.step_cubes(st.raw, st.flow, bidx)
                    else:       # DataParallel's uneven scatter (chunks of ceil(n / world), trailing replicas may get nothing)
                        per = -(-n_glob // world)
                        bidx = bidx[rank * per:(rank + 1) * per]
                        ws = trainer.step_cubes_uneven(st.raw, st.flow, bidx, n_glob)
                else:
                    ws = trainer.step_cubes(st.raw, st.flow, bidx)           # a single cube is a valid batch (BatchNorm over H x W)
                if ws is not None:
                    l_raw, l_of = trainer.losses(ws)
                    raw_losses.update(l_raw, bidx.numel())
                    of_losses.update(l_of if l_of is not None else torch.zeros((), device=device), bidx.numel())
                if idx % 5 == 0:
                    avg_r, avg_o = _global_avg(dist, raw_losses, of_losses, device)      # every rank takes part; rank 0 prints
                    if rank == 0:
                        log('Block: {}, epoch {}, seg {}, batch {} of {}, raw loss: {}, of loss: {}'.format(
                            tag, epoch, si, idx, n // batch_size, avg_r, avg_o))
    # DataParallel keeps replica 0's BatchNorm statistics (train.py:375): every rank scores with -- and rank 0 saves -- those
    trainer.sync_from_rank0(params=False)
    sd = {('module.' + k): v.detach().clone() for k, v in net.state_dict().items()}     # train.py:410 (DataParallel keys)

    # A forward pass to store the training scores (train.py:413-427), eval mode, shuffle=False
    net.eval()
    rs, os_ = [], []
    for si in range(len(segments)):
        st = store(si)
        n = len(st)
        lo, hi = (rank * n) // world, ((rank + 1) * n) // world
        r_loc, o_loc = [], []
        for s in range(lo, hi, batch_size):
            idx = st.take(torch.arange(s, min(hi, s + batch_size), device=device))
            r, o = trainer.score_cubes(st.raw, st.flow, idx)
            r_loc.append(r.clone())
            if o is not None:
                o_loc.append(o.clone())
        r_loc = torch.cat(r_loc) if r_loc else torch.zeros(0, device=device)
        o_loc = torch.cat(o_loc) if o_loc else torch.zeros(0, device=device)
        if world > 1:
            r_loc, o_loc = _gather_var(dist, r_loc, n, world), _gather_var(dist, o_loc, n, world, net.useFlow)
        rs.append(r_loc.cpu().numpy())
        os_.append(o_loc.cpu().numpy())
    return sd, np.concatenate(rs), np.concatenate(os_)


def _global_avg(dist, raw_m, of_m, device):
    """running-average losses over ALL ranks' shards (the reference logs the loss of the whole batch, train.py:394-399)."""
    if dist is None:
        return raw_m.avg, of_m.avg
    t = torch.stack([raw_m.sum, of_m.sum, torch.tensor(float(raw_m.count), device=device, dtype=torch.float64)])
    dist.all_reduce(t)
    cnt = max(1.0, float(t[2]))
    return float(t[0]) / cnt, float(t[1]) / cnt


def _gather_var(dist, t, n, world, present=True):
    """all-gather of per-rank contiguous score shards (tiny; no collective in the math).  present=False: this score does not
    exist (useFlow = False) -> empty on every rank."""
    if not present or (t.numel() == 0 and n == 0):
        return t[:0]
    mx = (n + world - 1) // world + 1
    pad = torch.zeros(mx, device=t.device, dtype=t.dtype)
    pad[:t.numel()] = t
    out = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(out, pad)
    parts = []
    for r in range(world):
        lo, hi = (r * n) // world, ((r + 1) * n) // world
        parts.append(out[r][:hi - lo])
    return torch.cat(parts)


def _training_blocks(c, base, store=None):
    """The one place that tells the three routes apart: ``(scenes, rows, blocks)``.  The saved files nest ``[h][w]``, ``rows[h]`` blocks
    in grid row ``h``, below ``scenes`` scenes for ShanghaiTech (else None).  ``blocks`` yields ``((s, h, w), segments)`` in training order,
    ``segments`` as ``train_block`` takes them: the block's index list into ``store`` (``extract_train_device``), ShanghaiTech's segment
    files (train.py:292-299), or the block's arrays of the ``foreground_train_*`` files.  A block with <= 1 cube is left out
    (train.py:370 "num > 1 for data parallel"); a ShanghaiTech block never is."""
    ds, fg, hb, wb = c['dataset_name'], c['mode_fg'], c['h_block'], c['w_block']
    if store is not None:
        def blocks():
            for h, w in ((h, w) for h in range(hb) for w in range(wb)):
                block_idx = store['groups'][(None, h, w)][0] if (None, h, w) in store['groups'] else np.zeros(0, np.int64)
                if len(block_idx) > 1:
                    yield (None, h, w), [(store['raw'], store['flow'], block_idx)]
        return None, [wb] * hb, blocks()
    if ds == 'ShanghaiTech':
        tot_seg = len([f for f in os.listdir(os.path.dirname(base))
                       if f.startswith('%s_foreground_train_%s_seg_' % (ds, fg)) and f.endswith('-raw.npy')])
        probe = np.load(base + 'foreground_train_{}_seg_0-raw.npy'.format(fg), allow_pickle=True)
        grid = [(s, h, w) for s in range(len(probe)) for h in range(len(probe[s])) for w in range(len(probe[s][h]))]
        del probe

        def seg_loader(k, s, h, w):
            a = np.load(base + 'foreground_train_{}_seg_{}-raw.npy'.format(fg, k), allow_pickle=True)
            b = np.load(base + 'foreground_train_{}_seg_{}-flow.npy'.format(fg, k), allow_pickle=True)
            return np.asarray(a[s][h][w]), np.asarray(b[s][h][w])
        return max(g[0] for g in grid) + 1, [wb] * hb, (
            (g, [lambda k=k, g=g: seg_loader(k, *g) for k in range(tot_seg)]) for g in grid)
    fset = np.load(base + 'foreground_train_{}-raw.npy'.format(fg), allow_pickle=True)
    fset2 = np.load(base + 'foreground_train_{}-flow.npy'.format(fg), allow_pickle=True)

    def blocks():
        for h, w in ((h, w) for h in range(len(fset)) for w in range(len(fset[h]))):
            data = np.asarray(fset[h][w])
            if len(data) > 1:
                data2 = np.asarray(fset2[h][w])
                yield (None, h, w), [lambda data=data, data2=data2: (data, data2)]
    return None, [len(row) for row in fset], blocks()


def _train_blocks(c, net, scenes, rows, blocks, device, dist=None, log=print):
    """The block loop of ``main``: ``train_block`` on every ``((s, h, w), segments)`` of ``_training_blocks``, ``net`` carried from
    block to block as the reference carries it.  Returns the three nested lists that are saved: ``(model_set, raw_scores_set,
    of_scores_set)``, ``[h][w]`` (below ``[scene]`` for ShanghaiTech), empty lists where a block was left out."""
    def nested():
        def grid():
            return [[[] for _ in range(n)] for n in rows]
        return grid() if scenes is None else [grid() for _ in range(scenes)]

    model_set, raw_scores_set, of_scores_set = nested(), nested(), nested()
    for (s, h, w), segments in blocks:
        sd, r, o = train_block(net, segments, c['epochs'], c['batch_size'], c['lambda_raw'], c['lambda_of'],
                               c['shuffle_seed'], device, log=log, tag='({}, {})'.format(h, w), dist=dist, overlap=c['overlap_wgrad'])
        models, raw_sc, of_sc = ((t if s is None else t[s])[h] for t in (model_set, raw_scores_set, of_scores_set))
        models[w].append({k: v.cpu() for k, v in sd.items()})
        raw_sc[w] = r
        of_sc[w] = o
    return model_set, raw_scores_set, of_scores_set


def train_store(c, store, net, dist=None, log=print):
    """Every (h, w) block trained from a device-resident store: ``store`` is the dict of ``foreground.extract_train_device`` (or of
    ``vec_vad_amd.stream_train.StreamCollector.finish``), each block's cubes its index list ``store['groups'][(None, h, w)]``.
    Returns ``(model_set, raw_scores_set, of_scores_set)``, the three nested lists ``main`` saves."""
    scenes, rows, blocks = _training_blocks(c, None, store)
    return _train_blocks(c, net, scenes, rows, blocks, store['raw'].device, dist, log)


def save_outputs(c, model_set, raw_scores_set, of_scores_set, log=print):
    """The three files of the training stage under ``<data_root_dir>/<modality>/``, written as the reference writes them."""
    base = os.path.join(c['data_root_dir'], c['modality'], c['dataset_name'] + '_')
    fg, method = c['mode_fg'], c['method']
    torch.save(raw_scores_set, base + 'raw_training_scores_{}_{}.npy'.format(fg, method))
    torch.save(of_scores_set, base + 'of_training_scores_{}_{}.npy'.format(fg, method))
    log('training scores saved!')
    torch.save(model_set, base + 'model_{}_{}.npy'.format(fg, method))
    log('Training of {} for dataset: {} has completed!'.format(method, c['dataset_name']))


def main(config_path='config.cfg', flownet2=None):
    """``flownet2``: the network ``[mi355x] direct_flow`` computes the training split's flow with (only with ``direct_train``);
    None loads ``[mi355x] flownet2_checkpoint``."""
    c = read_config(config_path)
    cp, ds, root, mod = c['cp'], c['dataset_name'], c['data_root_dir'], c['modality']
    direct = c['direct_train']
    if direct and ds == 'ShanghaiTech':                         # before any GPU work
        raise NotImplementedError(DIRECT_TRAIN_SHANGHAI)
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(device)
    dist, rank, world = _dist()
    if not direct and not cp.getboolean(ds, 'train_foreground_saved'):      # train.py:102-226, cubes cut on the GPU (vv_crop_resize)
        _extract_once(c, device, dist)
    net = build_network(c)
    base = os.path.join(root, mod, ds + '_')
    store = None
    if direct:          # every rank cuts the whole split into its own store: nothing to wait for, nothing on a shared disk
        # (after build_network: loading FlowNet2 must not move the random state the initial weights are drawn from)
        from foreground import extract_train_device
        store = extract_train_device(c, device, log=print if rank == 0 else (lambda *a: None), flownet2=flownet2)
    if store is not None:
        model_set, raw_scores_set, of_scores_set = train_store(c, store, net, dist)
    else:
        model_set, raw_scores_set, of_scores_set = _train_blocks(c, net, *_training_blocks(c, base), device, dist)
    if rank == 0:
        save_outputs(c, model_set, raw_scores_set, of_scores_set)
    if dist is not None:
        dist.barrier()


if __name__ == '__main__':
    main()
