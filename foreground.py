"""Foreground (cube) extraction stage shared by train.py and test.py -- reference train.py:102-226 and test.py:98-180.

For every frame: decode its temporal context (raw frames and the pre-computed optical flow ``.npy`` fields), cut every
detected box out of every context frame and resize it to ``patch_size`` (ONE ``vv_crop_resize`` launch per modality per
frame instead of one ``cv2.resize`` call per box per frame), drop boxes whose flow energy is below ``motionThr``, and file
the cubes under the grid block(s) the box falls in.  Outputs use the reference's file names and nesting so that either
implementation can consume the other's files.

``extract_train_device`` is the training stage without cube files (``[mi355x] direct_train``): ``extract_device`` in train mode, the
whole split in one store.  ``extract_device`` is the test stage without those files (``[mi355x] direct_test``): many consecutive frames per launch, every
frame decoded and uploaded once per chunk, the motion test on the device (``vv_cube_energy``), and the kept cubes cut straight
into a device-resident store (``vv_cube_cut``) that test.py's ``score_store`` scores through index lists.

The bounding boxes themselves come from ``raw_datasets/<ds>/bboxes_{train,test}_<mode>.npy``.  ``load_bboxes`` writes that
file for the detector-free modes when it is absent (train.py:44-99): 'frame', 'simple_patch' and 'obj_det_with_motion', whose
motion stage runs on the GPU (vec_vad_amd/motion.py) on top of whatever detector output ``bboxes_<mode>_obj_det.npy`` holds.
The mmdet detector itself is not part of this build.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from utils import calc_block_idx
from vad_datasets import frame_size, get_inputs, unified_dataset_interface


def save_nested(path, nested, depth):
    """np.save of a ``depth``-level nested list of arrays as an object array of exactly that nesting (what the
    reference's ``np.save(path, nested_list)`` produced under NumPy < 1.24 whenever the leaves were ragged)."""
    def shape_of(x, d):
        return () if d == 0 else (len(x),) + shape_of(x[0], d - 1)
    arr = np.empty(shape_of(nested, depth), dtype=object)
    for idx in np.ndindex(arr.shape):
        leaf = nested
        for i in idx:
            leaf = leaf[i]
        arr[idx] = np.asarray(leaf)
    # atomic: a reader (another rank, a later run) sees the previous complete file or the new complete file, never a torn one
    final = path if path.endswith('.npy') else path + '.npy'
    tmp = '%s.tmp%d' % (final, os.getpid())
    with open(tmp, 'wb') as f:
        np.save(f, arr, allow_pickle=True)
    os.replace(tmp, final)


def _motion_bboxes(c, mode, ap_path, device, log):
    """'obj_det_with_motion' without a saved file (train.py:62-76): per frame, the appearance boxes (rows of ``ap_path``, the
    file the reference's 'obj_det' mode saves, when it exists; none otherwise) followed by the motion boxes of the frame and
    its two neighbours.  Consecutive frames go through the GPU in chunks: every frame of a chunk is decoded and uploaded once
    and the windows, which repeat frames at video borders ('hard'), are index triples into the chunk."""
    from vec_vad_amd.motion import motion_boxes
    cp, ds = c['cp'], c['dataset_name']
    dataset = unified_dataset_interface(dataset_name=ds, dir=os.path.join(c['raw_dataset_dir'], ds), context_frame_num=1,
                                        mode=mode, border_mode='hard')
    n = len(dataset)
    if os.path.exists(ap_path):
        ap_all = np.load(ap_path, allow_pickle=True)
        if len(ap_all) != n:
            raise ValueError('{} holds boxes of {} frames, the dataset has {}'.format(ap_path, len(ap_all), n))
        ap_all = [np.asarray(b)[:, :4] if np.asarray(b).ndim == 2 else np.zeros((0, 4), np.float32) for b in ap_all]
    else:
        log('no {}: motion boxes only (no appearance boxes)'.format(ap_path))
        ap_all = [np.zeros((0, 4), np.float32) for _ in range(n)]
    per_launch = max(1, cp.getint('mi355x', 'motion_frames_per_launch', fallback=16))
    all_bboxes = []
    for s in range(0, n, per_launch):
        e = min(s + per_launch, n)
        log('Extracting bboxes of frames {}-{}, {} in total'.format(s + 1, e, n))
        ranges = [dataset.context_range(i) for i in range(s, e)]
        used = sorted({f for r in ranges for f in r})
        local = {f: k for k, f in enumerate(used)}
        frames = np.stack([get_inputs(dataset.all_frame_addr[f]) for f in used])             # [F,H,W,C] uint8, BGR
        frames = torch.from_numpy(np.ascontiguousarray(frames)).to(device)
        win = [[local[f] for f in r] for r in ranges]
        mt = motion_boxes(frames, win, ap_all[s:e], ds)
        for i, m in zip(range(s, e), mt):
            all_bboxes.append(np.concatenate((ap_all[i], m), axis=0) if m.shape[0] > 0 else ap_all[i])
    return all_bboxes


def load_bboxes(c, mode, dataset=None, device='cuda', log=print):
    """train.py:44-99 / test.py:50-96.  ``<raw_dataset_dir>/<ds>/bboxes_<mode>_<fg mode>.npy`` is loaded when
    ``<mode>_bbox_saved`` is set or the file exists.  Otherwise the detector-free modes are computed and saved there (an object
    array of per-frame arrays, written atomically):
      frame                 the whole frame (needs ``dataset`` for the frame count)
      simple_patch          the (3,4) and (6,8) patch grids of train.py:81-86, 60 boxes per frame
      obj_det_with_motion   the rows of ``bboxes_<mode>_obj_det.npy`` (what the reference's 'obj_det' mode saves: detector
                            boxes after ``del_cover_bboxes``; first four columns) when that file exists, none otherwise,
                            followed by the motion boxes found on the GPU (vec_vad_amd/motion.py), ``[mi355x]
                            motion_frames_per_launch`` consecutive frames per launch
    'obj_det' itself needs the mmdet detector, which is not part of this build: without a file it raises."""
    cp, ds, fg = c['cp'], c['dataset_name'], c['mode_fg']
    ds_dir = os.path.join(c['raw_dataset_dir'], ds)
    path = os.path.join(ds_dir, 'bboxes_{}_{}.npy'.format(mode, fg))
    if cp.getboolean(ds, '{}_bbox_saved'.format(mode)) or os.path.exists(path):
        return np.load(path, allow_pickle=True)
    if fg == 'frame' and dataset is not None:
        h, w = frame_size[ds][0], frame_size[ds][1]
        boxes = [np.array([[0, 0, w, h]]) for _ in range(len(dataset))]
        np.save(path, boxes)
        return boxes
    if fg == 'simple_patch':
        from fore_det.simple_patch import get_patch_loc
        n = len(dataset) if dataset is not None else len(unified_dataset_interface(
            dataset_name=ds, dir=ds_dir, context_frame_num=1, mode=mode, border_mode='hard'))
        h, w = frame_size[ds][0], frame_size[ds][1]
        grid = np.concatenate([get_patch_loc(h, w, h_num, w_num) for h_num, w_num in ((3, 4), (6, 8))], axis=0)
        boxes = [grid.copy() for _ in range(n)]
    elif fg == 'obj_det_with_motion':
        boxes = _motion_bboxes(c, mode, os.path.join(ds_dir, 'bboxes_{}_obj_det.npy'.format(mode)), device, log)
    else:
        raise NotImplementedError(
            '{}_bbox_saved = False with mode {!r}: the object detector (reference train.py:44-95: mmdet cascade R-CNN, '
            'fore_det.get_ap_bboxes) is not part of this build; produce {} with the reference once.'.format(mode, fg, path))
    save_nested(path, boxes, 1)
    log('bboxes for {}ing data saved!'.format(mode))
    return np.load(path, allow_pickle=True)


def _datasets(c, mode, all_bboxes, direct_flow=False):
    """The raw and the flow dataset of the stage.  ``direct_flow``: the flow dataset indexes the RAW tree (same videos, same frame
    numbering, the flow context's windows) -- its frames stand for the flow fields ``calc_optical_flow.chunk_flows`` computes, and
    nothing under ``optical_flow/`` is globbed."""
    cp, ds, method = c['cp'], c['dataset_name'], c['method']
    kw = dict(dataset_name=ds, mode=mode, border_mode=cp.get(method, 'border_mode'), all_bboxes=all_bboxes,
              patch_size=cp.getint(ds, 'patch_size'))
    raw = unified_dataset_interface(dir=os.path.join('raw_datasets', ds), file_format=frame_size[ds][2],
                                    context_frame_num=cp.getint(method, 'context_frame_num'), **kw)
    if direct_flow:
        flow = unified_dataset_interface(dir=os.path.join('raw_datasets', ds), file_format=frame_size[ds][2],
                                         context_frame_num=cp.getint(method, 'context_of_num'), **kw)
    else:
        flow = unified_dataset_interface(dir=os.path.join('optical_flow', ds), file_format='.npy',
                                         context_frame_num=cp.getint(method, 'context_of_num'), **kw)
    return raw, flow


def _stage(c, mode, direct_flow=False):
    """What every extractor starts from: the split's boxes and datasets, the ``<root>/<modality>/<ds>_`` prefix of its files (the
    directory is made), the block grid and its steps, ``motionThr``, ``<mode>_block_mode`` and the patch size."""
    cp, ds, hb, wb = c['cp'], c['dataset_name'], c['h_block'], c['w_block']
    boxes = load_bboxes(c, mode)
    raw_ds, flow_ds = _datasets(c, mode, boxes, direct_flow)
    os.makedirs(os.path.join(c['data_root_dir'], c['modality']), exist_ok=True)
    return SimpleNamespace(boxes=boxes, raw_ds=raw_ds, flow_ds=flow_ds, base=os.path.join(c['data_root_dir'], c['modality'], ds + '_'),
                           hb=hb, wb=wb, h_step=frame_size[ds][0] / hb, w_step=frame_size[ds][1] / wb, patch=cp.getint(ds, 'patch_size'),
                           motion_thr=cp.getfloat(ds, 'motionThr'), block_mode=cp.getint(ds, '{}_block_mode'.format(mode)))


def _blocks(st, bb):
    """The ``(hi, wi)`` grid cells box ``bb`` is filed under."""
    return calc_block_idx(bb[0], bb[2], bb[1], bb[3], st.h_step, st.w_step, mode=st.block_mode)


def _write_frame_index(st, ds, mode):
    """Writes and returns ``scene_idx`` (ShanghaiTech, else None) and the frame-level ``labels`` the evaluation step reads (test
    split with ground truth, else None; test.py:376-392 gets them through the dataset)."""
    scene_idx = labels = None
    if ds == 'ShanghaiTech':
        scene_idx = np.asarray(st.raw_ds.scene_idx)
        np.save(st.base + 'scene_idx.npy', st.raw_ds.scene_idx)
    if mode == 'test' and st.raw_ds.return_gt:
        labels = np.array([bool(np.asarray(st.raw_ds._gt(i)).max() > 0) for i in range(len(st.raw_ds))])
        np.save(st.base + 'frame_labels_test.npy', labels)
    return scene_idx, labels


PIXEL_GT_SHANGHAI = ('[mi355x] pixel_criterion = True does not cover ShanghaiTech (this build reads only its frame-level '
                     'test_frame_mask): set it to False')


def gt_source(c):
    """The per-pixel ground truth of the test split for ``[mi355x] pixel_criterion`` / ``region_criterion``: the dataset the reference's evaluation step
    builds (test.py:366-368: no context, 'hard' border) over ``<raw_dataset_dir>/<ds>``.  Returns ``gt`` with ``len(gt)`` = the
    number of test frames and ``gt(i)`` = the mask of frame ``i`` as a contiguous uint8 ``[h,w]`` array (non-zero = anomalous
    pixel).  Raises a one-line ``ValueError`` for ShanghaiTech (before anything is read), for a tree without per-pixel ground truth
    and for a mask that is not ``frame_size[ds][:2]``."""
    ds = c['dataset_name']
    if ds == 'ShanghaiTech':
        raise ValueError(PIXEL_GT_SHANGHAI)
    root = os.path.join(c['raw_dataset_dir'], ds)
    dataset = unified_dataset_interface(dataset_name=ds, dir=root, context_frame_num=0, mode='test', border_mode='hard')
    h, w = frame_size[ds][0], frame_size[ds][1]
    n_gt = len(dataset.all_gt_addr) if hasattr(dataset, 'all_gt_addr') else (dataset.all_gt.shape[1] if dataset.return_gt else 0)
    if not dataset.return_gt or n_gt != len(dataset):
        raise ValueError('[mi355x] pixel_criterion = True: {} holds per-pixel ground truth for {} of its {} test frames'.format(
            root, n_gt if dataset.return_gt else 0, len(dataset)))

    class Source:
        frame_video_idx = list(dataset.frame_video_idx)      # the video of every test frame ([mi355x] region_criterion: tracks)

        def __len__(self):
            return len(dataset)

        def __call__(self, i):
            g = np.asarray(dataset._gt(i))
            if g.shape != (h, w):
                raise ValueError('ground truth of test frame {} is {}, {} frames are {}x{}'.format(i, g.shape, ds, h, w))
            return np.ascontiguousarray(g != 0 if g.dtype != np.uint8 else g, dtype=np.uint8)

    return Source()


def test_video_idx(c):
    """The video of every test frame, in frame order (``[mi355x] smooth_masks``: a temporal window does not cross a video border): the
    ``frame_video_idx`` of the test split's frame indexer over ``<raw_dataset_dir>/<ds>`` -- what ``gt_source`` carries and
    ``calc_optical_flow.flow_pairs`` reads.  Any dataset; no frame and no ground truth is decoded."""
    ds = c['dataset_name']
    return list(unified_dataset_interface(dataset_name=ds, dir=os.path.join(c['raw_dataset_dir'], ds), context_frame_num=0, mode='test',
                                          border_mode='hard').frame_video_idx)


def render_sources(c, flow=False):
    """What ``[mi355x] render`` decodes: ``(frames, flows)``, the test split's frame indexer over ``raw_datasets/<ds>`` without a context
    (the raw dataset of ``_datasets`` at ``context_frame_num = 0``: ``get_inputs(frames.all_frame_addr[i])`` is frame ``i`` as the
    extractors decode it, BGR uint8 ``[h,w,3]``) and, with ``flow``, the same over ``optical_flow/<ds>`` (float32 ``[h,w,2]`` per frame: the
    field ``calc_optical_flow`` stores for it), else None.  No box, no ground truth; nothing is decoded here."""
    ds = c['dataset_name']
    kw = dict(dataset_name=ds, mode='test', border_mode='hard', context_frame_num=0)
    frames = unified_dataset_interface(dir=os.path.join('raw_datasets', ds), file_format=frame_size[ds][2], **kw)
    flows = unified_dataset_interface(dir=os.path.join('optical_flow', ds), file_format='.npy', **kw) if flow else None
    if flows is not None and len(flows) != len(frames):
        raise ValueError('[mi355x] render_flow = True: optical_flow/{} holds the flow of {} test frames, raw_datasets/{} {} frames'.format(
            ds, len(flows), ds, len(frames)))
    return frames, flows


def frame_cubes(raw_ds, flow_ds, idx, motion_thr, device='cuda'):
    """Cubes of frame ``idx`` that pass the motion test: (raw ``[m,(T,)P,P,3]`` uint8, flow ``[m,(Tf,)P,P,2]`` float32,
    kept box indices).  Flow energy per box = sum of squares over the patch (mean over the context frames when there is a
    context), train.py:159-170."""
    raw = raw_ds.cubes_device(idx, device)                  # [n,T,P,P,C]
    flow = flow_ds.cubes_device(idx, device)                # [n,Tf,P,P,2]
    mag = (flow.double() ** 2).sum(dim=(2, 3, 4)).mean(dim=1)          # one context frame: the mean is the sum itself
    keep = torch.nonzero(mag.cpu() > motion_thr).flatten().numpy()
    raw, flow = raw.cpu().numpy(), flow.cpu().numpy()
    if raw_ds.context_frame_num == 0:
        raw = raw[:, 0]
    if flow_ds.context_frame_num == 0:
        flow = flow[:, 0]
    return raw[keep], flow[keep], keep


def extract_train(c, device='cuda', log=print):
    """train.py:102-226 for modality raw2flow.  Writes ``<root>/raw2flow/<ds>_foreground_train_<fg>-{raw,flow}.npy``
    (ShanghaiTech: ``..._seg_<k>-{raw,flow}.npy`` every ``saveSegNum`` frames, frames visited in a random order)."""
    st = _stage(c, 'train')
    all_bboxes, raw_ds, flow_ds, hb, wb = st.boxes, st.raw_ds, st.flow_ds, st.hb, st.wb
    shanghai = c['dataset_name'] == 'ShanghaiTech'
    base = st.base + 'foreground_train_{}'.format(c['mode_fg'])

    def empty():
        def grid():
            return [[([], []) for _ in range(wb)] for _ in range(hb)]
        return [grid() for _ in range(raw_ds.scene_num)] if shanghai else grid()

    def dump(sets, suffix):
        pick = (lambda k: [[[np.array(cell[k]) for cell in row] for row in scene] for scene in sets]) if shanghai else \
            (lambda k: [[np.array(cell[k]) for cell in row] for row in sets])
        save_nested(base + suffix + '-raw.npy', pick(0), 3 if shanghai else 2)
        save_nested(base + suffix + '-flow.npy', pick(1), 3 if shanghai else 2)

    order = np.random.default_rng(c['shuffle_seed']).permutation(len(raw_ds)) if shanghai else np.arange(len(raw_ds))
    seg_num = c['cp'].getint(c['dataset_name'], 'saveSegNum') if shanghai else 0
    sets, count, seg = empty(), 0, 0
    for it, idx in enumerate(order):
        idx = int(idx)
        log('Extracting foreground in {}-th batch, {} in total'.format(it + 1, len(raw_ds)))
        boxes = all_bboxes[idx]
        if len(boxes) > 0:
            raw, flow, keep = frame_cubes(raw_ds, flow_ds, idx, st.motion_thr, device)
            grid = sets[raw_ds.scene_idx[idx] - 1] if shanghai else sets
            for k, b in enumerate(keep):
                for (hi, wi) in _blocks(st, boxes[b]):
                    grid[hi][wi][0].append(raw[k])
                    grid[hi][wi][1].append(flow[k])
        count += 1
        if shanghai and count == seg_num:
            dump(sets, '_seg_{}'.format(seg))
            sets, count, seg = empty(), 0, seg + 1
    if shanghai:
        if len(raw_ds) % seg_num != 0:
            dump(sets, '_seg_{}'.format(seg))
    else:
        dump(sets, '')
    log('foreground for training data saved!')


def extract_test(c, device='cuda', log=print):
    """test.py:98-176: per-frame, per-block cubes + their boxes ->
    ``<ds>_foreground_test_<fg>-{raw,flow}.npy``, ``<ds>_foreground_bbox_test_<fg>.npy`` (+ ``<ds>_scene_idx.npy``)."""
    st = _stage(c, 'test')
    _write_frame_index(st, c['dataset_name'], 'test')
    n = len(st.raw_ds)
    sets = [[[([], [], []) for _ in range(st.wb)] for _ in range(st.hb)] for _ in range(n)]
    for idx in range(n):
        log('Extracting foreground in {}-th batch, {} in total'.format(idx + 1, n))
        boxes = st.boxes[idx]
        if len(boxes) > 0:
            raw, flow, keep = frame_cubes(st.raw_ds, st.flow_ds, idx, st.motion_thr, device)
            for k, b in enumerate(keep):
                bb = boxes[b]
                for (hi, wi) in _blocks(st, bb):
                    cell = sets[idx][hi][wi]
                    cell[0].append(raw[k])
                    cell[1].append(flow[k])
                    cell[2].append(bb)
    for k, name in ((0, 'foreground_test_{}-raw.npy'), (1, 'foreground_test_{}-flow.npy'), (2, 'foreground_bbox_test_{}.npy')):
        save_nested(st.base + name.format(c['mode_fg']), [[[np.array(cell[k]) for cell in row] for row in fr] for fr in sets], 3)
    log('foreground for testing data saved!')


def block_groups(cube_frame, cube_blocks, n_frames, scene_idx=None):
    """Index lists of a cube store (pure, no GPU).  ``cube_frame[s]`` = frame of store cube ``s`` (cubes are stored in frame
    order), ``cube_blocks[s]`` = the ``(hi, wi)`` grid cells its box falls in (``calc_block_idx``).  Returns ``{(scene, hi, wi):
    (idx int64 [m], off int32 [n_frames + 1])}``: the cubes of that block, by frame and then in store order, with CSR offsets --
    the cubes of frame ``f`` are ``idx[off[f]:off[f+1]]``.  ``scene`` is ``scene_idx[f] - 1`` (ShanghaiTech: one model per scene)
    or None.  A box that lies in two blocks is one cube named by two lists."""
    lists = {}
    last = -1
    for s, (f, blocks) in enumerate(zip(cube_frame, cube_blocks)):
        if f < last:
            raise ValueError('store cubes must be in frame order (cube %d: frame %d after frame %d)' % (s, f, last))
        last = f
        key = None if scene_idx is None else int(scene_idx[f]) - 1
        for (hi, wi) in sorted(blocks):
            idx, cnt = lists.setdefault((key, hi, wi), ([], np.zeros(n_frames, np.int64)))
            idx.append(s)
            cnt[f] += 1
    return {k: (np.asarray(idx, np.int64), np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32))
            for k, (idx, cnt) in lists.items()}


def extract_device(c, mode='test', device='cuda', log=print, flownet2=None):
    """The extraction of ``extract_test`` without cube files: returns ``(info, parts)``.

    ``info``: ``n_frames``, ``scene_idx`` (ShanghaiTech, also written to ``<ds>_scene_idx.npy``; else None) and ``labels`` (also
    written to ``<ds>_frame_labels_test.npy`` when the test set has ground truth; else None) -- known before any frame is cut.
    ``parts``: a generator.  Frames are visited in order, ``[mi355x] direct_frames_per_chunk`` at a time: the union of the chunk's
    context windows (the datasets' own ``context_range``) is decoded and uploaded once, ``vv_cube_energy`` applies the motion test,
    its ``keep`` bytes come to the host (the one sync of a chunk), the kept boxes get store slots in frame and box order, and
    ``vv_cube_cut`` writes their raw and flow cubes into one device store in ``CubeStore`` layout.  Each yielded part is a dict:
    ``raw`` / ``flow`` (the store, of which the first ``n`` cubes are valid), ``groups`` (``block_groups`` over all ``n_frames``),
    ``boxes`` (float64 ``[n,4]``, per cube) and ``frames`` = the ``(first, end)`` frame range the part covers; the ranges of
    successive parts tile ``[0, n_frames)``.  The store holds ``min([mi355x] direct_max_cubes, number of boxes)`` cubes; when the
    next frame's cubes would not fit, the part collected so far is yielded and the store is reused, so the consumer must be done
    with a part before it asks for the next one.  A frame's cubes are never split between two parts.
    No ``foreground_test_*`` / ``foreground_bbox_test_*`` file is written.

    ``c['direct_flow']`` (``[mi355x] direct_flow``): no ``optical_flow/`` file is read either.  The flow windows come from a dataset
    over the raw tree; per chunk the frames of the raw windows and of the flow pairs (``calc_optical_flow.flow_pairs``) are decoded
    and uploaded once, and ``calc_optical_flow.chunk_flows`` computes the flow field of every frame some flow window names,
    ``[mi355x] direct_flow_pairs`` pairs per FlowNet2 launch, straight into the chunk's flow tensor.  A flow shared by two chunks is
    computed in both.  ``flownet2``: the network to use; None loads ``[mi355x] flownet2_checkpoint`` (``direct_flow_fp16``: in fp16 mode)."""
    from vec_vad_amd.extract import boxes_to_crops, chunk_windows, cube_cut, cube_energy
    direct_flow = bool(c.get('direct_flow', False))
    if direct_flow:
        from calc_optical_flow import chunk_flows, flow_pairs, load_flownet2
        if flownet2 is None:
            flownet2 = load_flownet2(c['flownet2_checkpoint'], device=device, fp16=c['direct_flow_fp16'])
        flow_pairs_per_launch = max(1, c['direct_flow_pairs'])
    st = _stage(c, mode, direct_flow)
    all_bboxes, raw_ds, flow_ds, hb, wb, motion_thr, P = st.boxes, st.raw_ds, st.flow_ds, st.hb, st.wb, st.motion_thr, st.patch
    n = len(raw_ds)
    scene_idx, labels = _write_frame_index(st, c['dataset_name'], mode)
    info = dict(n_frames=n, scene_idx=scene_idx, labels=labels)
    per_chunk, max_cubes = max(1, c['direct_frames_per_chunk']), max(1, c['direct_max_cubes'])

    def window(dataset, i):
        return [i] if dataset.context_frame_num == 0 else dataset.context_range(i)

    def upload(dataset, used):
        fr = np.stack([get_inputs(dataset.all_frame_addr[f]) for f in used])            # [F,H,W,C], each frame once
        return torch.from_numpy(np.ascontiguousarray(fr)).to(device)

    def parts():
        cap = max(1, min(max_cubes, int(sum(len(b) for b in all_bboxes))))
        store = None
        used_slots, first = 0, 0
        cube_frame, cube_blocks, cube_boxes = [], [], []

        def part(end):
            return dict(raw=store[0], flow=store[1], n=used_slots, frames=(first, end),
                        groups=block_groups(cube_frame, cube_blocks, n, info['scene_idx']),
                        boxes=np.asarray(cube_boxes, np.float64).reshape(-1, 4))

        for s in range(0, n, per_chunk):
            e = min(s + per_chunk, n)
            idxs = [i for i in range(s, e) if len(all_bboxes[i]) > 0]
            log('Extracting foreground of frames {}-{}, {} in total'.format(s + 1, e, n))
            if not idxs:
                continue
            used_r, win_r = chunk_windows([window(raw_ds, i) for i in idxs])
            used_f, win_f = chunk_windows([window(flow_ds, i) for i in idxs])
            if direct_flow:
                pairs = flow_pairs(flow_ds, used_f)
                used = sorted(set(used_r) | {f for p in pairs for f in p})
                local = {f: k for k, f in enumerate(used)}
                fr_raw = upload(raw_ds, used)                  # the raw windows' frames and the pairs' frames, each once
                win_r = np.array([local[f] for f in used_r], np.int32)[win_r]
                fr_flow = torch.empty((len(used_f),) + tuple(fr_raw.shape[1:3]) + (2,), dtype=torch.float32, device=device)
                chunk_flows(flownet2, fr_raw, [(local[a], local[b]) for a, b in pairs], np.arange(len(used_f)), fr_flow,
                            flow_pairs_per_launch)
            else:
                fr_raw, fr_flow = upload(raw_ds, used_r), upload(flow_ds, used_f)
            H, W = fr_raw.shape[1], fr_raw.shape[2]
            counts = [len(all_bboxes[i]) for i in idxs]
            crops = np.concatenate([boxes_to_crops(all_bboxes[i], H, W) for i in idxs])
            rows = np.repeat(np.arange(len(idxs)), counts)                    # chunk-local frame of every box
            wr, wf = win_r[rows], win_f[rows]                  # host tables: cube_energy / cube_cut check them without a sync
            _, keep = cube_energy(fr_flow, crops, wf, P, motion_thr)
            keep = keep.cpu().numpy().astype(bool)
            if store is None:
                store = (torch.empty((cap, win_r.shape[1], P, P, fr_raw.shape[3]), dtype=fr_raw.dtype, device=device),
                         torch.empty((cap, win_f.shape[1], P, P, fr_flow.shape[3]), dtype=torch.float32, device=device))
            slot = np.full(len(crops), -1, np.int32)

            def cut():
                if (slot >= 0).any():
                    cube_cut(fr_raw, crops, wr, slot, P, store[0])
                    cube_cut(fr_flow, crops, wf, slot, P, store[1])

            p = 0
            for k, i in enumerate(idxs):
                kept = np.nonzero(keep[p:p + counts[k]])[0]
                if len(kept) > cap:
                    raise ValueError('frame {} has {} cubes, [mi355x] direct_max_cubes holds {}'.format(i, len(kept), cap))
                if used_slots + len(kept) > cap:           # the store is full: hand over what it holds, then reuse it
                    cut()
                    yield part(i)
                    slot[:] = -1
                    used_slots, first = 0, i
                    cube_frame, cube_blocks, cube_boxes = [], [], []
                for b in kept:
                    bb = all_bboxes[i][b]
                    blocks = _blocks(st, bb)
                    if any(not (0 <= hi < hb and 0 <= wi < wb) for hi, wi in blocks):
                        raise IndexError('box {} of frame {} falls outside the {}x{} block grid'.format(b, i, hb, wb))
                    slot[p + b] = used_slots
                    used_slots += 1
                    cube_frame.append(i)
                    cube_blocks.append(blocks)
                    cube_boxes.append(np.asarray(bb, np.float64)[:4])
                p += counts[k]
            cut()
        if store is None:
            store = (torch.empty((0, 1, P, P, 3), dtype=torch.uint8, device=device),
                     torch.empty((0, 1, P, P, 2), dtype=torch.float32, device=device))
        yield part(n)

    return info, parts()


def extract_train_device(c, device='cuda', log=print, flownet2=None):
    """The extraction of ``extract_train`` without cube files (``[mi355x] direct_train``; UCSDped2 / avenue): ``extract_device`` with
    ``mode='train'`` (``train_block_mode``, the boxes of ``load_bboxes(c, 'train')``, no labels), the kept cubes of the WHOLE split
    in one device store -- the trainer visits every cube every epoch.  Returns a dict: ``raw`` / ``flow`` (the store, of which the
    first ``n`` cubes are valid, in frame and then box order), ``groups`` = ``{(None, hi, wi): (idx, off)}`` (``block_groups``;
    ``store[idx]`` are the arrays ``extract_train`` files under block ``(hi, wi)``, in their order; a box in two blocks is one cube
    named by two lists) and ``n_frames``.  No ``foreground_train_*`` file is written; with ``c['direct_flow']`` nothing under
    ``optical_flow/`` is read (``flownet2`` as for ``extract_device``).

    A split whose kept cubes do not fit ``[mi355x] direct_max_cubes`` raises ValueError (the rest of the split is still visited,
    without keeping its cubes, so that the message can tell the number needed): no partial set is returned.  ShanghaiTech (one
    model per scene, randomly ordered ``saveSegNum`` segments) raises NotImplementedError before any GPU work."""
    if c['dataset_name'] == 'ShanghaiTech':
        from train import DIRECT_TRAIN_SHANGHAI
        raise NotImplementedError(DIRECT_TRAIN_SHANGHAI)
    info, parts = extract_device(c, 'train', device, log, flownet2=flownet2)
    first = next(parts)
    out = dict(raw=first['raw'], flow=first['flow'], n=first['n'], groups=first['groups'], n_frames=info['n_frames'])
    later = [p['n'] for p in parts]          # the store is reused from here on: ``out`` is not handed to anybody
    if later:
        raise ValueError('[mi355x] direct_max_cubes = {}: the training split keeps {} cubes, and direct_train needs all of them in '
                         'one store (raise direct_max_cubes, or train from cube files with direct_train = False)'.format(
                             c['direct_max_cubes'], out['n'] + sum(later)))
    log('foreground for training data cut: {} cubes of {} frames in the device store'.format(out['n'], out['n_frames']))
    return out
