#!/usr/bin/env python
"""``python test.py`` -- abnormal-event detection stage of VEC_VAD on the MI355X UNet-bank engine.

Drop-in for the reference's test.py:193-399: loads ``<ds>_model_<mode>_SelfComplete.npy`` and the training-score files
written by train.py (or by the reference: same torch-pickle layout and ``module.``-prefixed keys), scores every test
cube in eval mode, z-normalises with the training-score mean / population std (test.py:260-266,338-345), paints the
scores into the bbox rectangles and max-combines them into the per-frame map ``results/<ds>/score_mask/<frame>``
(test.py:350-358), then evaluates frame-level ROC-AUC (test.py:362-399, utils.py:29-65).

Differences on purpose: the reference runs one tiny batch per frame (1-30 cubes); eval-mode BatchNorm makes scores
batch independent, so many frames are scored per launch (``[mi355x] score_batch``).  Ground-truth frame labels come from
``<data_root>/<modality>/<ds>_frame_labels_test.npy`` (bool per frame; write it once from
``unified_dataset_interface(..., mode='test')`` targets, test.py:366-392); without that file the evaluation step is
skipped.  Cube errors never leave HBM between the UNet bank and the frame score (``vv_frame_scores``); the h x w masks are
only painted when ``[mi355x] save_score_masks`` asks for the reference's ``score_mask/<frame>`` files.

``[mi355x] direct_test = True`` (default False) scores straight from frames and boxes: ``foreground.extract_device`` cuts the
cubes of many frames per launch into a device-resident store and ``score_store`` scores them through per-block index lists, so no
``foreground_test_*`` / ``foreground_bbox_test_*`` file is written or read and every frame is decoded once per chunk.  The frame
scores, score masks and the evaluation are those of the staged path.

``[mi355x] direct_flow = True`` (default False; needs ``direct_test``) also computes the optical flow of every chunk on the GPU
(``calc_optical_flow.chunk_flows``: FlowNet2 from a captured graph between two HIP resize kernels), so the test stage reads nothing
under ``optical_flow/``.  ``main(config_path, flownet2=None)`` takes the network to use; None loads ``[mi355x] flownet2_checkpoint``.

``[mi355x] pixel_criterion = True`` (default False; UCSDped2 / avenue) adds the pixel-level criterion the masks are stored for and
the reference never evaluates (test.py:362-365 ``criterion = 'frame'``): per frame one number (``scoring.pixel_scores``), computed
on the GPU from the device-resident cube scores and the per-pixel ground truth, ``results/<ds>/pixel_scores_<fg>_<method>.npy``
and ``<modality>_<fg>_<method>_pixel_results.npz``.  ``[mi355x] device_score_masks = True`` paints the ``score_mask`` files on the
GPU (``scoring.paint_masks``) instead of the numpy loop over boxes; the same files.

``[mi355x] pixel_maps = True`` (default False) keeps the per-pixel reconstruction error of every scored cube on the device, paints it
back into the frame through the cube's rectangle (``scoring.error_zmaps`` + ``scoring.paint_error_masks``: fine masks that say where
inside a box the anomaly lies, with the support of the ``score_mask`` files) and saves them as ``results/<ds>/error_mask/<frame>``
when ``save_score_masks`` is on; with ``pixel_criterion`` the same criterion is also evaluated on the fine masks
(``scoring.mask_pixel_scores``): ``pixel_scores_fine_<fg>_<method>.npy`` and ``<modality>_<fg>_<method>_pixel_fine_results.npz``.
Everything else -- frame scores, ``score_mask`` files, pixel scores -- is what a run without the key writes.

``[mi355x] region_criterion = True`` (default False; UCSDped2 / avenue; independent of ``pixel_criterion``) adds the region- and
track-based detection criteria (RBDC / TBDC, ``scoring`` module docstring) with the scored boxes as detections: per chunk the ground truth
is labelled into regions, matched against the chunk's boxes and linked to the frame before on the GPU (``scoring.label_regions``,
``region_match``, ``region_links``); ``results/<ds>/region_scores_<fg>_<method>.npz`` keeps the region, track and false-positive scores
and ``<modality>_<fg>_<method>_region_results.npz`` the curves and the two numbers.  Regions and tracks are derived from the per-pixel
ground truth, not read from hand-drawn annotations as for published numbers.  Every other file is what a run without the key writes.

``[mi355x] smooth_masks = True`` (default False) adds the step the object-centric VAD protocol takes before it thresholds anything: the
``score_mask`` volume is filtered on the GPU by a 3-D mean over the painted pixels (``scoring.smooth_masks``; ``smooth_frames`` frames of
the same video x ``smooth_pixels`` x ``smooth_pixels`` pixels) and the frame score is the maximum of the filtered mask.  The scored
groups of the whole test set stay on the device (24 B per cube) and one ``_smooth_stage`` runs after all scoring, chunk by chunk with a
temporal halo, so neither ``direct_frames_per_chunk`` nor ``direct_max_cubes`` changes the result.  Writes
``frame_scores_smooth_<fg>_<method>.npy`` and ``<modality>_<fg>_<method>_frame_smooth_results.npz`` (per scene for ShanghaiTech); with
``pixel_criterion`` ``pixel_scores_smooth_*.npy`` and ``*_pixel_smooth_results.npz``; with ``save_score_masks``
``results/<ds>/score_mask_smooth/<frame>``.  A box of a block without a trained model (``+BIG``) floods its neighbourhood.  Every other
file is what a run without the key writes; the two windows are untuned.

``[mi355x] auc_statistics = True`` (default False; any dataset, ShanghaiTech included; also with ``scores_saved = True``) adds, for every
score vector the run has (``frame``, ``frame_smooth``, ``pixel``, ``pixel_fine``, ``pixel_smooth``) and when the frame labels are there,
the micro AUROC (per-scene mean for ShanghaiTech) and the macro AUROC (mean of the per-video AUROCs) with bootstrap percentile intervals
(``scoring.auc_bootstrap``: ``auc_bootstrap`` replicates of a moving-block or video bootstrap whose weighted pair counts come from the
GPU in integers), and the paired difference of every non-plain vector against its plain counterpart (``scoring.auc_paired``).  Writes
``<modality>_<fg>_<method>_<name>_bootstrap.npz`` and prints one line per statistic.  Every other file is what a run without the key
writes.  The default block length is an untuned pick: no accuracy claim follows from an interval made with it.

``[mi355x] render = True`` (default False) writes pictures a person can look at: after all scoring (and after the smooth stage) one
``_render_stage`` runs over the kept groups and writes ``results/<ds>/render/<frame>.png`` for every ``render_every``-th test frame -- the
frame with the score mask (``render_source``: ``score`` or ``smooth``) blended over it through a colour table that spans ``render_range``,
the outlines of the scored boxes, the contour of the per-pixel ground truth where the tree has one (UCSDped2 / avenue) and, with
``render_flow``, the Middlebury colour image of the frame's flow field to the right (``vec_vad_amd/render.py``; both composed on the GPU).
Staged route, direct route and direct route in parts write the same pictures.  With ``scores_saved = True`` nothing is scored, so nothing
is rendered.  Every other file is what a run without the key writes.
"""
import collections
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from train import read_config, build_network  # noqa: E402
from utils import save_roc_pr_curve_data  # noqa: E402
from vad_datasets import frame_size  # noqa: E402
from vec_vad_amd.trainer import FusedTrainer  # noqa: E402
from vec_vad_amd import scoring  # noqa: E402

BIG = 100000


def load_model(net, state_dict, device):
    """test.py:255-257: the saved keys carry DataParallel's 'module.' prefix."""
    sd = {(k[len('module.'):] if k.startswith('module.') else k): v for k, v in state_dict.items()}
    net.load_state_dict(sd)
    net.to(device)
    net.eval()
    return net


def load_artifacts(base, fg, method, shanghai, build_net, device, h_block=1, w_block=1):
    """test.py:230-266: the three files train.py wrote (torch pickles despite the .npy suffix, train.py:432-436) -> (net_set,
    raw statistics, flow statistics) with the reference's nesting -- [h][w] for UCSDped2 / avenue, [scene][h][w] for ShanghaiTech;
    a block without a trained model is an empty list (train.py:370 skips blocks with <= 1 cube).  The nesting of all three results
    follows the model FILE: ``h_block`` / ``w_block`` are accepted for compatibility and ignored.  Works on files written by the
    reference itself (tests/test_ref_written_files.py): 'module.'-prefixed keys, aliased storages, int64 num_batches_tracked."""
    weights = torch.load(base + 'model_{}_{}.npy'.format(fg, method), map_location='cpu', weights_only=False)
    raw_tr = torch.load(base + 'raw_training_scores_{}_{}.npy'.format(fg, method), weights_only=False)
    of_tr = torch.load(base + 'of_training_scores_{}_{}.npy'.format(fg, method), weights_only=False)
    return artifacts_from(weights, raw_tr, of_tr, shanghai, build_net, device)


def artifacts_from(weights, raw_tr, of_tr, shanghai, build_net, device):
    """What follows the file loads of ``load_artifacts``: the three nested lists the training stage saves (``train.train_store`` returns
    them) -> (net_set, raw statistics, flow statistics)."""
    def build(wl):
        return [load_model(build_net(), wl[0], device)] if len(wl) > 0 else []

    def stat(a):
        a = np.asarray(a)
        return (np.mean(a), np.std(a)) if a.size else (0.0, 1.0)      # population std, test.py:264-266

    def over(fn, src, like, depth):
        return fn(src) if depth == 0 else [over(fn, src[i], like[i], depth - 1) for i in range(len(like))]

    depth = 3 if shanghai else 2
    return over(build, weights, weights, depth), over(stat, raw_tr, weights, depth), over(stat, of_tr, weights, depth)


def _blank(device, *shape):
    """Scores ``[n_frames]`` before any cube has been seen, or masks ``[k,h,w]`` without a painted pixel: float64 of ``-BIG``."""
    return torch.full((*shape,), -float(BIG), dtype=torch.float64, device=device)


class _Gathered:
    """The results of the launches that score a list of ``n`` cubes: raw scores, flow scores and, with ``maps``, the two per-pixel
    error maps behind them, on the device.  A flow tensor is allocated when the first launch returns one, so it stays None for a bank
    without a flow branch."""

    def __init__(self, n, maps, device):
        self.n, self.maps, self.device = n, maps, device
        self.parts = [torch.empty(n, device=device), None, torch.empty((n, 32, 32), device=device) if maps else None, None]

    def put(self, s0, m, *launch):
        """The first ``m`` results of a launch -- (raw, of | None), with ``maps`` followed by (e_raw, e_of | None) -- are those of
        cubes ``[s0, s0 + m)``."""
        for k, x in enumerate(launch):
            if x is not None:
                if self.parts[k] is None:
                    self.parts[k] = torch.empty((self.n,) + x.shape[1:], device=self.device)
                self.parts[k][s0:s0 + m] = x[:m]

    def result(self):
        """(raw [n], of [n] | None), with ``maps`` followed by (e_raw [n,32,32], e_of [n,32,32] | None)."""
        return tuple(self.parts if self.maps else self.parts[:2])


def score_cubes_device(trainer, cube_list, flow_list, score_batch, chunk_cubes=None, maps=False):
    """cube_list / flow_list: per-frame arrays [n_i,5,32,32,3] uint8 / [n_i,(Tf,)32,32,2] fp32 (n_i may be 0).
    The cubes go to the GPU in bounded super-chunks (``chunk_cubes``, default 32 launches' worth, >= 4096: ~55 KB per cube for the
    5raw+5of bank, so host and device staging stay at a few hundred MB whatever the size of the test set) through ONE fixed device
    staging buffer, and every chunk is scored by ``score_index_list`` in launches of exactly ``score_batch`` cubes (the tail launch
    re-scores the chunk's last cube as padding: eval-mode scores do not depend on the batch) -- one workspace, one launch plan and
    one captured hipGraph serve the whole test set.  Returns the DEVICE tensors (raw [n], of [n] | None) of all cubes in frame order -- they feed
    vv_frame_scores without visiting the host.  ``maps``: also the per-pixel error maps (e_raw [n,32,32], e_of [n,32,32] | None) behind them."""
    dev = trainer.bank.device
    keep = [k for k in range(len(cube_list)) if len(cube_list[k])]
    if not keep:
        return (torch.zeros(0, device=dev), None) + ((torch.zeros((0, 32, 32), device=dev), None) if maps else ())
    counts = [len(cube_list[k]) for k in keep]
    n = int(sum(counts))
    B = int(min(score_batch, n)) if n < score_batch else int(score_batch)
    cap = int(chunk_cubes) if chunk_cubes else max(4096, 32 * B)
    cap = max(B, min(cap, n))

    def prep(k):
        raw = np.asarray(cube_list[k])
        flow = np.asarray(flow_list[k], dtype=np.float32)
        if raw.dtype != np.uint8:
            raise TypeError('foreground cubes must be uint8 (the -raw.npy files of train.py:218-222), got %s' % raw.dtype)
        return (raw[:, None] if raw.ndim == 4 else raw), (flow[:, None] if flow.ndim == 4 else flow)

    r0, f0 = prep(keep[0])
    rawd = torch.empty((cap,) + r0.shape[1:], dtype=torch.uint8, device=dev)
    flowd = torch.empty((cap,) + f0.shape[1:], dtype=torch.float32, device=dev)
    gathered = _Gathered(n, maps, dev)
    done = 0
    pend_r, pend_f, pend_n = [], [], 0

    def flush():
        nonlocal done, pend_r, pend_f, pend_n
        m_tot = pend_n
        if not m_tot:
            return
        rawd[:m_tot].copy_(torch.from_numpy(np.ascontiguousarray(np.concatenate(pend_r))))
        flowd[:m_tot].copy_(torch.from_numpy(np.ascontiguousarray(np.concatenate(pend_f))))
        # launches of B cubes whatever the chunk holds: B comes from the whole list, and the bank picks its kernels by it
        gathered.put(done, m_tot, *score_index_list(trainer, rawd, flowd, torch.arange(m_tot, device=dev), score_batch, batch=B,
                                                    maps=maps))
        done += m_tot
        pend_r, pend_f, pend_n = [], [], 0

    for k in keep:
        raw, flow = prep(k)
        p = 0
        while p < len(raw):              # a single frame may hold more cubes than a chunk
            take = min(len(raw) - p, cap - pend_n)
            pend_r.append(raw[p:p + take])
            pend_f.append(flow[p:p + take])
            pend_n += take
            p += take
            if pend_n == cap:
                flush()
    flush()
    return gathered.result()


def score_cubes_batched(trainer, cube_list, flow_list, score_batch):
    """Host view of ``score_cubes_device``: per-frame (raw_scores [n_i], of_scores [n_i] | None) numpy arrays."""
    r, o = score_cubes_device(trainer, cube_list, flow_list, score_batch)
    r = r.cpu().numpy()
    o = o.cpu().numpy() if o is not None else None
    out, p = [], 0
    for c in cube_list:
        n = len(c)
        out.append((r[p:p + n], o[p:p + n] if o is not None else None))
        p += n
    return out


def paint_frame(scores, bboxes, h, w):
    """test.py:350-357: each cube's score fills its (ceil'ed) bbox; maps are max-combined; untouched pixels = -1e5."""
    res = -1.0 * np.ones((h, w)) * BIG
    for m in range(len(scores)):
        bb = bboxes[m]
        x_min, x_max = int(np.ceil(bb[0])), int(np.ceil(bb[2]))
        y_min, y_max = int(np.ceil(bb[1])), int(np.ceil(bb[3]))
        region = res[y_min:y_max, x_min:x_max]
        np.maximum(region, scores[m], out=region)
    return res


def _mask_scores(r, o, stats, w_raw, w_of, trained):
    """Host copy of the per-cube scores that ``paint_frame`` paints (test.py:338-348): z-normalised and weighted, ``BIG`` for a
    block without a trained model."""
    if not trained:
        return np.ones(r.numel()) * BIG
    sc = w_raw * ((r.cpu().numpy().astype(np.float32) - stats[0, 0]) / stats[0, 1])
    if o is not None:
        sc = sc + w_of * ((o.cpu().numpy().astype(np.float32) - stats[0, 2]) / stats[0, 3])
    return sc


def _save_frames(out_dir, first_frame, masks):
    """THE mask writer: ``<out_dir>/<first_frame + k>`` for every mask of ``masks`` (float64 ``[k,h,w]``, device tensor, host tensor or
    array; a device tensor comes to the host in one copy).  Every file is the torch pickle of an array of its own, C-contiguous, as
    the reference saves its masks (test.py:358).  ``out_dir`` exists: the stage that writes there makes it once."""
    masks = masks.cpu().numpy() if torch.is_tensor(masks) else masks
    for k in range(len(masks)):
        torch.save(masks[k].copy(), os.path.join(out_dir, '{}'.format(first_frame + k)))


def _save_masks(result_dir, frames, mask_groups, h, w):
    """``<result_dir>/<frame>`` for every frame of ``frames``, painted on the host: one h x w float64 mask alive at a time, like the
    reference (test.py:350-358).  mask_groups: (off indexed by frame, host cube scores, boxes) per scored group."""
    os.makedirs(result_dir, exist_ok=True)
    for f in frames:
        fmap = -1.0 * np.ones((h, w)) * BIG
        for off, sc, boxes in mask_groups:
            if off[f + 1] > off[f]:
                sl = slice(off[f], off[f + 1])
                np.maximum(fmap, paint_frame(sc[sl], boxes[sl], h, w), out=fmap)
        _save_frames(result_dir, f, fmap[None])


def _frame_chunks(first, end, per_chunk, halo=0):
    """Frames ``[first, end)`` in chunks of ``per_chunk``: ``(a, b, pa, pb)`` per chunk ``[a, b)``, with ``[pa, pb)`` the chunk widened by
    ``halo`` frames on either side and clamped to the frames that exist, ``[0, end)`` -- what a temporal window around the chunk's
    frames reads."""
    for a in range(first, end, per_chunk):
        b = min(a + per_chunk, end)
        yield a, b, max(0, a - halo), min(end, b + halo)


def _gt_chunk(gt, frames, device):
    """The per-pixel ground truth of ``frames`` (``gt``: a ground-truth source) on the device, uint8 ``[len(frames),h,w]``, in one upload."""
    return torch.from_numpy(np.stack([gt(i) for i in frames])).to(device)


def _video_idx(c, gt):
    """The video of every test frame: the open ground-truth source knows it, otherwise the test split is indexed for it."""
    if gt is not None:
        return gt.frame_video_idx
    from foreground import test_video_idx
    return test_video_idx(c)


class PixelEval:
    """What ``score_frames`` / ``score_store`` need for the pixel-level stage (their ``pixel`` keyword).  ``gt``: the ground-truth
    source (``foreground.gt_source``: ``gt(i)`` -> uint8 ``[h,w]``) or None for no pixel criterion; ``percent``: the overlap in
    integer percent; ``out``: CUDA float64 ``[n_frames]`` that receives the pixel scores of the frames a call covers; ``labels``:
    the frame labels (bool ``[n_frames]``) the ground-truth pixel counts are checked against, or None; ``device_masks``: paint the
    ``result_dir`` masks on the GPU; ``frames_per_chunk``: frames per ground-truth upload / mask download.  ``maps`` (``[mi355x]
    pixel_maps``): the per-pixel error maps of every scored cube are kept and painted into fine masks, saved per frame under
    ``error_dir`` when one is given and, with a ground-truth source, reduced to ``out_fine`` (CUDA float64 ``[n_frames]``) like ``out``.

    ``regions`` (``[mi355x] region_criterion``; needs a ground-truth source): the region stage runs on every chunk next to the pixel
    scores, with ``region_iou`` the match bound in integer percent and ``video_idx`` the video of every test frame
    (``frame_video_idx``).  The object then carries the accumulating region state across chunks and across the parts of
    ``score_store`` -- the last label map of the frame before (for the links), and per chunk the region counts, areas, scores, link
    words and false-positive scores --, which ``region_state`` turns into the lists the curves are made of.  Frames must arrive in
    increasing order, each once.  ``criterion = False`` keeps a ground-truth source without the pixel scores (``out`` not needed).

    ``keep_groups`` (``[mi355x] smooth_masks`` or ``render``): every call appends its scored groups -- (off over all test frames, device
    cube scores, device rectangles), 24 B per cube -- to ``groups``, across the parts of ``score_store``.  Both ``_smooth_stage`` and
    ``_render_stage`` read them, once, after all scoring; without the keyword ``groups`` is None."""

    def __init__(self, gt=None, percent=40, out=None, labels=None, device_masks=False, frames_per_chunk=64, maps=False, error_dir=None,
                 out_fine=None, criterion=True, regions=False, region_iou=10, video_idx=None, keep_groups=False):
        self.gt, self.percent, self.out, self.labels = gt, int(percent), out, labels
        self.device_masks, self.frames_per_chunk = bool(device_masks), max(1, int(frames_per_chunk))
        self.maps, self.error_dir, self.out_fine = bool(maps), error_dir, out_fine
        self.criterion, self.regions, self.region_iou = bool(criterion), bool(regions), int(region_iou)
        self.video_idx = None if video_idx is None else np.asarray(video_idx)
        if gt is not None and self.criterion and out is None:
            raise ValueError('PixelEval: a ground-truth source needs an `out` vector for the pixel scores')
        if self.maps and gt is not None and self.criterion and out_fine is None:
            raise ValueError('PixelEval: maps with a ground-truth source need an `out_fine` vector for the fine pixel scores')
        if self.regions and (gt is None or self.video_idx is None):
            raise ValueError('PixelEval: regions need a ground-truth source and the video index of every frame')
        self.prev_labels, self.next_frame = None, 0        # label map of frame next_frame - 1 (device), the frame expected next
        self.region_chunks = []                            # per chunk: (first frame, n_regions, area, score, links, fp scores), host
        self.groups = [] if keep_groups else None          # every scored group of the test set, for _smooth_stage and _render_stage

    def region_stage(self, gt, off, scores, rects, a, b):
        """The region stage of frames ``[a, b)``: ``gt`` the chunk's uploaded ground truth, (off, scores, rects) its merged cubes."""
        if a != self.next_frame:
            raise ValueError('PixelEval: the region stage expects frame {} next, got {}'.format(self.next_frame, a))
        labels, n_regions = scoring.label_regions(gt, frame0=a)
        area, best, state = scoring.region_match(labels, scores, off, rects, self.region_iou)
        vid = self.video_idx
        same = np.array([f > 0 and vid[f] == vid[f - 1] for f in range(a, b)], np.uint8)
        links = scoring.region_links(labels, self.prev_labels, same)
        self.region_chunks.append((a, n_regions.cpu().numpy(), area.cpu().numpy(), best.cpu().numpy(), links.cpu().numpy(),
                                   scores[state == 2].cpu().numpy()))
        if b > a:
            self.prev_labels, self.next_frame = labels[-1].clone(), b

    def region_state(self, track_percent=10):
        """What the chunks add up to: region score / frame / area / track (one entry per region, in frame and number order), track
        scores, false-positive scores (descending) and the number of frames seen."""
        n_reg = np.concatenate([c[1] for c in self.region_chunks] or [np.zeros(0, np.int32)]).astype(np.int64)
        links = np.concatenate([c[4] for c in self.region_chunks] or [np.zeros((0, scoring.REGION_MAX), np.int64)])
        pick = np.arange(scoring.REGION_MAX)[None, :] < n_reg[:, None]                      # [F,64]: the regions that exist
        score = np.concatenate([c[3] for c in self.region_chunks] or [np.zeros((0, scoring.REGION_MAX))])[pick]
        area = np.concatenate([c[2] for c in self.region_chunks] or [np.zeros((0, scoring.REGION_MAX), np.int32)])[pick]
        frame = np.repeat(np.arange(n_reg.size), n_reg)
        track, _, k = scoring.link_tracks(n_reg, links, track_percent)
        fp = np.sort(np.concatenate([c[5] for c in self.region_chunks] or [np.zeros(0)]))[::-1]
        return dict(region_score=score.astype(np.float64), region_frame=frame.astype(np.int64), region_area=area.astype(np.int32),
                    region_track=track, track_score=scoring.track_scores(score, track, k), fp_score=np.ascontiguousarray(fp),
                    n_frames=np.int64(self.next_frame))


def _pixel_stage(pixel, dev_groups, first, end, h, w, result_dir, device, map_groups=None):
    """Frames ``[first, end)`` of the scored groups ``dev_groups`` ((off, device cube scores, device rectangles) each) in chunks:
    the chunk's cubes are merged into frame order and reduced to pixel scores against the chunk's ground truth (uploaded once),
    and / or its masks are painted on the device, group by group, brought to the host once and saved per frame.  ``map_groups``
    (``pixel.maps``; one entry per group of ``dev_groups``: None for a block without a model, else (e_raw, e_of, stats, w_raw, w_of)):
    the chunk's z-maps are formed and painted group by group into one fine-mask buffer, which is saved per frame under
    ``pixel.error_dir`` and / or reduced to ``pixel.out_fine`` against the same ground truth.  With ``pixel.regions`` the region stage
    (``PixelEval.region_stage``) runs on the same merged cubes and the same uploaded ground truth."""
    paint = pixel.device_masks and result_dir
    if paint:
        os.makedirs(result_dir, exist_ok=True)
    if map_groups is not None and pixel.error_dir:
        os.makedirs(pixel.error_dir, exist_ok=True)
    for a, b, _, _ in _frame_chunks(first, end, pixel.frames_per_chunk):
        sub = [(off[a:b + 1], sc, rc) for off, sc, rc in dev_groups]
        gt = None
        if pixel.gt is not None:
            off, sc, rc = scoring.merge_groups(sub, n_frames=b - a, device=device)
            gt = _gt_chunk(pixel.gt, range(a, b), device)
            if pixel.regions:
                pixel.region_stage(gt, off, sc, rc, a, b)
            cnt = None
            if pixel.criterion:
                _, cnt = scoring.pixel_scores(gt, sc, off, rc, pixel.percent, out=pixel.out[a:b])
            if cnt is not None and pixel.labels is not None:
                bad = np.nonzero((cnt.cpu().numpy() > 0) != np.asarray(pixel.labels[a:b], bool))[0]
                if len(bad):
                    raise ValueError('frame {}: its label and its per-pixel ground truth disagree on whether it is anomalous'.format(
                        a + int(bad[0])))
        if paint:
            _save_frames(result_dir, a, _paint_frames(dev_groups, a, b, h, w, device))
        if map_groups is not None:
            fine = _blank(device, b - a, h, w)
            for (off, _, rc), kept in zip(sub, map_groups):
                lo, hi = int(off[0]), int(off[-1])
                if hi <= lo:
                    continue
                if kept is None:     # a block without a model: BIG all over the box, as in the painted mask
                    z = torch.full((hi - lo, 32, 32), float(BIG), dtype=torch.float64, device=device)
                else:
                    e_raw, e_of, stats, w_raw, w_of = kept
                    z = scoring.error_zmaps(e_raw[lo:hi], e_of[lo:hi] if e_of is not None else None, np.zeros(hi - lo, np.int32), stats,
                                            w_raw, w_of)
                scoring.paint_error_masks(z, off - lo, rc[lo:hi], h, w, out=fine)
                del z
            if gt is not None and pixel.criterion:
                scoring.mask_pixel_scores(gt, fine, pixel.percent, out=pixel.out_fine[a:b])
            if pixel.error_dir:
                _save_frames(pixel.error_dir, a, fine)


def _group_scorer(net_set, stats_raw, stats_of, h, w, w_raw, w_of, useFlow, device, trainers, fs_dev, mask_groups, dev_groups=None,
                  map_groups=None):
    """The per-group body of ``score_frames`` and ``score_store``.  The returned ``group(key, hh, ww, n, off, boxes, score)`` scores
    the ``n`` cubes of block ``(hh, ww)`` (of scene ``key``, or None) with ``score(trainer)`` -> device (raw [n], of [n] | None),
    max-accumulates their frame scores into ``fs_dev`` (``off``: CSR over the frames, ``boxes`` float64 ``[n,4]``) and, when
    ``mask_groups`` is a list, appends the group's (off, host cube scores, boxes) for ``_save_masks``; when ``dev_groups`` is a list,
    the group's (off, device cube scores, device rectangles) for ``_pixel_stage``; when ``map_groups`` is a list, ``score(trainer)`` also
    returns the per-pixel error maps (e_raw, e_of | None) and the group's entry for ``_pixel_stage`` is appended next to them."""
    def group(key, hh, ww, n, off, boxes, score):
        def pick(nested):
            return nested[key][hh][ww] if key is not None else nested[hh][ww]
        models = pick(net_set)
        if len(models) > 0:
            net = models[0]
            if id(net) not in trainers:
                trainers[id(net)] = FusedTrainer(net)
            st_r = pick(stats_raw)
            st_o = pick(stats_of) if useFlow else (0.0, 1.0)
            r, o, *e = score(trainers[id(net)])
            o = o if useFlow else None
            stats = np.array([[st_r[0], st_r[1], st_o[0], st_o[1]]], np.float64)
            cube_stat = np.zeros(n, np.int32)
        else:        # anomaly: no object in the training set in this block (test.py:346-348)
            r, o, e = torch.zeros(n, device=device), None, None
            stats = np.array([[0.0, 1.0, 0.0, 1.0]])
            cube_stat = np.full(n, -1, np.int32)
        scoring.frame_scores(r, o, off, cube_stat, stats, scoring.box_paints(boxes, h, w), w_raw, w_of, out=fs_dev)
        if mask_groups is not None:
            mask_groups.append((off, _mask_scores(r, o, stats, w_raw, w_of, len(models) > 0), boxes))
        if dev_groups is not None:
            dev_groups.append((off, scoring.cube_scores(r, o, cube_stat, stats, w_raw, w_of),
                               torch.from_numpy(scoring.box_rects(boxes, h, w)).to(device)))
        if map_groups is not None:
            map_groups.append(None if e is None else (e[0], e[1] if useFlow else None, stats, w_raw, w_of))
    return group


def _mask_lists(result_dir, pixel):
    """(mask_groups, dev_groups, map_groups) for a call: the host list feeds ``_save_masks``, the device lists ``_pixel_stage`` (and,
    with ``pixel.groups``, ``_smooth_stage`` and ``_render_stage`` once every call has been made)."""
    device_masks = pixel is not None and pixel.device_masks
    maps = pixel is not None and pixel.maps and (pixel.gt is not None or bool(pixel.error_dir))
    keep = pixel is not None and pixel.groups is not None
    return ([] if result_dir and not device_masks else None,
            [] if pixel is not None and (pixel.gt is not None or (device_masks and result_dir) or maps or keep) else None,
            [] if maps else None)


def _paint_frames(groups, a, b, h, w, device):
    """THE mask painter: the score masks of frames ``[a, b)`` on the device, float64 ``[b-a,h,w]`` -- every scored group of ``groups``
    ((off over all frames, device cube scores, device rectangles) each) painted into one buffer of ``-BIG``."""
    masks = _blank(device, b - a, h, w)
    for off, sc, rc in groups:
        if off[b] > off[a]:
            scoring.paint_masks(sc, off[a:b + 1], rc, h, w, out=masks)
    return masks


def _smooth_stage(groups, video_idx, n_frames, h, w, smooth_frames, smooth_pixels, frames_per_chunk, device, gt=None, percent=40,
                  result_dir=None):
    """``[mi355x] smooth_masks``: the score masks of all ``n_frames`` test frames, smoothed (``scoring.smooth_masks``), in chunks
    ``[a, b)`` of ``frames_per_chunk`` frames.  ``groups``: every scored group of the test set ((off over all frames, device cube scores,
    device rectangles) each); per chunk the frames ``[a - rt, b + rt)`` that exist (``rt = smooth_frames // 2``: the temporal halo) are
    painted on the device, group by group, and frames ``[a, b)`` of the filtered buffer are kept -- the chunk size changes nothing.
    ``video_idx``: the video of every test frame.  Returns ``(fs_smooth, ps_smooth)``, host float64 ``[n_frames]``: the smoothed frame
    scores (the maximum of every smoothed mask) and, with a ground-truth source ``gt``, the pixel criterion on the smoothed masks
    (``scoring.mask_pixel_scores``; else None).  ``result_dir``: the smoothed masks are saved there per frame, like the ``score_mask`` files."""
    video_idx = np.asarray(video_idx).reshape(-1)
    if video_idx.size != n_frames:
        raise ValueError('[mi355x] smooth_masks: the test split indexes {} frames, {} test frames are scored'.format(video_idx.size,
                                                                                                                    n_frames))
    fs = _blank(device, n_frames)
    ps = fs.clone() if gt is not None else None
    if result_dir:
        os.makedirs(result_dir, exist_ok=True)
    for a, b, pa, pb in _frame_chunks(0, n_frames, frames_per_chunk, halo=smooth_frames // 2):
        masks = _paint_frames(groups, pa, pb, h, w, device)
        smoothed, fmax = scoring.smooth_masks(masks, video_idx[pa:pb], smooth_frames, smooth_pixels, lo=a - pa, hi=b - pa)
        fs[a:b] = fmax
        if gt is not None:
            scoring.mask_pixel_scores(_gt_chunk(gt, range(a, b), device), smoothed, percent, out=ps[a:b])
        if result_dir:
            _save_frames(result_dir, a, smoothed)
    return fs.cpu().numpy(), ps.cpu().numpy() if ps is not None else None


def _render_range(groups, setting):
    """``[mi355x] render_range``: the ``(lo, hi)`` the colour table spans.  ``'auto'``: the smallest and the largest cube score of the
    run (``groups`` as for ``_smooth_stage``) among those with ``|v| < BIG`` -- the same for both sources; ``(0, 1)`` when there is none
    or they are equal."""
    if setting != 'auto':
        return float(setting[0]), float(setting[1])
    lo = hi = None
    for _, sc, _ in groups:
        v = sc[sc.abs() < BIG]
        if v.numel():
            lo = float(v.min()) if lo is None else min(lo, float(v.min()))
            hi = float(v.max()) if hi is None else max(hi, float(v.max()))
    return (0.0, 1.0) if lo is None or lo == hi else (lo, hi)


def _render_stage(c, groups, n_frames, h, w, device, out_dir, gt=None, video_idx=None, flownet2=None):
    """``[mi355x] render``: ``<out_dir>/<frame>.png`` for every ``render_every``-th test frame -- the frame with its score mask, the
    outlines of its scored boxes and the contour of its ground truth drawn over it (``render.overlay``) and, with ``render_flow``, the
    colour image of its flow field to the right (``render.flow_color``; ``[h, 2w, 3]``).  ``groups``: every scored group of the test set,
    as for ``_smooth_stage``.  Per chunk of ``direct_frames_per_chunk`` frames the picked frames are decoded and uploaded once, the chunk's
    masks are painted on the device (``render_source = smooth``: painted with the temporal halo and filtered as ``_smooth_stage`` does, so
    the values are those of the ``score_mask_smooth`` files; ``video_idx``: the video of every test frame), the pictures are composed on
    the device, come to the host in one copy and are written with Pillow (PNG: lossless).  ``gt``: a ground-truth source or None.  The
    flow of a frame is the field ``calc_optical_flow`` stores for it: read from ``optical_flow/``, or with ``direct_flow`` recomputed from
    the frames (``calc_optical_flow.flow_pairs`` + ``chunk_flows`` with ``flownet2``, ``direct_flow_pairs`` pairs per launch).  Returns the
    number of pictures written."""
    from PIL import Image
    from foreground import render_sources
    from vad_datasets import get_inputs
    from vec_vad_amd import render
    flow_files = c['render_flow'] and not c['direct_flow']
    frames_ds, flows_ds = render_sources(c, flow=flow_files)
    if len(frames_ds) != n_frames:
        raise ValueError('[mi355x] render: the test split indexes {} frames, {} test frames are scored'.format(len(frames_ds), n_frames))
    if c['render_flow'] and not flow_files:
        from calc_optical_flow import chunk_flows, flow_pairs, load_flownet2
        if flownet2 is None:
            flownet2 = load_flownet2(c['flownet2_checkpoint'], device=device, fp16=c['direct_flow_fp16'])
    smooth = c['render_source'] == 'smooth'
    if smooth:
        video_idx = np.asarray(video_idx).reshape(-1)
        if video_idx.size != n_frames:
            raise ValueError('[mi355x] render: the test split indexes {} frames, {} test frames are scored'.format(video_idx.size, n_frames))
    rt = c['smooth_frames'] // 2 if smooth else 0
    lo, hi = _render_range(groups, c['render_range'])
    alpha = (256 * c['render_alpha'] + 50) // 100
    lut = render.colormap()
    os.makedirs(out_dir, exist_ok=True)
    written = 0
    for a, b, pa, pb in _frame_chunks(0, n_frames, c['direct_frames_per_chunk'], halo=rt):
        sel = [f for f in range(a, b) if f % c['render_every'] == 0]
        if not sel:
            continue
        whole = len(sel) == b - a
        masks = _paint_frames(groups, pa, pb, h, w, device)
        if smooth:
            masks, _ = scoring.smooth_masks(masks, video_idx[pa:pb], c['smooth_frames'], c['smooth_pixels'], lo=a - pa, hi=b - pa)
        if not whole:
            masks = masks.index_select(0, torch.tensor([f - a for f in sel], device=device))
        off_s, sc_s, rc_s = scoring.merge_groups([], n_frames=len(sel), device=device)      # no box
        if c['render_boxes']:
            off_m, sc_s, rc_s = scoring.merge_groups([(off[a:b + 1], sc, rc) for off, sc, rc in groups], n_frames=b - a, device=device)
            if not whole:
                idx = torch.from_numpy(np.concatenate([np.arange(off_m[f - a], off_m[f - a + 1], dtype=np.int64) for f in sel])).to(device)
                sc_s, rc_s = sc_s.index_select(0, idx), rc_s.index_select(0, idx)
            off_s = np.concatenate([[0], np.cumsum(np.diff(off_m)[[f - a for f in sel]])]).astype(np.int32)
        # every frame the chunk needs -- the picked ones and, for a recomputed flow, their partners -- is decoded once
        pairs = flow_pairs(frames_ds, sel) if c['render_flow'] and not flow_files else []
        used = sorted(set(sel) | {f for p in pairs for f in p})
        local = {f: k for k, f in enumerate(used)}
        decoded = torch.from_numpy(np.ascontiguousarray(np.stack([get_inputs(frames_ds.all_frame_addr[f]) for f in used]))).to(device)
        picked = decoded if used == sel else decoded.index_select(0, torch.tensor([local[f] for f in sel], device=device))
        g = _gt_chunk(gt, sel, device) if gt is not None else None
        img = render.overlay(picked, masks, rc_s, sc_s, off_s, lo, hi, alpha, gt=g, lut=lut, bgr=True)
        if c['render_flow']:
            if flow_files:
                fl = torch.from_numpy(np.stack([np.asarray(get_inputs(flows_ds.all_frame_addr[f]), np.float32) for f in sel])).to(device)
            else:
                fl = torch.empty((len(sel), h, w, 2), dtype=torch.float32, device=device)
                chunk_flows(flownet2, decoded, [(local[p], local[q]) for p, q in pairs], np.arange(len(sel)), fl, max(1, c['direct_flow_pairs']))
            img = torch.cat([img, render.flow_color(fl, c['render_flow_max'])], dim=2)
        img = img.cpu().numpy()
        for k, f in enumerate(sel):
            Image.fromarray(img[k]).save(os.path.join(out_dir, '{}.png'.format(f)))
        written += len(sel)
    return written


class Vector(collections.namedtuple('Vector', 'name scores needs header summary per_scene device_line plain')):
    """One row of ``VECTORS``.  ``name``: also the stem of the ROC file; ``scores``: the stem of the score file; ``needs``: the config
    keys that must all be on for a run to have the vector; ``header`` / ``summary``: the line printed before / after its ROC is written
    (None: no line; formatted with the config and ``auc``); ``per_scene``: the summary of the per-scene evaluation that ShanghaiTech
    gets instead (None: evaluated like any dataset); ``device_line``: what the device pair-count line that follows calls the number
    (None: no such line); ``plain``: the vector its paired bootstrap difference is taken against."""
    __slots__ = ()

    def scores_path(self, ds, fg, method):
        return os.path.join('results', ds, '{}_{}_{}.npy'.format(self.scores, fg, method))

    def results_path(self, ds, mod, fg, method, scene=None):
        return os.path.join('results', ds, '{}_{}_{}_{}_results{}.npz'.format(mod, fg, method, self.name,
                                                                              '' if scene is None else '_scene_{}'.format(scene)))


_SMOOTHED = ' of the smoothed masks ({smooth_frames} frames x {smooth_pixels} x {smooth_pixels} pixels) is {auc}'
# every score vector a run can have, by name, in the order they are evaluated: plain vectors in front of the ones derived from them
VECTORS = {v.name: v for v in (
    Vector('frame', 'frame_scores', (), 'Evaluating {dataset_name} by frame-criterion:', None,
           'Average frame-level AUC is {auc}', 'AUC@ROC', None),
    Vector('frame_smooth', 'frame_scores_smooth', ('smooth_masks',), None, 'Frame-level AUC' + _SMOOTHED,
           'Average frame-level AUC' + _SMOOTHED, None, 'frame'),
    Vector('pixel', 'pixel_scores', ('pixel_criterion',), 'Evaluating {dataset_name} by pixel-criterion:',
           'Pixel-level AUC (overlap {pixel_overlap_percent}%) is {auc}', None, 'Pixel-level AUC@ROC', None),
    Vector('pixel_fine', 'pixel_scores_fine', ('pixel_criterion', 'pixel_maps'), None,
           'Fine pixel-level AUC (overlap {pixel_overlap_percent}%) is {auc}', None, 'Fine pixel-level AUC@ROC', 'pixel'),
    Vector('pixel_smooth', 'pixel_scores_smooth', ('pixel_criterion', 'smooth_masks'), None,
           'Pixel-level AUC of the smoothed masks (overlap {pixel_overlap_percent}%) is {auc}', None, None, 'pixel'),
)}


def _auc_stage(c, vectors, labels, video_idx, scene_idx, path_format, device, log=print):
    """``[mi355x] auc_statistics``: micro and macro AUROC with bootstrap intervals (``scoring.auc_bootstrap``) of every score vector of
    ``vectors`` (name -> host scores ``[n_frames]``; plain vectors in front of the ones derived from them), written to
    ``path_format.format(name)`` with ``micro_`` / ``macro_`` prefixed keys and printed, one line per statistic.  A vector with a
    ``plain`` counterpart in ``VECTORS`` also gets the paired difference against it (``scoring.auc_paired``; ``paired_`` prefixed keys).
    ``video_idx`` / ``scene_idx``: the video (and, for ShanghaiTech, the scene) of every test frame.  Returns name -> result."""
    video_idx = np.asarray(video_idx).reshape(-1)
    if video_idx.size != len(labels):
        raise ValueError('[mi355x] auc_statistics: the test split indexes {} frames, {} frame labels are given'.format(video_idx.size, len(labels)))
    kw = dict(replicates=c['auc_bootstrap'], unit=c['auc_bootstrap_unit'], block=c['auc_bootstrap_block'], seed=c['auc_bootstrap_seed'],
              confidence=c['auc_confidence'])
    what = '{}% interval of {} {} replicates'.format(kw['confidence'], kw['replicates'], kw['unit'] + (
        ' ({} frames)'.format(kw['block']) if kw['unit'] == 'block' else ''))
    plain = {name: VECTORS[name].plain for name in vectors if name in VECTORS and VECTORS[name].plain}
    done = {}
    for name, scores in vectors.items():
        res = scoring.auc_bootstrap(torch.from_numpy(np.asarray(scores, np.float64)).to(device), labels, video_idx, scene_idx, **kw)
        flat = scoring.auc_flatten(res)
        for kind in ('micro', 'macro'):
            e = res[kind]
            log('{} {} AUROC is {} [{}, {}] ({}, {} invalid; {} groups with both classes)'.format(
                name, kind, e['auc'], e['lo'], e['hi'], what, e['n_invalid'], e['n_groups_valid']))
        if name in plain:
            pair = scoring.auc_paired(res, done[plain[name]])
            flat.update(scoring.auc_flatten(pair, 'paired_'))
            for kind in ('micro', 'macro'):
                e = pair[kind]
                log('{} - {} {} AUROC is {} [{}, {}] ({} invalid; share of replicates with a difference <= 0: {})'.format(
                    name, plain[name], kind, e['diff'], e['lo'], e['hi'], e['n_invalid'], e['frac_le0']))
        np.savez(path_format.format(name), **flat)
        log('Results written to {}'.format(path_format.format(name)))
        done[name] = res
    return done


def score_frames(net_set, stats_raw, stats_of, foreground_set, foreground_set2, bbox_set, h, w, w_raw, w_of, useFlow,
                 device, score_batch=2048, scene_idx=None, result_dir=None, log=print, return_device=False, pixel=None):
    """Per-frame anomaly scores.  ``net_set[(s,)hh][ww]`` is a list with 0 or 1 eval-mode networks;
    ``stats_*[(s,)hh][ww]`` = (mean, std) of the training scores.

    The per-cube errors stay in HBM: ``vv_frame_scores`` z-normalises, weights and max-reduces them per frame
    (= the maximum of the reference's painted h x w mask, test.py:350-357,391).  Only when ``result_dir`` is given are the
    masks themselves painted (on the host) and saved as ``<result_dir>/<frame>`` like the reference does.

    ``pixel`` (a ``PixelEval``, default None: nothing below happens): the per-cube scores and rectangles of every group also stay on
    the device; with a ground-truth source the pixel scores of all frames go to ``pixel.out``, and with ``pixel.device_masks`` the
    ``result_dir`` masks are painted on the GPU (same files) and no per-cube score visits the host."""
    n_frames = len(foreground_set)
    mask_groups, dev_groups, map_groups = _mask_lists(result_dir, pixel)      # per scored group: (frame -> slice, host cube scores, boxes); masks are painted one frame at a time
    maps = map_groups is not None
    fs_dev = _blank(device, n_frames)
    hb, wb = len(foreground_set[0]), len(foreground_set[0][0])
    group = _group_scorer(net_set, stats_raw, stats_of, h, w, w_raw, w_of, useFlow, device, {}, fs_dev, mask_groups, dev_groups,
                          map_groups)
    keys = sorted(set(scene_idx[f] - 1 for f in range(n_frames))) if scene_idx is not None else [None]
    for hh in range(hb):
        for ww in range(wb):
            for key in keys:      # frames are grouped by the model that scores them (one per scene for ShanghaiTech)
                frames = [f for f in range(n_frames) if scene_idx is None or scene_idx[f] - 1 == key]
                counts = np.zeros(n_frames, np.int64)
                for f in frames:
                    counts[f] = len(foreground_set[f][hh][ww])
                if counts.sum() == 0:
                    continue
                frames = [f for f in frames if counts[f]]
                boxes = np.concatenate([np.asarray(bbox_set[f][hh][ww], dtype=np.float64)[:, :4] for f in frames])
                off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)      # indexed by frame: cubes of frame f = [off[f], off[f+1])
                group(key, hh, ww, int(off[-1]), off, boxes, lambda tr: score_cubes_device(
                    tr, [foreground_set[f][hh][ww] for f in frames], [foreground_set2[f][hh][ww] for f in frames], score_batch,
                    maps=maps))
    if mask_groups is not None:
        _save_masks(result_dir, range(n_frames), mask_groups, h, w)
    if dev_groups is not None:
        _pixel_stage(pixel, dev_groups, 0, n_frames, h, w, result_dir, device, map_groups)
        if pixel.groups is not None:
            pixel.groups += dev_groups
    return fs_dev if return_device else fs_dev.cpu().numpy()


def score_index_list(trainer, raw_store, flow_store, idx, score_batch, batch=None, maps=False):
    """Scores of the store cubes named by ``idx`` (int64 ``[n]``, numpy or device tensor, n > 0, repeats allowed): THE launch loop
    of the test stage.  Launches of exactly ``batch`` cubes -- default: ``score_batch``, or ``n`` when the list is shorter than one
    launch; ``score_cubes_device`` passes the size it derived from its whole list for every chunk --, the tail launch padded by
    repeating the last index.  Returns the DEVICE tensors (raw [n], of [n] | None) in list order; with ``maps`` also the per-pixel
    error maps (e_raw [n,32,32], e_of [n,32,32] | None) of the same cubes -- the padding of the tail launch is dropped from all four."""
    dev = trainer.bank.device
    n = len(idx)
    B = int(batch) if batch is not None else (n if n < score_batch else int(score_batch))
    idx_d = (idx if torch.is_tensor(idx) else torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))).to(dev)
    gathered = _Gathered(n, maps, dev)
    for s0 in range(0, n, B):
        m = min(B, n - s0)
        sel = idx_d[s0:s0 + m]
        if m < B:
            sel = torch.cat([sel, sel[-1:].expand(B - m)])
        gathered.put(s0, m, *(trainer.score_cubes(raw_store, flow_store, sel, maps=True) if maps
                              else trainer.score_cubes(raw_store, flow_store, sel)))
    return gathered.result()


def score_store(net_set, stats_raw, stats_of, store, groups, boxes, h, w, w_raw, w_of, useFlow, device, score_batch=2048,
                scene_idx=None, result_dir=None, out=None, frame_range=None, trainers=None, return_device=False, pixel=None):
    """``score_frames`` for a device-resident cube store (``foreground.extract_device``).  ``store`` = (raw uint8 ``[N,5,32,32,3]``,
    flow float32 ``[N,Tf,32,32,2]``) CUDA tensors in ``CubeStore`` layout; ``groups`` = ``{(scene, hh, ww): (idx, off)}`` as built by
    ``foreground.block_groups`` (scene = ``scene_idx[f] - 1`` when ``scene_idx`` is given, else None; ``off`` CSR over all frames);
    ``boxes`` float ``[N,>=4]``, one row per store cube.  A cube named by two index lists is stored once and scored once per list.

    Both routes run one group body (``_group_scorer``) and one launch loop (``score_index_list``, which ``score_cubes_device`` calls
    on its staging buffers), so the statistics, ``cube_stat``, paints and launch shapes -- hence the frame scores and the masks under
    ``result_dir`` -- are the staged path's by construction.  ``out`` (CUDA float64 ``[n_frames]``, initialised to ``-BIG``) is max-accumulated into: a test set that comes
    in several parts (``[mi355x] direct_max_cubes``) is scored part by part, with ``frame_range`` = the ``(first, end)`` frames whose
    masks this call writes (default: all) and ``trainers`` = a dict that keeps the engines between calls.  ``pixel``: as for
    ``score_frames``, for the frames of ``frame_range`` -- a part never splits a frame, so each call fills its own range of ``pixel.out``."""
    raw_store, flow_store = store
    boxes = np.asarray(boxes, dtype=np.float64).reshape(len(boxes), -1)[:, :4]
    if out is not None:
        n_frames = out.numel()
    elif groups:
        n_frames = len(next(iter(groups.values()))[1]) - 1
    elif frame_range is not None:
        n_frames = frame_range[1]
    else:
        raise ValueError('score_store: no group, no out and no frame_range to tell the number of frames')
    fs_dev = out if out is not None else _blank(device, n_frames)
    mask_groups, dev_groups, map_groups = _mask_lists(result_dir, pixel)
    maps = map_groups is not None
    group = _group_scorer(net_set, stats_raw, stats_of, h, w, w_raw, w_of, useFlow, device, {} if trainers is None else trainers,
                          fs_dev, mask_groups, dev_groups, map_groups)
    for gk in sorted(groups, key=lambda k: (k[1], k[2], -1 if k[0] is None else k[0])):
        if (gk[0] is None) != (scene_idx is None):
            raise ValueError('group %r does not fit scene_idx %s' % (gk, 'given' if scene_idx is not None else 'absent'))
        idx, off = groups[gk]
        if len(idx):
            group(*gk, len(idx), off, boxes[idx], lambda tr: score_index_list(tr, raw_store, flow_store, idx, score_batch, maps=maps))
    first, end = frame_range if frame_range is not None else (0, n_frames)
    if mask_groups is not None:
        _save_masks(result_dir, range(first, end), mask_groups, h, w)
    if dev_groups is not None:
        _pixel_stage(pixel, dev_groups, first, end, h, w, result_dir, device, map_groups)
        if pixel.groups is not None:
            pixel.groups += dev_groups
    return fs_dev if return_device else fs_dev.cpu().numpy()


def score_direct(c, device, mask_dir=None, log=print, flownet2=None, pixel=None):
    """``[mi355x] direct_test``: frames and boxes in, frame scores out.  The parts of ``foreground.extract_device`` are scored as
    they come and max-accumulated into one device vector; the store, the engines and their captured launches serve every part.
    ``flownet2``: the FlowNet2 that ``[mi355x] direct_flow`` computes the flow with (None: loaded from the configured checkpoint).
    ``pixel``: a function ``(n_frames, labels) -> PixelEval | None`` called once the extraction knows both; every part fills its own
    frame range of the pixel scores."""
    from foreground import extract_device
    ds, fg, method = c['dataset_name'], c['mode_fg'], c['method']
    base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
    h, w, _, _ = frame_size[ds]
    info, parts = extract_device(c, 'test', device, log, flownet2=flownet2)
    net_set, st_r, st_o = load_artifacts(base, fg, method, ds == 'ShanghaiTech', lambda: build_network(c), device, c['h_block'],
                                         c['w_block'])
    fs_dev = _blank(device, info['n_frames'])
    trainers = {}
    pixel = pixel(info['n_frames'], info['labels']) if pixel is not None else None
    for part in parts:
        score_store(net_set, st_r, st_o, (part['raw'], part['flow']), part['groups'], part['boxes'], h, w, c['w_raw'], c['w_of'],
                    c['useFlow'], device, c['score_batch'], info['scene_idx'], mask_dir, out=fs_dev, frame_range=part['frames'],
                    trainers=trainers, return_device=True, pixel=pixel)
    return fs_dev.cpu().numpy()


def _region_scores_path(c):
    return os.path.join('results', c['dataset_name'], 'region_scores_{}_{}.npz'.format(c['mode_fg'], c['method']))


def _load_scores(c):
    """``scores_saved = True``: what an earlier run left under ``results/<ds>/`` -> (name -> score vector for every row of ``VECTORS``
    whose keys are on, region scores | None)."""
    ds, fg, method = c['dataset_name'], c['mode_fg'], c['method']
    vectors = {v.name: np.load(v.scores_path(ds, fg, method)) for v in VECTORS.values() if all(c[key] for key in v.needs)}
    return vectors, dict(np.load(_region_scores_path(c))) if c['region_criterion'] else None


def _score(c, gt, device, flownet2=None):
    """Scores the test set on the staged or the direct route, then runs the stages that read the kept groups of the whole set
    (``smooth_masks``, ``render``).  ``gt``: the open ground-truth source or None.  Every score vector is saved under its ``VECTORS``
    path as soon as it exists.  Returns (name -> score vector, region scores | None) like ``_load_scores``."""
    ds, fg, method = c['dataset_name'], c['mode_fg'], c['method']
    shanghai = ds == 'ShanghaiTech'
    base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
    h, w, _, _ = frame_size[ds]
    if not c['direct_test'] and not c['cp'].getboolean(ds, 'test_foreground_saved'):   # test.py:98-176
        from foreground import extract_test
        extract_test(c, device)
    out_dir = os.path.join('results', ds)
    mask_dir = os.path.join(out_dir, 'score_mask') if c['save_score_masks'] else None
    error_dir = os.path.join(out_dir, 'error_mask') if c['save_score_masks'] and c['pixel_maps'] else None
    pix_gt = gt is not None and c['pixel_criterion']      # the pixel scores are wanted (the source may be open for the regions alone)
    maps = c['pixel_maps'] and (error_dir is not None or pix_gt)      # neither a file nor a score to form them for: off
    pixel = None

    def pixel_eval(n_frames, labels):
        """The ``pixel`` keyword of the scoring calls: None when no key asks for anything a ``PixelEval`` does."""
        nonlocal pixel
        if gt is None and not (c['device_score_masks'] and mask_dir) and not maps and not c['smooth_masks'] and not c['render']:
            return None
        if gt is not None and len(gt) != n_frames:
            raise ValueError('per-pixel ground truth for {} frames, {} test frames are scored'.format(len(gt), n_frames))
        out = _blank(device, n_frames) if pix_gt else None
        pixel = PixelEval(gt, c['pixel_overlap_percent'], out, labels, c['device_score_masks'], c['direct_frames_per_chunk'],
                          maps=maps, error_dir=error_dir, out_fine=out.clone() if maps and pix_gt else None, criterion=pix_gt,
                          regions=c['region_criterion'], region_iou=c['region_iou_percent'],
                          video_idx=gt.frame_video_idx if c['region_criterion'] else None, keep_groups=c['smooth_masks'] or c['render'])
        return pixel

    if c['direct_test']:      # frames -> scores without cube files
        fs = score_direct(c, device, mask_dir, flownet2=flownet2, pixel=pixel_eval)
    else:
        fset = np.load(base + 'foreground_test_{}-raw.npy'.format(fg), allow_pickle=True)
        fset2 = np.load(base + 'foreground_test_{}-flow.npy'.format(fg), allow_pickle=True)
        bset = np.load(base + 'foreground_bbox_test_{}.npy'.format(fg), allow_pickle=True)
        scene_idx = np.load(base + 'scene_idx.npy') if shanghai else None
        net_set, st_r, st_o = load_artifacts(base, fg, method, shanghai, lambda: build_network(c), device, c['h_block'], c['w_block'])
        lab_file = base + 'frame_labels_test.npy'
        fs = score_frames(net_set, st_r, st_o, fset, fset2, bset, h, w, c['w_raw'], c['w_of'], c['useFlow'], device,
                          c['score_batch'], scene_idx, mask_dir,
                          pixel=pixel_eval(len(fset), np.load(lab_file).astype(bool) if os.path.exists(lab_file) else None))
    os.makedirs(out_dir, exist_ok=True)
    vectors, regions = {}, None

    def put(name, scores):
        vectors[name] = scores
        np.save(VECTORS[name].scores_path(ds, fg, method), scores)

    put('frame', fs)
    if pix_gt:
        put('pixel', pixel.out.cpu().numpy())
        if pixel.maps:
            put('pixel_fine', pixel.out_fine.cpu().numpy())
    if c['region_criterion']:
        regions = pixel.region_state(c['track_percent'])
        if int(regions['n_frames']) != len(fs):
            raise ValueError('the region stage saw {} of the {} test frames'.format(int(regions['n_frames']), len(fs)))
        np.savez(_region_scores_path(c), **regions)
    if c['smooth_masks']:      # one stage over the kept groups of the whole test set, after all scoring
        fs_smooth, ps_smooth = _smooth_stage(
            pixel.groups, _video_idx(c, gt), len(fs), h, w, c['smooth_frames'], c['smooth_pixels'], c['direct_frames_per_chunk'],
            device, gt if pix_gt else None, c['pixel_overlap_percent'],
            os.path.join(out_dir, 'score_mask_smooth') if c['save_score_masks'] else None)
        put('frame_smooth', fs_smooth)
        if ps_smooth is not None:
            put('pixel_smooth', ps_smooth)
    if c['render']:            # pictures of the kept groups, after all scoring (and after the smooth stage, whose masks it may draw)
        render_gt = gt
        if render_gt is None and not shanghai:
            from foreground import gt_source
            try:
                render_gt = gt_source(c)      # the contour is drawn where the tree holds per-pixel ground truth
            except ValueError:
                render_gt = None
        render_dir = os.path.join(out_dir, 'render')
        print('Rendered {} frames to {}'.format(_render_stage(
            c, pixel.groups, len(fs), h, w, device, render_dir, render_gt,
            _video_idx(c, render_gt) if c['render_source'] == 'smooth' else None, flownet2), render_dir))
    return vectors, regions


def _scene_auc(scores, labels, scene_idx, path_of):
    """The ShanghaiTech protocol (test.py:366-392): the ROC of every scene on its own, written to ``path_of(scene)``; the mean AUROC."""
    return float(np.mean([save_roc_pr_curve_data(scores[scene_idx == si], labels[scene_idx == si], path_of(si))
                          for si in sorted(set(scene_idx))]))


def _region_results(c, regions):
    """criterion = 'region' / 'track' (scoring.py module docstring): needs no frame labels, only the region scores."""
    if regions is None:
        return
    ds = c['dataset_name']
    print('Evaluating {} by region- and track-criterion (regions and tracks derived from the per-pixel ground truth):'.format(ds))
    path = os.path.join('results', ds, '{}_{}_{}_region_results.npz'.format(c['modality'], c['mode_fg'], c['method']))
    fpr, rbdr, tbdr, rbdc, tbdc = scoring.region_curves(regions['region_score'], regions['track_score'], regions['fp_score'],
                                                        int(regions['n_frames']))
    np.savez(path, fpr=fpr, rbdr=rbdr, tbdr=tbdr, rbdc=rbdc, tbdc=tbdc)
    print('Results written to {}:'.format(path))
    print('RBDC (IoU {}%) is {}'.format(c['region_iou_percent'], rbdc))
    print('TBDC (IoU {}%, {}% of a track) is {}'.format(c['region_iou_percent'], c['track_percent'], tbdc))


def _evaluate(c, vectors, regions, gt, device):
    """The evaluation (test.py:362-399): every vector of ``vectors`` against the frame labels, row by row of ``VECTORS`` -- its ROC
    file and its printed lines --, then ``auc_statistics`` and the region criteria.  Returns the frame-level AUROC (the mean over the
    scenes for ShanghaiTech), or None without frame labels."""
    ds, fg, mod, method = c['dataset_name'], c['mode_fg'], c['modality'], c['method']
    base = os.path.join(c['data_root_dir'], mod, ds + '_')
    lab_path = base + 'frame_labels_test.npy'
    if not os.path.exists(lab_path):
        print('no {} -> frame-level evaluation skipped (ground-truth masks need the dataset frame indexers)'.format(lab_path))
        _region_results(c, regions)
        return None
    labels = np.load(lab_path).astype(bool)
    scene_idx = np.load(base + 'scene_idx.npy') if ds == 'ShanghaiTech' else None
    vectors = {name: vectors[name] for name in VECTORS if name in vectors}      # in the table's order
    auc = {}
    for name, scores in vectors.items():
        v = VECTORS[name]
        if v.header:
            print(v.header.format(**c))
        if scene_idx is not None and v.per_scene:
            auc[name] = _scene_auc(scores, labels, scene_idx, lambda si: v.results_path(ds, mod, fg, method, scene=si))
            print(v.per_scene.format(auc=auc[name], **c))
            continue
        path = v.results_path(ds, mod, fg, method)
        print('Results written to {}:'.format(path))
        auc[name] = save_roc_pr_curve_data(scores, labels, path)
        if v.summary:
            print(v.summary.format(auc=auc[name], **c))
        if v.device_line:
            # the same number from the device-side pair count (vv_roc_auc_counts); the .npz above keeps the reference's layout
            print('{} (device pair count) is {}'.format(v.device_line, scoring.roc_auc(
                torch.from_numpy(np.asarray(scores, np.float64)).to(device), labels)))
    if c['auc_statistics']:      # macro AUROC and bootstrap intervals of every score vector the run has, from the vectors alone
        print('Evaluating {} with bootstrap statistics:'.format(ds))
        _auc_stage(c, vectors, labels, _video_idx(c, gt), np.asarray(scene_idx).astype(np.int64) if scene_idx is not None else None,
                   os.path.join('results', ds, '{}_{}_{}_{{}}_bootstrap.npz'.format(mod, fg, method)), device)
    _region_results(c, regions)
    return auc['frame']


def main(config_path='config.cfg', flownet2=None):
    c = read_config(config_path)
    if c['direct_flow'] and not c['direct_test']:
        raise ValueError('[mi355x] direct_flow = True needs direct_test = True: only the direct test path computes the flow on the GPU')
    ds = c['dataset_name']
    saved = c['cp'].getboolean(ds, 'scores_saved')
    gt = None
    want_gt = c['pixel_criterion'] or c['region_criterion']      # either one opens the ground-truth source
    if want_gt and not saved:
        from foreground import gt_source
        gt = gt_source(c)                 # ShanghaiTech / a tree without per-pixel ground truth: refused before any GPU work
    elif want_gt and ds == 'ShanghaiTech':
        from foreground import PIXEL_GT_SHANGHAI
        raise ValueError(PIXEL_GT_SHANGHAI)
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(device)
    vectors, regions = _load_scores(c) if saved else _score(c, gt, device, flownet2)
    return _evaluate(c, vectors, regions, gt, device)


if __name__ == '__main__':
    main()
