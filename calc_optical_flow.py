"""Optical-flow extraction driver -- drop-in for the reference's ``calc_optical_flow.py``.

For every frame of a dataset (``unified_dataset_interface(..., context_frame_num=1, border_mode='hard')``) the flow to
the next frame is estimated by FlowNet2 at 512x384 and written, resized back to the frame size WITHOUT rescaling the
vectors, to ``./optical_flow/<same sub-path as the frame>/<frame name>.npy`` as ``[h,w,2]`` float32
(calc_optical_flow.py:12-85).

What runs where: decoded frames are uploaded once per frame triple; both cv2-style resizes (``vv_crop_resize``), the
whole FlowNet2 forward (``vv_conv2d_mfma`` + correlation / resample2d / channelnorm kernels, replayed from a hipGraph)
and the layout changes stay on the GPU; only the final ``[h,w,2]`` field comes back for ``np.save``.

``flow_pairs`` / ``chunk_flows`` are the same computation for test.py's direct path (``[mi355x] direct_flow``): the flow of many frames
of a chunk that is already on the device, written into a device tensor -- ``vv_flow_pairs_prep`` fills the captured graph's input,
the graph is replayed, ``vv_flow_resize_back`` reads its output; no file, no host copy, no framework kernel in between.
"""
import os

import numpy as np
import torch

from vad_datasets import context_range, unified_dataset_interface
from FlowNet2_src import FlowNet2
from vec_vad_amd.extract import crop_resize, flow_pairs_prep, flow_resize_back

FLOW_W, FLOW_H = 512, 384                    # cv2.resize(..., (512, 384)), calc_optical_flow.py:46-58
CHECKPOINT = 'FlowNet2_src/pretrained/FlowNet2_checkpoint.pth.tar'


def pair_of(frame_range):
    """Which two of the three context frames are matched (calc_optical_flow.py:43,61): normally (current, next); at a
    video border, where 'hard' clipping repeats the current frame, the first two entries."""
    if frame_range[1] == frame_range[0] or frame_range[1] == frame_range[2]:
        return 0, 1
    return 1, 2


def load_flownet2(path=CHECKPOINT, device='cuda', fp16=False):
    """calc_optical_flow.py:15-22: keep the checkpoint entries whose key exists in the model.  fp16=True: FlowNet2(fp16=True),
    fp16 activations on fp16 MFMA (the parameters and the written .npy files stay float32)."""
    net = FlowNet2(fp16=fp16)
    pretrained = torch.load(path, map_location='cpu', weights_only=False)['state_dict']
    own = net.state_dict()
    own.update({k: v for k, v in pretrained.items() if k in own})
    net.load_state_dict(own)
    return net.to(device).eval()


def flow_of_frames(flownet2, frames_chw, frame_range, graphed=True):
    """frames_chw: the dataset item, ``[3,C,H,W]`` (numpy or tensor, uint8 image frames).  Returns ``[H,W,2]`` float32
    (CUDA tensor)."""
    dev = next(flownet2.parameters()).device
    fr = torch.as_tensor(frames_chw).to(dev)
    if fr.dim() != 4 or fr.shape[0] != 3:
        raise ValueError('expected the 3-frame context stack [3,C,H,W] of context_frame_num=1, got %s' % (tuple(fr.shape),))
    a, b = pair_of(frame_range)
    pair = fr[[a, b]].permute(0, 2, 3, 1).contiguous()                       # [2,H,W,C]
    H, W = pair.shape[1], pair.shape[2]
    small = crop_resize(pair, np.array([[0, 0, W, H]], np.int32), FLOW_H, FLOW_W)[0]      # [2,384,512,C]
    if small.shape[3] == 1:
        small = small.expand(-1, -1, -1, 3)                                  # grey frames: same plane three times
    ims = small.permute(3, 0, 1, 2)[None].float().contiguous()               # [1,3,2,384,512], 0..255, BGR
    flow = (flownet2.forward_graphed(ims) if graphed else flownet2(ims))[0]  # [2,384,512]
    flow = flow.permute(1, 2, 0).contiguous()[None]                          # [1,384,512,2]
    return crop_resize(flow, np.array([[0, 0, FLOW_W, FLOW_H]], np.int32), H, W)[0, 0]


def flows_of_frames(flownet2, items, graphed=True):
    """Several frames per launch: ``items`` = [(frames_chw [3,C,H,W], frame_range), ...] of ONE frame size.  FlowNet2 at batch 1
    leaves most of the chip idle on its H/16 ... H/64 levels (a few hundred output pixels per layer); 4 pairs per launch take
    5.3 ms per pair instead of 6.8 on MI355X (1024x448), 8 pairs 5.0.  Returns a list of ``[H,W,2]`` float32 CUDA tensors.
    Per-pair results agree with the one-pair launch to fp32 round-off (the split-K choice of a layer depends on the batch)."""
    dev = next(flownet2.parameters()).device
    ims, sizes = [], []
    for frames_chw, frame_range in items:
        fr = torch.as_tensor(frames_chw).to(dev)
        if fr.dim() != 4 or fr.shape[0] != 3:
            raise ValueError('expected the 3-frame context stack [3,C,H,W] of context_frame_num=1, got %s' % (tuple(fr.shape),))
        a, b = pair_of(frame_range)
        pair = fr[[a, b]].permute(0, 2, 3, 1).contiguous()
        H, W = pair.shape[1], pair.shape[2]
        small = crop_resize(pair, np.array([[0, 0, W, H]], np.int32), FLOW_H, FLOW_W)[0]
        if small.shape[3] == 1:
            small = small.expand(-1, -1, -1, 3)
        ims.append(small.permute(3, 0, 1, 2).float())
        sizes.append((H, W))
    ims = torch.stack(ims).contiguous()                                      # [N,3,2,384,512]
    flow = flownet2.forward_graphed(ims) if graphed else flownet2(ims)       # [N,2,384,512]
    out = []
    for k, (H, W) in enumerate(sizes):
        f = flow[k].permute(1, 2, 0).contiguous()[None]
        out.append(crop_resize(f, np.array([[0, 0, FLOW_W, FLOW_H]], np.int32), H, W)[0, 0])
    return out


def flow_pairs(dataset_or_frame_video_idx, frames):
    """Pure, no GPU: for every global frame index ``f`` of ``frames`` the ``(first, second)`` frame whose flow ``calc_optical_flow``
    stores as ``<f>.npy`` -- ``pair_of`` applied to the 'hard' context of one frame each side: (f, f + 1) inside a video, (f, f) on a
    video's first frame, (f - 1, f) on its last, (f, f) when the dataset is one single frame.  The first argument is a dataset (any context and border
    mode: only its video structure is read) or its ``frame_video_idx`` list.  Raises NotImplementedError where ``context_range``
    does (a one-frame video next to another video), like the staged driver."""
    fvi = getattr(dataset_or_frame_video_idx, 'frame_video_idx', dataset_or_frame_video_idx)
    n = len(fvi)
    out = []
    for f in frames:
        r = context_range(int(f), 'hard', 1, n, fvi)
        a, b = pair_of(r)
        out.append((r[a], r[b]))
    return out


def launch_tables(pairs, rows, pairs_per_launch):
    """Pure, no GPU: ``pairs`` ``[n,2]`` and their output ``rows`` ``[n]`` cut into launches of exactly ``pairs_per_launch`` pairs, as
    a list of (int32 ``[P,2]``, int32 ``[P]``).  The tail launch repeats its last pair with row -1 (computed, not written), so one
    captured graph serves any number of pairs."""
    P = int(pairs_per_launch)
    if P < 1:
        raise ValueError('pairs_per_launch must be at least 1, got %d' % P)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    rows = np.asarray(rows, np.int32).reshape(-1)
    if len(rows) != len(pairs):
        raise ValueError('one row per pair: %d rows for %d pairs' % (len(rows), len(pairs)))
    out = []
    for s in range(0, len(pairs), P):
        p, r = pairs[s:s + P], rows[s:s + P]
        pad = P - len(p)
        if pad:
            p = np.concatenate([p, np.repeat(p[-1:], pad, axis=0)])
            r = np.concatenate([r, np.full(pad, -1, np.int32)])
        out.append((np.ascontiguousarray(p), np.ascontiguousarray(r)))
    return out


def chunk_flows(flownet2, frames_u8, pairs, rows, out, pairs_per_launch=4):
    """``out[rows[i]]`` (CUDA float32 ``[R,H,W,2]``) = the flow of ``pairs[i]``, what ``flow_of_frames`` returns for that pair.
    frames_u8: CUDA uint8 ``[F,H,W,C]``, the decoded frames of a chunk; pairs ``[n,2]`` index it.  Every launch carries exactly
    ``pairs_per_launch`` pairs at 512x384 (``launch_tables``): ``vv_flow_pairs_prep`` writes the input buffer of the graph captured
    for that shape (``FlowNet2.graph_entry``), the graph is replayed, ``vv_flow_resize_back`` reads its output buffer.  A flow
    depends on its two frames and on ``pairs_per_launch`` (a layer's split-K choice depends on the batch), not on the chunk."""
    H, W = frames_u8.shape[1], frames_u8.shape[2]
    tables = launch_tables(pairs, rows, pairs_per_launch)
    if not tables:
        return out
    static_in, static_out, graph = flownet2.graph_entry((int(pairs_per_launch), 3, 2, FLOW_H, FLOW_W))
    for p, r in tables:
        flow_pairs_prep(frames_u8, p, FLOW_H, FLOW_W, out=static_in)
        graph.replay()
        flow_resize_back(static_out, r, H, W, out)
    return out


def flow_path(dataset, idx, of_root_dir='./optical_flow'):
    """optical_flow/<dataset dir components below the dataset root's parent>/<frame name>.npy (calc_optical_flow.py:13,27-37)."""
    skip = len(dataset.dir.split('/')) - 1
    addr = dataset.all_frame_addr[idx]
    name = addr.split('/')[-1].split('.')[0]
    return os.path.join(of_root_dir, *addr.split('/')[skip:-1]), name + '.npy'


def calc_optical_flow(dataset, flownet2=None, of_root_dir='./optical_flow', log=print, pairs_per_launch=4):
    """pairs_per_launch = 1 is the reference's frame-by-frame loop (calc_optical_flow.py:39-85); the default groups consecutive
    frames of equal size into one FlowNet2 launch (``flows_of_frames``)."""
    if flownet2 is None:
        flownet2 = load_flownet2()

    def save(idx, flow):
        of_path, fname = flow_path(dataset, idx, of_root_dir)
        os.makedirs(of_path, exist_ok=True)
        np.save(os.path.join(of_path, fname), flow.cpu().numpy())

    pend = []          # (idx, frames, frame_range) of one frame size

    def flush():
        if len(pend) == 1:
            save(pend[0][0], flow_of_frames(flownet2, pend[0][1], pend[0][2]))
        elif pend:
            for (idx, _, _), flow in zip(pend, flows_of_frames(flownet2, [(f, r) for _, f, r in pend])):
                save(idx, flow)
        del pend[:]

    for idx in range(len(dataset)):
        log('Calculating optical flow for {}-th frame'.format(idx + 1))
        batch, _ = dataset[idx]
        if pend and tuple(np.shape(batch)) != tuple(np.shape(pend[0][1])):
            flush()
        pend.append((idx, batch, dataset.context_range(idx)))
        if len(pend) >= max(1, pairs_per_launch):
            flush()
    flush()


if __name__ == '__main__':
    # Same example as the reference (calc_optical_flow.py:105-112); change dataset_name for the other datasets.
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--fp16', action='store_true', help='FlowNet2(fp16=True): fp16 activations, fp32 arithmetic')
    args = ap.parse_args()
    dataset_name = 'UCSDped2'
    net = load_flownet2(fp16=args.fp16)
    for mode in ('train', 'test'):
        calc_optical_flow(unified_dataset_interface(dataset_name=dataset_name, dir=os.path.join('raw_datasets', dataset_name),
                                                    context_frame_num=1, mode=mode, border_mode='hard'), flownet2=net)
