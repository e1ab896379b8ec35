#!/usr/bin/env python
"""``python stream_train.py`` -- the configured training split pushed frame by frame, as a camera would deliver it, and trained from.

Every video of the split goes through ONE ``vec_vad_amd.stream_train.StreamCollector`` one frame at a time: boxes from
``foreground.load_bboxes(c, 'train')``, videos from the split's frame indexer.  The collector computes the flow, cuts the cubes and
packs the kept ones into one device-resident training store; then every block trains from its index list (``train.train_store``) and
the three files of ``train.py`` are written: ``<ds>_model_<mode>_<method>.npy`` and ``<ds>_{raw,of}_training_scores_<mode>_<method>.npy``
under ``<data_root_dir>/<modality>/``.  On the same frames and boxes they are, bit for bit, those of ``train.py`` with ``[mi355x]
direct_train``, ``direct_flow`` and one pair per FlowNet2 launch.  Nothing under ``optical_flow/`` and no cube file is read or written.

With ``[mi355x] stream_boxes = motion`` no ``bboxes_train_*`` file is loaded or written either: every push hands over the frame and
the rows of ``bboxes_train_obj_det.npy`` for it (when that file exists; none otherwise), and the collector finds the motion boxes
itself, so the boxes are those of ``train_bbox_saved = False`` in mode ``obj_det_with_motion`` (another
``foreground_extraction_mode`` is refused).  The number of motion boxes that found no free slot is printed when it is not 0.

``main`` returns what ``StreamCollector.train`` returns, ``(net_set, stats_raw, stats_of)`` as ``test.load_artifacts`` forms them.
ShanghaiTech (one model per scene) and a ``torchrun`` world above 1 are refused before any GPU work.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from train import DIRECT_TRAIN_SHANGHAI, build_network, read_config  # noqa: E402


def main(config_path='config.cfg', flownet2=None):
    c = read_config(config_path)                      # a bad [mi355x] collect_max_cubes / stream_max_boxes / stream_boxes raises here
    ds = c['dataset_name']
    if ds == 'ShanghaiTech':                          # before any GPU work
        raise NotImplementedError(DIRECT_TRAIN_SHANGHAI)
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world > 1:
        raise ValueError('stream_train.py collects and trains in one process: a torchrun world of {} is refused (train.py trains '
                         'data-parallel from cube files or with direct_train)'.format(world))
    motion = c['stream_boxes'] == 'motion'
    if motion and c['mode_fg'] != 'obj_det_with_motion':
        raise ValueError("[mi355x] stream_boxes = motion collects the boxes of mode obj_det_with_motion; the configured mode is "
                         "{!r}".format(c['mode_fg']))
    import foreground as FG
    from stream import _detector_boxes
    from vad_datasets import get_inputs
    from vec_vad_amd.stream_train import StreamCollector
    device = torch.device('cuda', int(os.environ.get('LOCAL_RANK', '0')))
    torch.cuda.set_device(device)
    net = build_network(c)                            # before FlowNet2 is loaded: that must not move the random state of the weights
    if motion:                                        # the frame indexer alone: no bboxes_train_* file is loaded or written
        indexer = FG._datasets(c, 'train', None, direct_flow=True)[0]
        boxes = _detector_boxes(c, len(indexer), 'train')
    else:
        st = FG._stage(c, 'train', direct_flow=True)  # boxes and the frame indexer over the raw tree; no flow file is globbed
        indexer, boxes = st.raw_ds, st.boxes
    n = len(indexer)
    col = None
    for i in range(n):
        frame = get_inputs(indexer.all_frame_addr[i])
        if i > 0 and indexer.frame_video_idx[i] != indexer.frame_video_idx[i - 1]:
            col.end_video()
        if col is None:
            if flownet2 is None:
                from calc_optical_flow import load_flownet2
                flownet2 = load_flownet2(c['flownet2_checkpoint'], device=device, fp16=c['direct_flow_fp16'])
            col = StreamCollector(c, frame.shape, flownet2=flownet2, device=device)
        if motion:
            col.push(frame, ap_boxes=boxes[i])
        else:
            col.push(frame, boxes[i])
        if (i + 1) % 64 == 0 or i + 1 == n:
            print('Collecting foreground of frames {}-{}, {} in total'.format(i // 64 * 64 + 1, i + 1, n))
    if col is None:
        raise ValueError('the training split of {} has no frames'.format(ds))
    store = col.finish()
    print('foreground for training data collected: {} cubes of {} frames in the device store'.format(store['n'], store['n_frames']))
    if store['dropped_boxes']:
        print('{} motion boxes found no free slot and were dropped: raise [mi355x] stream_max_boxes ({})'.format(
            store['dropped_boxes'], c['stream_max_boxes']))
    return col.train(net=net, save=True)


if __name__ == '__main__':
    main()
