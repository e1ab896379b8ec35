#!/usr/bin/env python
"""Paired comparison of the score files of two runs on the same test split -- fp32 against ``precision = bf16``, ``direct_flow_fp16`` on
against off, smoothed against plain: is the difference of their AUROCs more than resampling noise?

    python tools/compare_scores.py A.npy B.npy [--config config.cfg]

``A.npy`` / ``B.npy``: two per-frame score vectors ``test.py`` saved (``results/<ds>/frame_scores_*.npy``, ``pixel_scores_*.npy``, ...).
The config names the dataset (frame labels ``<data_root>/<modality>/<ds>_frame_labels_test.npy``, the test split's videos, for
ShanghaiTech ``<ds>_scene_idx.npy``) and the ``[mi355x] auc_*`` settings.  Both vectors are bootstrapped with the same seed, so replicate
``r`` of both saw the same resample (``scoring.auc_bootstrap`` / ``auc_paired``).  Prints, for the micro and the macro AUROC, both numbers
with their intervals and the difference A - B with its interval and the share of replicates whose difference is <= 0 -- that share is
reported as it is; it is not a p-value.  With ``auc_bootstrap = 0`` only the AUROCs and their difference are printed.  Needs the GPU.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(a, b, c, log=print):
    """The comparison of two score vectors under the read config ``c``: (result of A, result of B, paired A - B)."""
    import torch
    from foreground import test_video_idx
    from vec_vad_amd import scoring
    ds = c['dataset_name']
    base = os.path.join(c['data_root_dir'], c['modality'], ds + '_')
    labels = np.load(base + 'frame_labels_test.npy').astype(bool)
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if a.size != labels.size or b.size != labels.size:
        raise ValueError('{} and {} scores for {} frame labels'.format(a.size, b.size, labels.size))
    scene_idx = np.load(base + 'scene_idx.npy').astype(np.int64) if ds == 'ShanghaiTech' else None
    video_idx = test_video_idx(c)
    kw = dict(replicates=c['auc_bootstrap'], unit=c['auc_bootstrap_unit'], block=c['auc_bootstrap_block'], seed=c['auc_bootstrap_seed'],
              confidence=c['auc_confidence'])
    dev = torch.device('cuda', torch.cuda.current_device())
    res = [scoring.auc_bootstrap(torch.from_numpy(v).to(dev), labels, video_idx, scene_idx, **kw) for v in (a, b)]
    pair = scoring.auc_paired(res[0], res[1])
    log('{}% intervals of {} {} replicates{}, seed {}'.format(kw['confidence'], kw['replicates'], kw['unit'],
                                                                ' ({} frames)'.format(kw['block']) if kw['unit'] == 'block' else '', kw['seed']))
    for kind in ('micro', 'macro'):
        for name, r in (('A', res[0][kind]), ('B', res[1][kind])):
            log('{} {} AUROC is {} [{}, {}] ({} invalid; {} groups with both classes)'.format(
                name, kind, r['auc'], r['lo'], r['hi'], r['n_invalid'], r['n_groups_valid']))
        p = pair[kind]
        log('A - B {} AUROC is {} [{}, {}] ({} invalid; share of replicates with a difference <= 0: {})'.format(
            kind, p['diff'], p['lo'], p['hi'], p['n_invalid'], p['frac_le0']))
    return res[0], res[1], pair


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--config', default='config.cfg')
    args = ap.parse_args(argv)
    sys.path.insert(0, ROOT)
    from train import read_config
    return compare(np.load(args.a), np.load(args.b), read_config(args.config))


if __name__ == '__main__':
    main()
