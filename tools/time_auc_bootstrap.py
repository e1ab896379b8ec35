#!/usr/bin/env python
"""Time the bootstrap pair counts (``[mi355x] auc_statistics = True``): the device stage (``scoring.auc_counts_device``: every
``vv_auc_boot_counts`` call that ``--replicates`` replicates take, tables uploaded and scratch allocated once) next to the plain-numpy
restatement (``tests/auc_bootstrap_restatement.py``) on the host, at the sizes of the three datasets:

    UCSDped2      2010 frames,  12 videos,  1 stratum
    avenue       15324 frames,  21 videos,  1 stratum
    ShanghaiTech 40791 frames, 107 videos, 12 strata

with synthetic scores (rounded to two decimals: ties), both units (block of ``--block`` frames, video) and both groupings (micro: one
group, or one per scene; macro: one group per video).  The device stage is timed with device events: two warm-up runs, then the median
of ``--reps`` runs.  The restatement runs once per case on the host, for all replicates, and its counts must equal the device's.
Prints one JSON line per case and a last one with the ratios; needs the GPU.

    timeout 1500 python tools/time_auc_bootstrap.py [--replicates 1000] [--block 25] [--reps 20] [--sizes UCSDped2,avenue,ShanghaiTech]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {'UCSDped2': (2010, 12, 1), 'avenue': (15324, 21, 1), 'ShanghaiTech': (40791, 107, 12)}


def synthetic(n, V, S, seed=7):
    """(scores, labels, video, scene | None): V videos of uneven lengths that add up to n, S scenes of consecutive videos, an anomalous
    stretch in two videos of three."""
    rng = np.random.default_rng(seed)
    cut = np.sort(rng.choice(np.arange(1, n // 8), V - 1, replace=False)) * 8 if V > 1 else np.zeros(0, np.int64)
    off = np.concatenate([[0], cut, [n]]).astype(np.int64)
    lens = np.diff(off)
    labels = np.zeros(n, bool)
    for v in range(V):
        if v % 3 != 2:
            a = off[v] + int(lens[v]) // 3
            labels[a:a + max(1, int(lens[v]) // 4)] = True
    scores = np.round(rng.standard_normal(n) + 1.0 * labels, 2)
    video = np.repeat(np.arange(V), lens)
    scene = np.repeat(np.arange(V) * S // V, lens) if S > 1 else None
    return scores, labels, video, scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replicates', type=int, default=1000)
    ap.add_argument('--block', type=int, default=25)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sizes', default='UCSDped2,avenue,ShanghaiTech')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch
    from vec_vad_amd import scoring, _lib
    import auc_bootstrap_restatement as R
    if not torch.cuda.is_available():
        raise SystemExit('time_auc_bootstrap.py needs the GPU: a host timing says nothing about the device stage')
    R_ = a.replicates
    rows = []
    for size in a.sizes.split(','):
        n, V, S = SIZES[size]
        scores, labels, video, scene = synthetic(n, V, S)
        for grouping, groups in (('micro', scene), ('macro', video)):
            t = scoring.auc_tables_device(scoring.auc_tables(scores, labels, video, groups, scene), 'cuda')
            for unit in ('block', 'video'):
                need = int(_lib.lib().vv_auc_boot_work(n, V, R_, scoring.AUC_UNITS[unit]))
                work = torch.empty(max(8, min(need, scoring.AUC_WORK_BYTES)), dtype=torch.uint8, device='cuda')
                out = torch.empty((R_, t['G'], 3), dtype=torch.int64, device='cuda')

                def stage():
                    scoring.auc_counts_device(t, unit, a.block, 0, 1, R_, out=out, work=work)

                stage()
                stage()
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    stage()
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                t0 = time.perf_counter()
                want = R.counts(scores, labels, video, groups, unit, a.block, 0, 1, R_, scene)
                host_ms = 1e3 * (time.perf_counter() - t0)
                row = dict(size=size, frames=n, videos=V, strata=S, grouping=grouping, groups=t['G'], unit=unit, block=a.block,
                           replicates=R_, reps=a.reps, work_bytes=int(work.numel()),
                           device_ms=dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms))), host_restatement_ms=host_ms,
                           host_over_device=host_ms / float(np.median(ms)),
                           restatement_equals_device=bool(np.array_equal(out.cpu().numpy(), want)))
                rows.append(row)
                print(json.dumps(row), flush=True)
    worst = {size: min(r['host_over_device'] for r in rows if r['size'] == size) for size in a.sizes.split(',')}
    summary = dict(summary=True, smallest_host_over_device=worst, all_equal=all(r['restatement_equals_device'] for r in rows))
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(dict(rows=rows, **summary), f, indent=1)


if __name__ == '__main__':
    main()
