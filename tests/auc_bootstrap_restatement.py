"""Plain numpy / Python-integer restatement of the macro AUROC and bootstrap statistics ([mi355x] auc_statistics), written from the
contract in include/vecvad_hip.h (vv_auc_boot_counts) and the docstrings of vec_vad_amd/scoring.py, not from the kernels: the counter-based
draw, the frame weights of both resampling units, the weighted tie-aware pair counts per group, the statistic of a replicate, the
percentile interval with its 5 % rule and the paired comparison.  Every count is a Python integer or an int64; nothing is accumulated
in floating point before the one quotient per group."""
import math
import warnings

import numpy as np

M64 = (1 << 64) - 1


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw(seed, r, s, j, m):
    return ((mix(mix(mix(mix(seed) ^ r) ^ s) ^ j) >> 32) * m) >> 32


def runs(idx):
    """CSR offsets of the contiguous runs of equal values in ``idx``."""
    idx = np.asarray(idx).reshape(-1)
    return np.concatenate([[0], np.nonzero(idx[1:] != idx[:-1])[0] + 1, [idx.size]]).astype(np.int64) if idx.size else np.zeros(1, np.int64)


def multiplicities(seed, r, stratum_off):
    """unit = VIDEO: how often every video is picked in replicate ``r``."""
    mult = np.zeros(int(stratum_off[-1]), np.int64)
    for s in range(len(stratum_off) - 1):
        first, vs = int(stratum_off[s]), int(stratum_off[s + 1] - stratum_off[s])
        for j in range(vs):
            mult[first + draw(seed, r, s, j, vs)] += 1
    return mult


def weights(unit, seed, r, video_off, stratum_off=None, block=1):
    """The frame weights of replicate ``r``: int64 ``[n]``."""
    video_off = [int(v) for v in video_off]
    n, V = video_off[-1], len(video_off) - 1
    if unit == 'none':
        return np.ones(n, np.int64)
    if unit == 'video':
        return np.repeat(multiplicities(seed, r, [0, V] if stratum_off is None else stratum_off), np.diff(video_off))
    assert unit == 'block'
    w = np.zeros(n, np.int64)
    for v in range(V):
        a, L = video_off[v], video_off[v + 1] - video_off[v]
        if L == 0:
            continue
        b = min(block, L)
        for j in range(-(-L // b)):
            start = draw(seed, r, (1 << 32) + v, j, L - b + 1)
            w[a + start:a + start + b] += 1
    return w


def group_counts(scores, labels, w):
    """(U2, P, N) of one group as Python integers: per distinct score the weighted negatives, their running sum below it, and for every
    positive ``w * (2 * below + tied)``."""
    scores, labels, w = np.asarray(scores, np.float64), np.asarray(labels).astype(bool), np.asarray(w, np.int64)
    values, rank = np.unique(scores, return_inverse=True)
    neg = np.zeros(values.size, np.int64)
    np.add.at(neg, rank[~labels], w[~labels])
    below = np.concatenate([[0], np.cumsum(neg)[:-1]]) if values.size else neg
    u2 = sum(int(wi) * (2 * int(below[k]) + int(neg[k])) for wi, k in zip(w[labels], rank[labels]))
    return u2, int(w[labels].sum()), int(w[~labels].sum())


def group_members(groups, n):
    """groups ``[n]`` (None: one group) -> the frame indices of every group, groups in ascending order of their ids."""
    if groups is None:
        return [np.arange(n)]
    groups = np.asarray(groups).reshape(-1)
    return [np.nonzero(groups == g)[0] for g in np.unique(groups)]


def counts(scores, labels, video_idx, groups, unit, block, seed, r0, R, strata=None):
    """int64 ``[R, G, 3]``: what ``scoring.auc_counts`` returns."""
    scores, labels = np.asarray(scores, np.float64).reshape(-1), np.asarray(labels).reshape(-1) != 0
    video_off = runs(video_idx)
    stratum_off = None if strata is None else runs(np.asarray(strata).reshape(-1)[video_off[:-1]])
    members = group_members(groups, scores.size)
    out = np.zeros((R, len(members), 3), np.int64)
    for k in range(R):
        w = weights(unit, seed, r0 + k, video_off, stratum_off, block)
        for g, idx in enumerate(members):
            out[k, g] = group_counts(scores[idx], labels[idx], w[idx])
    return out


def statistic(c):
    """(statistic, valid groups) of one replicate's ``[G, 3]`` counts."""
    aucs = [float(int(u2)) / (2.0 * float(int(p)) * float(int(q))) for u2, p, q in np.asarray(c).reshape(-1, 3) if p > 0 and q > 0]
    return (math.fsum(aucs) / len(aucs), len(aucs)) if aucs else (float('nan'), 0)


def interval(reps, confidence):
    """(lo, hi, n_invalid); NaN bounds and a warning when more than 5 % of the replicates are invalid."""
    reps = np.asarray(reps, np.float64)
    a = np.sort(reps[~np.isnan(reps)])
    n_invalid, M = int(reps.size - a.size), int(a.size)
    if n_invalid * 20 > reps.size:
        warnings.warn('%d of %d replicates are invalid' % (n_invalid, reps.size))
        return float('nan'), float('nan'), n_invalid
    if M == 0:
        return float('nan'), float('nan'), n_invalid
    k = ((100 - confidence) * (M - 1)) // 200
    return float(a[k]), float(a[M - 1 - k]), n_invalid


def bootstrap(scores, labels, video_idx, scene_idx=None, replicates=1000, unit='block', block=25, seed=0, confidence=95):
    """What ``scoring.auc_bootstrap`` returns."""
    video_off = runs(video_idx)
    video = np.repeat(np.arange(video_off.size - 1), np.diff(video_off))
    out = {}
    for name, groups in (('micro', scene_idx), ('macro', video)):
        auc, n_valid = statistic(counts(scores, labels, video, groups, 'none', 1, 0, 1, 1)[0])
        reps = np.array([statistic(c)[0] for c in counts(scores, labels, video, groups, unit, block, seed, 1, replicates, scene_idx)],
                        np.float64).reshape(-1)
        lo, hi, n_invalid = interval(reps, confidence) if replicates else (float('nan'), float('nan'), 0)
        out[name] = dict(auc=auc, replicates=reps, lo=lo, hi=hi, n_invalid=n_invalid, n_groups_valid=n_valid, n_replicates=replicates,
                         unit=unit, block=block, seed=seed, confidence=confidence)
    return out


def paired(a, b):
    """What ``scoring.auc_paired`` returns for two entries."""
    d = np.asarray(a['replicates'], np.float64) - np.asarray(b['replicates'], np.float64)
    lo, hi, n_invalid = interval(d, a['confidence']) if d.size else (float('nan'), float('nan'), 0)
    ok = d[~np.isnan(d)]
    return dict(diff=a['auc'] - b['auc'], replicates=d, lo=lo, hi=hi, n_invalid=n_invalid,
                frac_le0=float((ok <= 0).sum()) / ok.size if ok.size else float('nan'))


def array_set(seed=20):
    """The array set of the tests: 6 videos of 120 / 180 / 150 / 200 / 90 / 170 frames (910 in all), the third all-normal, the fifth
    all-anomalous, the others with one anomalous stretch each; scores rounded to two decimals (ties).  Returns (scores, labels, video)."""
    rng = np.random.default_rng(seed)
    lens = [120, 180, 150, 200, 90, 170]
    labels = []
    for v, L in enumerate(lens):
        lab = np.zeros(L, bool)
        if v == 4:
            lab[:] = True
        elif v != 2:
            a = int(rng.integers(L // 8, L // 2))
            lab[a:a + int(rng.integers(L // 5, L // 2))] = True
        labels.append(lab)
    labels = np.concatenate(labels)
    scores = np.round(rng.standard_normal(labels.size) + 1.0 * labels, 2)
    return scores, labels, np.repeat(np.arange(1, len(lens) + 1), lens)


def entries_equal(a, b):
    """Two entries (or flat dicts) hold the same keys and, bit for bit, the same values (NaN equals NaN)."""
    return sorted(a) == sorted(b) and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=np.asarray(a[k]).dtype.kind == 'f')
                                          for k in a)
