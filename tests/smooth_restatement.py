"""Plain-numpy restatement of the spatio-temporal mask smoothing ([mi355x] smooth_masks; include/vecvad_hip.h, vv_smooth_masks): what
tests/test_gpu_smooth.py compares the kernels with and tests/test_smooth_host.py checks on the CPU.  Nothing here imports the package.

Three separable passes of shifted adds; every sum starts from +0.0 and takes its terms in ascending offset order, left to right, in
float64 (numpy adds element by element: no pairwise or vector re-association happens inside ``a[...] += b[...]``), counts are int64."""
import numpy as np

BIG = 100000.0


def _shifted_sum(v, axis, r):
    """out[i] = v[i-r] + v[i-r+1] + ... + v[i+r] along ``axis``, terms outside the array left out, added in that order onto +0.0."""
    out = np.zeros_like(v)
    n = v.shape[axis]
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(n, n - d)              # destination range whose source i + d lies inside
        if hi <= lo:
            continue
        dst = [slice(None)] * v.ndim
        src = [slice(None)] * v.ndim
        dst[axis], src[axis] = slice(lo, hi), slice(lo + d, hi + d)
        out[tuple(dst)] += v[tuple(src)]
    return out


def smooth(masks, vid, kt, ks):
    """masks float64 [F,h,w] (-BIG = unpainted), vid [F], odd windows kt (frames) and ks (pixels) -> (S [F,h,w], frame maxima [F])."""
    masks = np.asarray(masks, np.float64)
    vid = np.asarray(vid).reshape(-1)
    F, h, w = masks.shape
    assert vid.size == F and kt % 2 == 1 and ks % 2 == 1
    rt, rs = kt // 2, ks // 2
    p = masks != -BIG
    V = np.where(p, masks, 0.0)
    N = p.astype(np.int64)
    A, a = _shifted_sum(V, 2, rs), _shifted_sum(N, 2, rs)
    B, b = _shifted_sum(A, 1, rs), _shifted_sum(a, 1, rs)
    C, c = np.zeros_like(B), np.zeros_like(b)
    for dt in range(-rt, rt + 1):
        for f in range(F):
            g = f + dt
            if 0 <= g < F and vid[g] == vid[f]:
                C[f] += B[g]
                c[f] += b[g]
    S = np.full(masks.shape, -BIG)
    S[p] = C[p] / c[p].astype(np.float64)
    return S, (S.reshape(F, -1).max(axis=1) if h * w else np.full(F, -BIG))


def brute(masks, vid, kt, ks):
    """The same filter as one 3-D window loop per painted pixel (frames outermost, then rows, then columns): another summation order,
    equal to ``smooth`` whenever every sum is exact (dyadic inputs)."""
    masks = np.asarray(masks, np.float64)
    F, h, w = masks.shape
    rt, rs = kt // 2, ks // 2
    S = np.full(masks.shape, -BIG)
    for f in range(F):
        frames = [g for g in range(max(0, f - rt), min(F, f + rt + 1)) if vid[g] == vid[f]]
        for y in range(h):
            for x in range(w):
                if masks[f, y, x] == -BIG:
                    continue
                tot, cnt = 0.0, 0
                for g in frames:
                    win = masks[g, max(0, y - rs):y + rs + 1, max(0, x - rs):x + rs + 1]
                    for v in win.reshape(-1):
                        if v != -BIG:
                            tot += float(v)
                            cnt += 1
                S[f, y, x] = tot / cnt
    return S
