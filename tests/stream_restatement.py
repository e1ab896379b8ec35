"""numpy float64 restatement of the masked score reduction of ``vv_stream_scores`` (include/vecvad_hip.h), shared by
tests/test_stream_host.py and tests/test_gpu_stream.py.  Every product, quotient and sum is a separate float64 numpy operation, like
the kernel's (FMA contraction off), so the kernel is compared with it bit for bit."""
import numpy as np

BIG = 100000


def stream_scores(raw, of, stats, w_raw, w_of, keep, n, mask, box_scores, frame_score, big=BIG):
    """One launch.  raw / of: float32 ``[cap]`` error sums (``of`` None drops the flow term); stats: ``(mu_r, sd_r, mu_o, sd_o)`` or
    None for a block without a model; keep / mask: ``[cap]`` flags; n: boxes of the round; box_scores: float64 ``[cap]`` as it stands
    before the launch; frame_score: the cell before the launch.  Returns ``(box_scores, frame_score)`` after it: a box ``b < n`` with
    ``keep[b]`` and ``mask[b]`` gets its score and enters the maximum, another box below ``n`` gets ``-big``, slots ``>= n`` keep what
    they hold; values of boxes that do not count are never looked at."""
    cap = len(box_scores)
    n = min(max(int(n), 0), cap)
    out = np.array(box_scores, np.float64)
    best = np.float64(frame_score)
    for b in range(n):
        if keep[b] and mask[b]:
            if stats is None:
                s = np.float64(big)
            else:
                s = np.float64(w_raw) * ((np.float64(np.float32(raw[b])) - np.float64(stats[0])) / np.float64(stats[1]))
                if of is not None:
                    s = s + np.float64(w_of) * ((np.float64(np.float32(of[b])) - np.float64(stats[2])) / np.float64(stats[3]))
            out[b] = s
            if s > best:                 # fmax: a NaN score (outside the domain) is dropped
                best = s
        else:
            out[b] = -np.float64(big)
    return out, float(best)
