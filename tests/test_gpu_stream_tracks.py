"""GPU: the tracks of a stream (vec_vad_amd/stream.py: tracks) -- ``vv_stream_tracks`` against the numpy restatement of
tests/stream_tracks_restatement.py over the hand-made and the random sequences of tests/test_stream_tracks_host.py, the whole state
(``t_meta``, ``t_hist``, ``next_id``) behind every frame included; ``StreamScorer(tracks=True)`` against the restatement fed with what
``wait()`` returns and against a scorer with the switch off; ``stream.main`` with the key on.  Every comparison is bit for bit: the
geometry is in integers, and every sum is taken in one stated order on both sides."""
import glob
import os

import numpy as np
import pytest
import torch

import stream_tracks_restatement as R
from test_gpu_stream import N_VIDEO, _stream, net, tree  # noqa: F401  (the fixtures of the synthetic tree)
from test_gpu_stream_masks import KS, KT, _keep_all, _run
from test_stream_tracks_host import H, RANDOM_SETTINGS, SEQUENCES, W, frame_arrays, random_sequence, run_restatement

pytestmark = pytest.mark.gpu

BIG = R.BIG


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. vv_stream_tracks over sequences ------------------------------------------------------------------------------------------------
def _kernel_over(settings, frames, host, width_of):
    """The frames of a sequence through ``stream_tracks``, the state staying on the device, against the restatement frame by frame.
    ``host``: how many of the rectangles are the host's (none | some | half | all | all-no-table).  Slots at or above n hold NaN, Inf and
    1e30 scores and whole-frame boxes and rectangles; the rectangles the host does not give are garbage too.  The table starts out
    full of garbage, which the first frame's reset has to clear.  Returns the restatement's tracker."""
    from vec_vad_amd.stream import stream_tracks
    steps, tr = run_restatement(settings, frames)
    mt, window = tr.meta.shape[0], tr.window
    t_meta = torch.full((mt, 8), 9, dtype=torch.int32, device='cuda')
    t_hist = torch.full((mt, window), float('nan'), dtype=torch.float64, device='cuda')
    next_id = torch.ones(1, dtype=torch.int32, device='cuda')
    for f, (frame, (want, want_meta, want_hist)) in enumerate(zip(frames, steps)):
        boxes, rows, reset = frame_arrays(frame)
        n, width = len(boxes), width_of(len(boxes))
        n_host = {'none': 0, 'some': n // 3, 'half': n // 2, 'all': n, 'all-no-table': n}[host]
        all_rows = np.tile(np.array([[np.nan, np.inf, 1e30]]), (rows.shape[0], width))[:, :width].copy()      # what must never be read
        all_rows[:, :n] = rows
        all_boxes = np.tile(np.array([[0, 0, W, H]], np.int32), (width, 1))
        all_boxes[:n] = boxes
        rects = np.tile(np.array([[0, H, 0, W]], np.int32), (width, 1))
        rects[:n_host] = R.resolve(boxes[:n_host], H, W)
        d_rects, d_track, d_score = cu(rects), cu(np.full((width, 2), 77, np.int32)), cu(np.full(width, 55.5))
        frame_score, counts = cu(np.array([55.5])), cu(np.full(3, 77, np.int32))
        stream_tracks(t_meta, t_hist, next_id, cu(all_rows), cu(np.array([n], np.int32)), n_host, d_rects,
                      None if host == 'all-no-table' else cu(all_boxes), H, W, reset, tr.iou_pct, tr.max_age, tr.min_hits, d_track, d_score,
                      frame_score, counts)
        got_track, got_score = d_track.cpu().numpy(), d_score.cpu().numpy()
        assert got_track[:n, 0].tolist() == want['ids'].tolist() and got_track[:n, 1].tolist() == want['hits'].tolist(), f
        assert np.array_equal(_bits(got_score[:n]), _bits(want['scores'])), f
        assert (got_track[n:] == 77).all() and (got_score[n:] == 55.5).all(), f              # slots at or above n: not written
        assert np.array_equal(d_rects.cpu().numpy(), rects), f                              # the rectangles are only read
        assert _bits(frame_score.cpu().numpy())[0] == _bits(want['score']), f
        assert counts.tolist() == [want['live'], want['dropped'], want['next_id']] and next_id.tolist() == [want['next_id']], f
        assert np.array_equal(t_meta.cpu().numpy(), want_meta), f
        assert np.array_equal(_bits(t_hist.cpu().numpy()), _bits(want_hist)), f
    return tr


@pytest.mark.parametrize('host', ['none', 'some', 'all', 'all-no-table'])
@pytest.mark.parametrize('name', sorted(SEQUENCES))
def test_stream_tracks_equals_the_restatement_on_hand_made_sequences(name, host):
    """One object drifting; ties that the slot and the box index decide; coasting, death and a reused slot; a full table; frames without
    boxes; a reset in mid-sequence; boxes that are no detections; +BIG in a mean; a history that wraps (test_stream_tracks_host.py has
    the expected values written out)."""
    settings, frames = SEQUENCES[name]
    tr = _kernel_over(settings, frames, host, lambda n: n + 4)
    if name == 'coast':
        assert tr.seen == dict(match=1, death=1, birth=2, reuse=1, drop=0)
    if name == 'full':
        assert tr.seen['drop'] == 2


@pytest.mark.parametrize('sub', ['A', 'B'])
@pytest.mark.parametrize('max_tracks', [8, 128])
def test_stream_tracks_equals_the_restatement_on_random_sequences(max_tracks, sub):
    """30 frames; A: 80..100 boxes in a width of 128 (more than one wave of detections), B: TRACK_STAGE - 1, TRACK_STAGE and
    TRACK_STAGE + 1 boxes in turn (the staging boundary).  Half the rectangles are the host's.  The restatement must have seen every
    path, so that a lucky seed cannot hide one."""
    from vec_vad_amd.stream import TRACK_STAGE
    frames, width = random_sequence(100 + max_tracks, sub)
    sizes = {len(f[0]) for f in frames}
    assert (max(sizes) > 64 and width == 128) if sub == 'A' else (sorted(sizes) == [TRACK_STAGE - 1, TRACK_STAGE, TRACK_STAGE + 1])
    tr = _kernel_over(dict(RANDOM_SETTINGS, max_tracks=max_tracks), frames, 'half', lambda n: width)
    assert all(v >= 1 for v in tr.seen.values()), tr.seen


def test_stream_tracks_bad_arguments_return_without_a_launch():
    from vec_vad_amd import _lib
    l = _lib.lib()
    t = torch.zeros(256, dtype=torch.float64, device='cuda')
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    #       0  1  2  3  4  5  6  7  8  9 10 11 12 13 14 15 16 17 18   19 20 21 22 23
    good = [p, p, p, 2, p, 1, 4, p, 0, p, p, 4, 4, 0, 30, 5, 8, 3, BIG, p, p, p, p, st]
    bad = [(0, None), (1, None), (2, None), (7, None), (21, None), (22, None), (4, None), (9, None), (19, None), (20, None),
           (3, 0), (3, 1025), (14, 0), (14, 101), (15, -1), (16, 0), (16, 33), (17, 0), (5, -1), (6, -1), (8, -1), (11, -1), (12, -1)]
    for i, v in bad:
        args = list(good)
        args[i] = v
        assert l.vv_stream_tracks(*args) == 1, i                                    # VV_ERR_BAD_ARG
    args = list(good)
    args[11], args[12] = 65536, 32768                                               # h * w = 2^31
    assert l.vv_stream_tracks(*args) == 1
    torch.cuda.synchronize()
    assert not t.any()


# ---- 2. the scorer --------------------------------------------------------------------------------------------------------------------
TRACK_KEYS = dict(track_iou_percent=20, track_max_age=1, track_window=3, track_min_hits=2, stream_max_tracks=4)


def _against_the_restatement(tree, got, settings):
    """The track attributes of waited results against the restatement fed with the ``box_scores`` and ``boxes`` that ``wait()``
    returned, with a reset at the video boundary.  Returns the tracker."""
    from vad_datasets import frame_size
    from vec_vad_amd.scoring import box_rects
    gh, gw = frame_size['UCSDped2'][:2]
    tr = R.Tracker(settings['stream_max_tracks'], settings['track_window'], settings['track_iou_percent'], settings['track_max_age'],
                   settings['track_min_hits'])
    for f, (r, (score, box, kept)) in enumerate(got):
        want = tr.step(box[None, :], len(box), box_rects(r.boxes, gh, gw), reset=f == 0 or tree['fvi'][f] != tree['fvi'][f - 1])
        assert r.track_ids.dtype == np.int32 and r.track_ids.tolist() == want['ids'].tolist(), f
        assert r.track_hits.tolist() == want['hits'].tolist(), f
        assert r.track_scores.dtype == np.float64 and np.array_equal(_bits(r.track_scores), _bits(want['scores'])), f
        assert isinstance(r.track_score, float) and _bits(r.track_score) == _bits(want['score']), f
        assert r.tracks_dropped == want['dropped'], f
        assert r.tracks.dtype == np.int32 and r.tracks.shape[1] == 7 and np.array_equal(r.tracks, tr.tracks()), f
    return tr


@pytest.mark.parametrize('mode', ['one-round', 'rounds', 'motion'])
def test_scorer_tracks_equal_the_restatement_of_what_wait_returns(tree, net, monkeypatch, mode):
    """Given boxes in one round and in rounds of two, and motion boxes, over the tree's two videos: the scores are those of a scorer
    with tracks off, and the track attributes the restatement's."""
    monkeypatch.chdir(tree['root'])
    kw = dict(max_boxes=2 if mode == 'rounds' else 8, boxes='motion' if mode == 'motion' else 'given')
    c = dict(tree['c'], smooth_frames=KT, smooth_pixels=KS, **TRACK_KEYS)
    got = _run(tree, net, c=c, tracks=True, **kw)
    off = _run(tree, net, c=c, **kw)
    for f, ((r, (score, box, kept)), (o, (oscore, obox, okept))) in enumerate(zip(got, off)):
        assert _bits(score) == _bits(oscore) and np.array_equal(_bits(box), _bits(obox)) and kept.tolist() == okept.tolist(), f
        assert np.array_equal(r.boxes, o.boxes) and r.dropped == o.dropped, f
        assert r.mask is None and r.smooth_mask is None and r.picture is None      # tracks need no mask
        assert all(getattr(o, a) is None for a in ('track_ids', 'track_hits', 'track_scores', 'track_score', 'tracks_dropped', 'tracks')), f
    tr = _against_the_restatement(tree, got, TRACK_KEYS)
    assert tr.seen['birth'] >= 3 and tr.next_id > 3
    first = got[N_VIDEO[0]][0]                                                     # the second video starts with an empty table
    assert first.track_hits.max(initial=0) <= 1 and (first.tracks[:, 2] == 1).all()


def test_scorer_with_a_window_of_one_gives_the_frame_score(tree, net, monkeypatch):
    """window = 1, min_hits = 1 and a table that holds every box: the frame's track score is the frame score ``vv_stream_scores`` left,
    and a box's track score its box score wherever it has a track."""
    monkeypatch.chdir(tree['root'])
    keys = dict(TRACK_KEYS, track_window=1, track_min_hits=1, stream_max_tracks=16)
    got = _run(tree, net, c=dict(tree['c'], **keys), tracks=True, max_boxes=8)
    tracked = 0
    for f, (r, (score, box, kept)) in enumerate(got):
        assert r.tracks_dropped == 0 and _bits(r.track_score) == _bits(score), f
        on = r.track_ids > 0
        assert np.array_equal(_bits(r.track_scores[on]), _bits(box[on])) and (box[~on] == -BIG).all() and (r.track_scores[~on] == -BIG).all(), f
        tracked += int(on.sum())
    assert tracked >= 3
    _against_the_restatement(tree, got, keys)


def test_pixel_stages_are_unchanged_by_tracks(tree, net, monkeypatch):
    """The first video's frames set into the corner of 240x360 noise frames, masks, smoothing and picture on: the same masks and the
    same picture with tracks on and off, and the tracks the restatement's."""
    from vad_datasets import frame_size
    import train as T
    monkeypatch.chdir(tree['root'])
    gh, gw = frame_size['UCSDped2'][:2]
    rng = np.random.default_rng(9)
    frames = []
    for f in tree['frames'][:N_VIDEO[0]]:
        big = rng.integers(0, 256, (gh, gw, 3), dtype=np.uint8)
        big[:48, :72] = f
        frames.append(big)
    _keep_all(tree, 'config_tracks.cfg')
    c = dict(T.read_config('config_tracks.cfg'), smooth_frames=KT, smooth_pixels=KS, render_range=(-5.0, 20.0), **TRACK_KEYS)
    kw = dict(frames=frames, c=c, max_boxes=8, masks=True, smooth=True, render=True)
    on, off = _run(tree, net, (gh, gw, 3), tracks=True, **kw), _run(tree, net, (gh, gw, 3), **kw)
    for f, ((r, w), (o, ow)) in enumerate(zip(on, off)):
        assert _bits(w[0]) == _bits(ow[0]) and np.array_equal(_bits(w[1]), _bits(ow[1])) and w[2].tolist() == ow[2].tolist(), f
        assert np.array_equal(_bits(r.mask), _bits(o.mask)) and np.array_equal(_bits(r.smooth_mask), _bits(o.smooth_mask)), f
        assert _bits(r.smooth_score) == _bits(o.smooth_score) and np.array_equal(r.picture, o.picture), f
        assert o.track_ids is None and r.track_ids is not None
    assert sum(bool((r.mask > -BIG).any()) for r, _ in on) >= 2
    tr = _against_the_restatement(tree, on, TRACK_KEYS)
    assert tr.seen['birth'] >= 2


# ---- 3. the script --------------------------------------------------------------------------------------------------------------------
def _files(root):
    return {p: open(p, 'rb').read() for p in sorted(glob.glob(os.path.join(root, '**', '*'), recursive=True)) if os.path.isfile(p)}


def _Npz(data):
    import io
    return np.load(io.BytesIO(data))


def test_stream_main_with_the_key_on_writes_the_track_scores_and_the_same_files(tree, net, monkeypatch, capsys):
    import stream as STREAM
    import train as T
    monkeypatch.chdir(tree['root'])
    saved = open('config.cfg').read()
    name = 'results/UCSDped2/stream_scores_track_obj_det_with_motion_SelfComplete.npy'
    assert saved.count('stream_tracks = off\n') == 1
    try:
        A = STREAM.main('config.cfg', flownet2=net)
        before = _files('results')
        assert not os.path.exists(name) and not glob.glob('results/UCSDped2/*track*')
        open('config.cfg', 'w').write(saved.replace('stream_tracks = off\n', 'stream_tracks = on\n'))
        c = T.read_config('config.cfg')
        assert c['stream_tracks'] is True
        capsys.readouterr()
        B = STREAM.main('config.cfg', flownet2=net)
        out = capsys.readouterr().out
    finally:
        open('config.cfg', 'w').write(saved)
    after = _files('results')
    assert np.array_equal(_bits(A), _bits(B)) and (A > -BIG).sum() >= 3
    roc = 'results/UCSDped2/raw2flow_obj_det_with_motion_SelfComplete_stream_track_results.npz'
    assert sorted(set(after) - set(before)) == sorted([name, roc])
    for p in before:                                                               # every file written without the key is the same
        if p.endswith('.npz'):                                                     # ... a zip archive carries the time it was written
            a, b = np.load(p), _Npz(before[p])
            assert sorted(a.files) == sorted(b.files) and all(a[k].tobytes() == b[k].tobytes() for k in a.files), p
        else:
            assert after[p] == before[p], p
    S = np.load(name)
    api = np.array([r.track_score for r, _ in _run(tree, net, c=c, max_boxes=c['stream_max_boxes'])])
    assert S.dtype == np.float64 and S.shape == (sum(N_VIDEO),) and np.array_equal(_bits(S), _bits(api))
    auc = float(np.load(roc)['roc_auc'])
    assert "Frame-level AUC of the stream's tracks is {}".format(auc) in out.splitlines()
