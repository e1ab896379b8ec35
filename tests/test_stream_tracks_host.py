"""Host side of the tracks of a stream (vec_vad_amd/stream.py: tracks): the restatement that tests/test_gpu_stream_tracks.py holds the
kernel against, on hand-made sequences with the expected ids and means written out; the seeds of that file's random sequences, which
must exercise a match, a death, a birth into a reused slot and a drop; the keys, their defaults and their refusals; the schedule's
``reset``.  No GPU."""
import os

import numpy as np
import pytest

import stream_tracks_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = R.BIG
H, W = 45, 70
STAGE = 256                # vec_vad_amd.stream.TRACK_STAGE, pinned below


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


# ---- hand-made sequences -------------------------------------------------------------------------------------------------------------
# name -> (Tracker settings, frames); a frame is (boxes [(x1, y1, x2, y2)], score rows [[..], ..], reset).  Frames are 45 x 70.
A, B, C = (5, 5, 25, 20), (40, 5, 60, 20), (20, 25, 45, 44)          # three objects far from each other
OBJ = (20, 10, 40, 30)
SEQUENCES = {
    # one object drifting 2 px right and 1 px down per frame; its larger score sits in row 0 or row 1 in turn
    'drift': (dict(max_tracks=4), [([(10 + 2 * f, 10 + f, 30 + 2 * f, 30 + f)], [[f + 1.0, -BIG][f % 2:][:1], [-BIG, f + 1.0][f % 2:][:1]], f == 0)
                                   for f in range(5)]),
    # frame 1: two boxes overlap track 1 by 300 of a union of 500 each -> the lower box takes it; frame 2: one box overlaps the
    # tracks in slots 0 and 1 by the same -> the lower slot takes it
    'tie': (dict(max_tracks=4, min_hits=1), [([OBJ], [[1.0]], True), ([(25, 10, 45, 30), (15, 10, 35, 30)], [[2.0, 3.0]], False),
                                             ([OBJ], [[5.0]], False)]),
    # max_age 2: two frames without a box are coasted through, three are not; the slot is taken by the next birth
    'coast': (dict(max_tracks=3, max_age=2, min_hits=2),
              [([OBJ], [[1.0]], True), ([], [[]], False), ([], [[]], False), ([OBJ], [[3.0]], False), ([], [[]], False), ([], [[]], False),
               ([], [[]], False), ([OBJ], [[7.0]], False)]),
    # a table of two slots and three objects
    'full': (dict(max_tracks=2, min_hits=1), [([A, B, C], [[1.0, 2.0, 9.0]], True), ([A, B, C], [[3.0, 2.0, 9.0]], False)]),
    # a reset in mid-sequence: the table is empty, the ids go on
    'reset': (dict(max_tracks=4, min_hits=2), [([A, B], [[1.0, 2.0]], True), ([A, B], [[3.0, 4.0]], False), ([A, B], [[5.0, 6.0]], True),
                                               ([A, B], [[7.0, 8.0]], False)]),
    # a box that scored -BIG, a box of no pixels and a box of no score row at all next to a detection
    'nondet': (dict(max_tracks=4, min_hits=1), [([A, (10, 10, 10, 30), B], [[-BIG, 4.0, 2.0], [-BIG, 1.0, -BIG]], True),
                                                ([A, (10, 10, 10, 30), B], [[-BIG, 4.0, 6.0], [-BIG, 1.0, -BIG]], False),
                                                ([A, B], np.zeros((0, 2)), False)]),
    # +BIG (a block without a model) floods the mean, as it floods smooth_masks
    'big': (dict(max_tracks=2, min_hits=1), [([OBJ], [[1.0]], True), ([OBJ], [[BIG]], False), ([OBJ], [[2.0]], False)]),
    # a history of three scores wraps twice over seven matches
    'wrap': (dict(max_tracks=2, window=3, min_hits=1), [([OBJ], [[f + 1.0]], f == 0) for f in range(7)]),
}
# per frame: ids, hits, track scores, the frame's track score, live, dropped, next_id
EXPECTED = {
    'drift': [([1], [1], [1.0], -BIG, 1, 0, 2), ([1], [2], [1.5], -BIG, 1, 0, 2), ([1], [3], [2.0], 2.0, 1, 0, 2),
              ([1], [4], [2.5], 2.5, 1, 0, 2), ([1], [5], [3.0], 3.0, 1, 0, 2)],
    'tie': [([1], [1], [1.0], 1.0, 1, 0, 2), ([1, 2], [2, 1], [1.5, 3.0], 3.0, 2, 0, 3), ([1], [3], [8.0 / 3.0], 8.0 / 3.0, 2, 0, 3)],
    'coast': [([1], [1], [1.0], -BIG, 1, 0, 2), ([], [], [], -BIG, 1, 0, 2), ([], [], [], -BIG, 1, 0, 2), ([1], [2], [2.0], 2.0, 1, 0, 2),
              ([], [], [], -BIG, 1, 0, 2), ([], [], [], -BIG, 1, 0, 2), ([], [], [], -BIG, 0, 0, 2), ([2], [1], [7.0], -BIG, 1, 0, 3)],
    'full': [([1, 2, 0], [1, 1, 0], [1.0, 2.0, -BIG], 2.0, 2, 1, 3), ([1, 2, 0], [2, 2, 0], [2.0, 2.0, -BIG], 2.0, 2, 1, 3)],
    'reset': [([1, 2], [1, 1], [1.0, 2.0], -BIG, 2, 0, 3), ([1, 2], [2, 2], [2.0, 3.0], 3.0, 2, 0, 3),
              ([3, 4], [1, 1], [5.0, 6.0], -BIG, 2, 0, 5), ([3, 4], [2, 2], [6.0, 7.0], 7.0, 2, 0, 5)],
    'nondet': [([0, 0, 1], [0, 0, 1], [-BIG, -BIG, 2.0], 2.0, 1, 0, 2), ([0, 0, 1], [0, 0, 2], [-BIG, -BIG, 4.0], 4.0, 1, 0, 2),
               ([0, 0], [0, 0], [-BIG, -BIG], -BIG, 1, 0, 2)],
    'big': [([1], [1], [1.0], 1.0, 1, 0, 2), ([1], [2], [(1.0 + BIG) / 2.0], (1.0 + BIG) / 2.0, 1, 0, 2),
            ([1], [3], [(1.0 + BIG + 2.0) / 3.0], (1.0 + BIG + 2.0) / 3.0, 1, 0, 2)],
    'wrap': [([1], [f + 1], [m], m, 1, 0, 2) for f, m in enumerate([1.0, 1.5, 2.0, 3.0, 4.0, 5.0, 6.0])],
}


def frame_arrays(frame):
    """A frame of a sequence as ``(boxes int32 [n,4], rows float64 [R,n], reset)``."""
    boxes, rows, reset = frame
    boxes = np.asarray(boxes, np.int32).reshape(-1, 4)
    rows = np.asarray(rows, np.float64)
    return boxes, rows.reshape(rows.shape[0] if rows.ndim == 2 else 0, len(boxes)), bool(reset)


@pytest.mark.parametrize('name', sorted(SEQUENCES))
def test_restatement_on_hand_made_sequences(name):
    settings, frames = SEQUENCES[name]
    tr = R.Tracker(**settings)
    assert len(frames) == len(EXPECTED[name])
    for f, (frame, want) in enumerate(zip(frames, EXPECTED[name])):
        boxes, rows, reset = frame_arrays(frame)
        got = tr.step(rows, len(boxes), R.resolve(boxes, H, W), reset)
        ids, hits, scores, score, live, dropped, next_id = want
        assert got['ids'].tolist() == ids and got['hits'].tolist() == hits, (name, f)
        assert np.array_equal(_bits(got['scores']), _bits(scores)), (name, f, got['scores'])
        assert _bits(got['score']) == _bits(score) and (got['live'], got['dropped'], got['next_id']) == (live, dropped, next_id), (name, f)
        assert len(tr.tracks()) == live and (tr.meta[tr.meta[:, 0] == 0] == 0).all() and (tr.hist[tr.meta[:, 0] == 0] == 0).all()
    if name == 'tie':
        assert tr.tracks().tolist() == [[1, 0, 3, 10, 30, 20, 40], [2, 1, 1, 10, 30, 15, 35]]
    if name == 'coast':
        assert tr.tracks().tolist() == [[2, 0, 1, 10, 30, 20, 40]] and tr.seen == dict(match=1, death=1, birth=2, reuse=1, drop=0)
    if name == 'wrap':
        assert tr.hist[0].tolist() == [7.0, 5.0, 6.0]
    if name == 'full':
        assert tr.seen['drop'] == 2


def test_pair_order_is_exact_where_floating_point_is_not():
    """Two IoUs that differ in the 18th digit: the cross products of the integers tell them apart, their float64 quotients do not.
    Equal IoUs: the lower slot, then the lower box."""
    a, b = (10 ** 17, 3 * 10 ** 17 + 1, 0, 0), (10 ** 17, 3 * 10 ** 17, 1, 1)
    assert a[0] / a[1] == b[0] / b[1] and R._pair_order(a, b) == 1 and R._pair_order(b, a) == -1
    assert R._pair_order((2, 4, 1, 0), (1, 2, 0, 5)) == 1 and R._pair_order((1, 2, 0, 5), (2, 4, 0, 6)) == -1
    assert R._pair_order((1, 2, 3, 4), (1, 2, 3, 4)) == 0


# ---- random sequences ----------------------------------------------------------------------------------------------------------------
RANDOM_SETTINGS = dict(window=4, iou_pct=30, max_age=3, min_hits=2)


def random_sequence(seed, sub, frames=30):
    """Seeded frames ``(boxes int32 [n,4], rows float64 [2,n], reset)`` and their table width.  Objects of 5..12 pixels jitter by up to
    2 px a frame, leave with probability 0.2 and are replaced or joined by new ones until the frame has its number of boxes: 80..100
    in a width of 128 (``A``, with a reset at frame 15), or ``STAGE - 1``, ``STAGE`` and ``STAGE + 1`` for three frames each in turn
    (``B``).  8% of the boxes score -BIG in both rows for a frame (the track coasts) -- 95% in frames 19..23, so that tracks die and
    their slots are taken again --, 1% +BIG; a box may reach over the frame's edge."""
    rng = np.random.default_rng(seed)
    width = 128 if sub == 'A' else STAGE + 8
    objs, out = [], []
    for f in range(frames):
        n = int(rng.integers(80, 101)) if sub == 'A' else STAGE - 1 + (f // 3) % 3
        objs = [(min(max(x + int(rng.integers(-2, 3)), -2), W - 3), min(max(y + int(rng.integers(-2, 3)), -2), H - 3), w, h)
                for x, y, w, h in objs if rng.random() >= 0.2]
        while len(objs) > n:
            objs.pop(int(rng.integers(len(objs))))
        while len(objs) < n:
            objs.insert(int(rng.integers(len(objs) + 1)), (int(rng.integers(-2, W - 3)), int(rng.integers(-2, H - 3)),
                                                           int(rng.integers(5, 13)), int(rng.integers(5, 13))))
        boxes = np.array([[x, y, x + w, y + h] for x, y, w, h in objs], np.int32).reshape(-1, 4)
        rows = rng.standard_normal((2, n)) * 3
        rows[1, rng.random(n) < 0.5] = -BIG
        rows[:, rng.random(n) < (0.95 if 19 <= f <= 23 else 0.08)] = -BIG
        rows[0, rng.random(n) < 0.01] = BIG
        out.append((boxes, rows, f == 0 or (sub == 'A' and f == 15)))
    return out, width


def run_restatement(settings, frames):
    """The restatement over a sequence: per frame its outputs and a copy of the state behind it; and the tracker."""
    tr = R.Tracker(**settings)
    steps = []
    for frame in frames:
        boxes, rows, reset = frame_arrays(frame)
        got = tr.step(rows, len(boxes), R.resolve(boxes, H, W), reset)
        steps.append((got, tr.meta.copy(), tr.hist.copy()))
    return steps, tr


@pytest.mark.parametrize('sub', ['A', 'B'])
@pytest.mark.parametrize('max_tracks', [8, 128])
def test_the_seeds_of_the_random_sequences_exercise_every_path(max_tracks, sub):
    frames, width = random_sequence(100 + max_tracks, sub)
    steps, tr = run_restatement(dict(RANDOM_SETTINGS, max_tracks=max_tracks), frames)
    assert all(v >= 1 for v in tr.seen.values()), tr.seen
    assert max(len(f[0]) for f in frames) <= width
    ids = np.concatenate([g['ids'] for g, _, _ in steps])
    assert (ids > 0).sum() >= 100 and tr.next_id == steps[-1][0]['next_id'] > max_tracks
    if sub == 'A':
        assert max(len(f[0]) for f in frames) > 64                     # more than one wave of detections
        assert steps[15][0]['hits'].max() == 1 and steps[15][0]['ids'].min(initial=1 << 30, where=steps[15][0]['ids'] > 0) > steps[14][0]['ids'].max()
    else:
        assert sorted({len(f[0]) for f in frames}) == [STAGE - 1, STAGE, STAGE + 1]


def test_with_a_window_of_one_the_track_score_is_the_box_score():
    """window = 1, min_hits = 1 and a table that holds every box: the track score of a box is its own score, and the frame's track
    score the largest score of a detection -- the frame score ``vv_stream_scores`` leaves."""
    frames, _ = random_sequence(5, 'A', frames=8)
    tr = R.Tracker(128, window=1, iou_pct=30, max_age=0, min_hits=1)
    for boxes, rows, reset in frames:
        rects = R.resolve(boxes, H, W)
        got = tr.step(rows, len(boxes), rects, reset)
        s = rows.max(axis=0)
        det = (rects[:, 1] > rects[:, 0]) & (rects[:, 3] > rects[:, 2]) & (s > -BIG)
        assert got['dropped'] == 0 and ((got['ids'] > 0) == det).all() and det.any() and not det.all()
        assert np.array_equal(_bits(got['scores'][det]), _bits(s[det])) and (got['scores'][~det] == -BIG).all()
        assert got['score'] == s[det].max()


# ---- keys, refusals, schedule ----------------------------------------------------------------------------------------------------------
def test_the_keys_in_the_stock_file_their_defaults_and_the_stage():
    import train as T
    from vec_vad_amd.stream import TRACK_STAGE, check_track_settings
    assert TRACK_STAGE == STAGE
    text = open(os.path.join(ROOT, 'config.cfg')).read()
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    want = dict(stream_tracks=False, track_iou_percent=30, track_max_age=5, track_window=8, track_min_hits=3, stream_max_tracks=128)
    for key, v in want.items():
        assert c['cp'].has_option('mi355x', key) and c[key] == v and type(c[key]) is type(v)
    assert text.count('\nstream_tracks = off\n') == 1 and 'untuned' in text
    assert check_track_settings(c, None) == (False, 30, 5, 8, 3, 128) and check_track_settings(c, True) == (True, 30, 5, 8, 3, 128)
    assert check_track_settings(dict(c, stream_tracks=True), None)[0] is True and check_track_settings({}, None) == (False, 30, 5, 8, 3, 128)


def test_a_config_without_the_keys_reads_the_defaults(tmp_path):
    import train as T
    text = open(os.path.join(ROOT, 'config.cfg')).read()
    keys = ('stream_tracks', 'track_iou_percent', 'track_max_age', 'track_window', 'track_min_hits', 'stream_max_tracks')
    p = tmp_path / 'config.cfg'
    p.write_text('\n'.join(l for l in text.splitlines() if not l.startswith(keys)) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'stream_tracks')
    assert [c[k] for k in keys] == [False, 30, 5, 8, 3, 128]
    p.write_text(text.replace('stream_tracks = off', 'stream_tracks = on').replace('track_window = 8', 'track_window = 33'))
    with pytest.raises(ValueError, match='track_window'):
        T.read_config(str(p))


@pytest.mark.parametrize('key,bad', [('track_iou_percent', 0), ('track_iou_percent', 101), ('track_max_age', -1), ('track_window', 0),
                                     ('track_window', 33), ('track_min_hits', 0), ('stream_max_tracks', 0), ('stream_max_tracks', 1025),
                                     ('track_window', 2.5), ('stream_max_tracks', True), ('track_min_hits', '3')])
def test_bad_settings_are_refused_in_one_line_before_the_gpu_is_touched(monkeypatch, key, bad):
    import torch
    from vec_vad_amd.stream import StreamScorer, check_track_settings

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    for name in ('set_device', 'current_device', 'is_available', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)
    import train as T
    c = dict(T.read_config(os.path.join(ROOT, 'config.cfg')), **{key: bad})
    for tracks in (True, None):
        with pytest.raises(ValueError, match=key) as e:
            check_track_settings(c, tracks)
        assert '\n' not in str(e.value)
    with pytest.raises(ValueError, match=key):
        StreamScorer(c, None, None, None, (240, 360, 3), flownet2=object(), tracks=True)


def test_the_schedule_says_which_issue_is_the_first_of_its_video():
    from vec_vad_amd.stream import RingSchedule
    s = RingSchedule(4, 0)
    for n in (3, 2, 4):
        got = [s.push()[1] for _ in range(n)][1:] + [s.end_video()]
        assert [i['frame'] for i in got] == list(range(n)) and [i['reset'] for i in got] == [True] + [False] * (n - 1)
