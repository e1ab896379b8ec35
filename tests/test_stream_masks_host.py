"""Host side of the pixel-level stages of a stream (vec_vad_amd/stream.py: masks / smooth / render): the restatement that
tests/test_gpu_stream_masks.py holds the kernels against is itself held against the centred filter of tests/smooth_restatement.py and
against ``scoring.box_rects``; the schedule's mask-ring fields; the keys; the refusals.  No GPU."""
import os

import numpy as np
import pytest

import smooth_restatement as SR
import stream_masks_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = R.BIG


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _masks(kind, F=7, h=11, w=13, seed=0):
    """A video of painted masks: rectangles of random values (``random``) or of multiples of 1/8 (``dyadic``: every sum is exact) over a
    background of -BIG, one frame with nothing painted."""
    rng = np.random.default_rng(seed)
    m = np.full((F, h, w), -BIG)
    for f in range(F):
        if f == 3:
            continue
        for _ in range(3):
            y0, x0 = rng.integers(0, h - 2), rng.integers(0, w - 2)
            y1, x1 = rng.integers(y0 + 1, h + 1), rng.integers(x0 + 1, w + 1)
            v = rng.integers(-40, 40) / 8.0 if kind == 'dyadic' else rng.standard_normal() * 3
            m[f, y0:y1, x0:x1] = np.maximum(m[f, y0:y1, x0:x1], v)
    return m


@pytest.mark.parametrize('kind', ['random', 'dyadic'])
@pytest.mark.parametrize('ks', [1, 3, 9])
@pytest.mark.parametrize('kt', [1, 2, 5])
def test_trailing_is_the_centred_filter_of_window_2kt_minus_1_read_at_the_last_frame(kt, ks, kind):
    m = _masks(kind)
    got = R.trailing(m, kt, ks)
    assert (got[3] == -BIG).all() and ((got == -BIG) == (m == -BIG)).all()            # the support is preserved
    for t in range(len(m)):
        want = SR.smooth(m[:t + 1], np.zeros(t + 1, np.int64), 2 * kt - 1, ks)[0][t]
        assert np.array_equal(_bits(got[t]), _bits(want)), (t, kt, ks)
        if kind == 'dyadic':
            assert np.array_equal(got[t], SR.brute(m[:t + 1], np.zeros(t + 1, np.int64), 2 * kt - 1, ks)[t]), (t, kt, ks)
    if kt == 1 and ks == 1:
        assert np.array_equal(got, m)


def test_resolve_equals_box_rects_on_integer_boxes():
    from vec_vad_amd.scoring import box_rects
    h, w = 45, 70
    rng = np.random.default_rng(1)
    boxes = rng.integers(-90, 160, (400, 4))
    boxes = np.concatenate([boxes, [[0, 0, w, h], [-3, 5, 40, 40], [5, -3, 40, 40], [60, 30, 75, 50], [10, 10, 10, 30], [30, 30, 10, 10],
                                    [-w, -h, w, h], [-w - 1, -h - 1, -1, -1], [w, h, w + 5, h + 5], [0, 0, -1, -1]]])
    got, want = R.resolve(boxes, h, w), box_rects(boxes.astype(np.float64), h, w)
    assert got.dtype == want.dtype == np.int32 and np.array_equal(got, want)
    assert (got >= 0).all() and (got[:, :2] <= h).all() and (got[:, 2:] <= w).all()
    assert got[-10].tolist() == [0, h, 0, w] and got[-9].tolist() == [5, 40, w - 3, 40]      # a negative x1 wraps: nothing painted
    assert (got[:, 1] <= got[:, 0]).any() and (got[:, 1] > got[:, 0]).any()


def test_paint_restatement_on_hand_made_boxes():
    rows = np.array([[1.0, -BIG, 5.0, np.nan], [0.5, 2.0, -BIG, np.inf]])
    rects = np.array([[0, 2, 0, 3], [1, 3, 2, 4], [2, 2, 0, 4], [0, 4, 0, 4]], np.int32)
    mask, box_max = R.paint(rows, 3, rects, 4, 4)
    assert box_max.tolist() == [1.0, 2.0, 5.0]
    assert mask.tolist() == [[1.0, 1.0, 1.0, -BIG], [1.0, 1.0, 2.0, 2.0], [-BIG, -BIG, 2.0, 2.0], [-BIG] * 4]      # box 2 is empty
    mask, box_max = R.paint(rows[:0], 3, rects, 4, 4)
    assert (mask == -BIG).all() and box_max.tolist() == [-BIG] * 3
    assert (R.paint(rows, 0, rects, 4, 4)[0] == -BIG).all()


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
def test_mask_ring_fields_across_a_video_boundary_and_for_a_short_video():
    from vec_vad_amd.stream import RingSchedule
    s = RingSchedule(4, 0, mask_frames=3)
    assert s.K == 3
    issues = []
    for n in (5, 2, 4):                                   # the second video is shorter than the window
        got = [s.push()[1] for _ in range(n)][1:] + [s.end_video()]
        assert [i['frame'] for i in got] == list(range(n))
        issues.append(got)
    for got in issues:
        for t, i in enumerate(got):
            assert i['mask_slot'] == t % 3
            assert i['mask_frames'] == list(range(max(0, t - 2), t + 1))      # never a frame of the video before
            assert i['mask_slots'] == [f % 3 for f in i['mask_frames']] and i['mask_slots'][-1] == i['mask_slot']
    assert issues[0][4]['mask_slots'] == [2, 0, 1]        # the ring's slot order wraps
    assert issues[1][0]['mask_slots'] == [0] and issues[1][1]['mask_slots'] == [0, 1]
    # without smoothing: one slot
    s = RingSchedule(4, 0)
    s.push(), s.push()
    i = s.end_video()
    assert (i['mask_slot'], i['mask_frames'], i['mask_slots']) == (0, [1], [0])


# ---- keys and refusals ---------------------------------------------------------------------------------------------------------------
def test_the_three_keys_in_the_stock_file_and_their_defaults(tmp_path):
    import train as T
    text = open(os.path.join(ROOT, 'config.cfg')).read()
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for key in ('stream_masks', 'stream_smooth', 'stream_render'):
        assert c['cp'].has_option('mi355x', key) and c[key] is False and text.count('\n%s = off\n' % key) == 1
    p = tmp_path / 'config.cfg'
    p.write_text(text.replace('stream_smooth = off', 'stream_smooth = on'))
    c = T.read_config(str(p))
    assert c['stream_smooth'] is True and c['stream_masks'] is False
    p.write_text('\n'.join(l for l in text.splitlines() if not l.startswith(('stream_masks', 'stream_smooth', 'stream_render'))) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'stream_masks') and not (c['stream_masks'] or c['stream_smooth'] or c['stream_render'])


def test_refusals_come_before_the_gpu_is_touched(tmp_path, monkeypatch):
    import torch
    import foreground as FG
    import stream as STREAM
    import train as T
    from vec_vad_amd.stream import StreamScorer

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    for name in ('set_device', 'current_device', 'is_available', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(FG, 'load_bboxes', touched)
    text = open(os.path.join(ROOT, 'config.cfg')).read()
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['render_range'] == 'auto' and c['dataset_name'] == 'UCSDped2'
    make = lambda c, shape=(240, 360, 3), **kw: StreamScorer(c, None, None, None, shape, flownet2=object(), **kw)
    cases = [(dict(c), dict(render=True), 'render_range'),                                                  # auto needs the whole run
             (dict(c, render_range=(-5.0, 20.0), render_source='smooth'), dict(render=True), 'stream_smooth'),
             (dict(c, render_range=(-5.0, 20.0), stream_render=True), dict(shape=(48, 72, 3)), '48x72 frames'),
             (dict(c, smooth_frames=34), dict(smooth=True), 'smooth_frames'),
             (dict(c, smooth_pixels=4), dict(smooth=True), 'smooth_pixels')]
    for cc, kw, match in cases:
        with pytest.raises(ValueError, match=match) as e:
            make(cc, **kw)
        assert '\n' not in str(e.value)
    # the script, from the keys alone
    monkeypatch.chdir(tmp_path)
    open('config.cfg', 'w').write(text.replace('stream_render = off', 'stream_render = on'))
    with pytest.raises(ValueError, match='render_range'):
        STREAM.main('config.cfg')
    open('config.cfg', 'w').write(text.replace('stream_render = off', 'stream_render = on').replace(
        'render_range = auto', 'render_range = -5,20').replace('render_source = score', 'render_source = smooth'))
    with pytest.raises(ValueError, match='stream_smooth'):
        STREAM.main('config.cfg')
    assert os.listdir('.') == ['config.cfg']
