"""Host side of the stream scorer that finds its own motion boxes (``StreamScorer(boxes='motion')``, vec_vad_amd/stream.py): the
motion window of the ring schedule against ``vad_datasets.context_range``, the ``[mi355x] stream_boxes`` key, the numpy restatement of
``vv_stream_boxes`` on hand-made boxes, and -- through tests/motion_boxes_restatement.py -- that the synthetic videos of
tests/test_gpu_stream_boxes.py contain what those tests rely on.  No GPU."""
import os

import numpy as np
import pytest

import stream_boxes_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfn', [0, 4])
@pytest.mark.parametrize('lengths', [(2, 3, 5), (5, 3, 2), (3, 5, 2), (5, 2), (2, 2)])
def test_motion_window_matches_context_range(lengths, cfn):
    """Videos of 2, 3 and 5 frames back to back as one split: every issue's motion window is ``context_range(i, 'hard', 1)``, the
    first and the last frame of the split included, and its slots name those frames in a model of the ring (slot -> frame)."""
    from vad_datasets import context_range
    from vec_vad_amd.stream import RingSchedule
    fvi = [v + 1 for v, n in enumerate(lengths) for _ in range(n)]
    sched = RingSchedule(cfn, 0, motion=True)
    ring, seen, s0 = {}, [], 0

    def check(issue):
        g = s0 + issue['frame']
        want = context_range(g, 'hard', 1, len(fvi), fvi)
        assert [s0 + f for f in issue['motion_frames']] == want
        assert [ring[s] for s in issue['motion_slots']] == want
        assert [ring[s] for s in issue['raw_slots']] == [s0 + f for f in issue['raw_frames']]      # the raw window survives a larger ring
        seen.append(g)

    for n in lengths:
        for k in range(n):
            slot, issue = sched.push()
            ring[slot] = s0 + k
            if issue is not None:
                check(issue)
        check(sched.end_video())
        s0 += n
    assert seen == list(range(len(fvi)))
    assert context_range(0, 'hard', 1, len(fvi), fvi) == [0, 0, 1] and context_range(len(fvi) - 1, 'hard', 1, len(fvi), fvi)[1:] == \
        [len(fvi) - 1] * 2


def test_ring_frames_is_unchanged_and_the_motion_ring_holds_three():
    from vec_vad_amd.stream import RingSchedule, motion_ring_frames, ring_frames
    assert [ring_frames(k) for k in (0, 1, 4)] == [2, 3, 6]
    assert [motion_ring_frames(k) for k in (0, 1, 4)] == [3, 3, 6]
    assert RingSchedule(0, 0).R == 2 and RingSchedule(0, 0, motion=True).R == 3
    assert RingSchedule(4, 4).R == RingSchedule(4, 4, motion=True).R == 6
    issue = RingSchedule(4, 0)
    issue.push()
    assert set(issue.push()[1]) >= {'motion_frames', 'motion_slots', 'raw_slots', 'pair_slots'}      # the fields are there in either mode


# ---- the key ---------------------------------------------------------------------------------------------------------------------------
def test_stream_boxes_in_the_stock_file_and_its_default(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'stream_boxes') and c['stream_boxes'] == 'given'
    assert _config_text().count('\nstream_boxes = given\n') == 1
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('\nstream_boxes = given\n', '\nstream_boxes = Motion \n'))
    assert T.read_config(str(p))['stream_boxes'] == 'motion'
    # a file from before the key still parses, with the default
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith('stream_boxes')) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'stream_boxes') and c['stream_boxes'] == 'given'


@pytest.mark.parametrize('bad', ['detector', 'true', '1', ''])
def test_bad_stream_boxes_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch, bad):
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
    monkeypatch.chdir(tmp_path)
    open('config.cfg', 'w').write(_config_text().replace('\nstream_boxes = given\n', '\nstream_boxes = ' + bad + '\n'))
    for call in (lambda: T.read_config('config.cfg'), lambda: STREAM.main('config.cfg'), lambda: StreamScorer.from_config('config.cfg')):
        with pytest.raises(ValueError, match='stream_boxes') as e:
            call()
        assert '\n' not in str(e.value)
    # the constructor's own argument, on a good configuration; and a frame larger than the nominal one in motion mode
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for v in ('detector', 1, True):
        with pytest.raises(ValueError, match='stream_boxes'):
            StreamScorer(c, None, None, None, (48, 72, 1), flownet2=object(), boxes=v)
    with pytest.raises(ValueError, match='larger than the nominal') as e:
        StreamScorer(c, None, None, None, (241, 360, 1), flownet2=object(), boxes='motion')
    assert '\n' not in str(e.value)
    assert os.listdir('.') == ['config.cfg']               # nothing written either


def test_stream_main_refuses_motion_boxes_under_another_foreground_mode(tmp_path, monkeypatch):
    """``stream_boxes = motion`` finds the boxes of mode obj_det_with_motion; the artifacts are loaded by the configured mode, so
    another mode is refused in one line before anything is loaded or the GPU is touched."""
    import torch
    import foreground as FG
    import stream as STREAM

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    for name in ('set_device', 'current_device', 'is_available', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)
    monkeypatch.setattr(FG, '_datasets', touched)
    monkeypatch.chdir(tmp_path)
    cfg = _config_text().replace('\nstream_boxes = given\n', '\nstream_boxes = motion\n')
    assert 'foreground_extraction_mode = obj_det_with_motion' in cfg
    open('config.cfg', 'w').write(cfg.replace('foreground_extraction_mode = obj_det_with_motion', 'foreground_extraction_mode = simple_patch'))
    with pytest.raises(ValueError, match='obj_det_with_motion') as e:
        STREAM.main('config.cfg')
    assert '\n' not in str(e.value) and os.listdir('.') == ['config.cfg']


# ---- the restatement on hand-made boxes ------------------------------------------------------------------------------------------------
GRID = dict(H=48, W=72, grid_h=96, grid_w=144, hb=2, wb=3)      # 48 x 48 cells


def test_restatement_on_hand_made_boxes():
    boxes = np.array([[10, 10, 30, 30],       # well inside cell (0, 0)
                      [40, 4, 70, 20],        # centre x = 55 in column 1, left corner probe (40 + 55) / 2 = 47.5 in column 0
                      [24, 8, 72, 48],        # touches the right and bottom frame edges; centre (28, 48): x exactly on the boundary
                      [0, 0, 4, 4]], np.int64)
    n, dropped, crops, masks, out = R.stream_boxes(4, boxes, 0, 8, block_mode=9, **GRID)
    assert (n, dropped) == (4, 0)
    assert crops[:4].tolist() == boxes.tolist() and out[:4].tolist() == boxes.tolist() and not crops[4:].any() and not out[4:].any()
    assert masks[:, 0].tolist() == [1, 0, 0, 0, 0, 0]
    assert masks[:, 1].tolist() == [1, 1, 0, 0, 0, 0]
    # box 2: centre (cy, cx) = (28, 48) -> column int(48 / 48) = 1; the left probes ((24 + 48) / 2 = 36) column 0; the bottom probes
    # ((48 + 28) / 2 = 38) stay in row 0
    assert masks[:, 2].tolist() == [1, 1, 0, 0, 0, 0]
    assert masks[:, 4:].sum() == 0
    # mode 1 sees the centre alone; mode 5 adds the edge mid-points but not the corners
    assert R.stream_boxes(4, boxes, 0, 8, block_mode=1, **GRID)[3][:, 1].tolist() == [0, 1, 0, 0, 0, 0]
    assert R.stream_boxes(4, boxes, 0, 8, block_mode=5, **GRID)[3][:, 1].tolist() == [1, 1, 0, 0, 0, 0]
    assert R.stream_boxes(4, boxes, 0, 8, block_mode=5, **GRID)[3][:, 0].tolist() == [1, 0, 0, 0, 0, 0]


def test_restatement_capacity_poison_and_appearance_slots():
    boxes = np.array([[10, 10, 30, 30], [40, 4, 70, 20], [24, 8, 72, 48], [0, 0, 4, 4], [1, 1, 9, 9], [2, 2, 8, 8]], np.int64)
    poison_c, poison_m, poison_o = np.full((8, 4), -77, np.int32), np.full((6, 8), 9, np.uint8), np.full((8, 4), -55, np.int32)
    # 3 appearance slots, 5 free: 7 found, 6 rows there (mcap), 5 fit
    n, dropped, crops, masks, out = R.stream_boxes(7, boxes, 3, 8, block_mode=9, crops=poison_c, masks=poison_m, boxes_out=poison_o, **GRID)
    assert (n, dropped) == (8, 2)
    assert (crops[:3] == -77).all() and (out[:3] == -55).all() and (masks[:, :3] == 9).all()      # the appearance slots are not touched
    assert out[3:].tolist() == boxes[:5].tolist() and crops[3:].tolist() == boxes[:5].tolist()
    assert masks[:, 3:].max() == 1 and masks[:, 3].tolist() == [1, 0, 0, 0, 0, 0]
    # no box at all: n = n_ap, the motion columns read 0, crops and boxes_out keep what they held
    n, dropped, crops, masks, out = R.stream_boxes(0, boxes, 3, 8, block_mode=9, crops=poison_c, masks=poison_m, boxes_out=poison_o, **GRID)
    assert (n, dropped) == (3, 0) and (crops == -77).all() and (out == -55).all()
    assert (masks[:, :3] == 9).all() and not masks[:, 3:].any()
    # a full table: every found box is dropped
    assert R.stream_boxes(2, boxes, 8, 8, block_mode=9, **GRID)[:2] == (8, 2)
    # a box that paints no pixel of the nominal mask gets no bit (x1 = x2 clipped at the mask edge cannot come from vv_mask_boxes;
    # the crop of a 20 x 20 frame inside an 8 x 8 nominal mask can)
    g = dict(H=20, W=20, grid_h=8, grid_w=8, hb=1, wb=1)
    n, _, crops, masks, _ = R.stream_boxes(2, np.array([[9, 9, 15, 15], [2, 2, 9, 9]]), 0, 4, block_mode=1, **g)
    assert n == 2 and masks[0].tolist() == [0, 1, 0, 0] and crops[0].tolist() == [9, 9, 15, 15]


# ---- the synthetic videos of the GPU tests ---------------------------------------------------------------------------------------------
def _restated_boxes(frames, fvi, ap=None):
    import motion_boxes_restatement as M
    out = []
    for i, w in enumerate(R.motion_windows(fvi)):
        f3 = np.stack([np.repeat(frames[k][..., None], 3, axis=2) for k in w])
        out.append(M.get_mt_bboxes(f3, () if ap is None else ap[i][:, :4], 'UCSDped2'))
    return out


def test_the_synthetic_videos_hold_what_the_gpu_tests_rely_on():
    import motion_boxes_restatement as M
    frames, fvi = R.synthetic_frames()
    assert fvi == [1, 1, 1, 1, 2, 2, 2] and all(f.shape == (R.H, R.W) and f.dtype == np.uint8 for f in frames)
    plain = _restated_boxes(frames, fvi)
    counts = [len(b) for b in plain]
    assert sum(c >= 2 for c in counts) >= 2                              # two frames with at least two surviving boxes
    assert counts[-1] == 0 and np.array_equal(frames[-1], frames[-2])   # a frame without a motion box: nothing moves in its window
    assert max(counts) >= 2 and counts.count(max(counts)) >= 1          # the overflow test drops exactly one box of the fullest frame
    assert max(counts) <= R.CAP
    # the small rectangle moves (its component is in the mask) and the area filter rejects it: no box covers it
    k = M.CONSTANTS['UCSDped2']
    w, h, where = R.RECTS[0][2]
    assert (w, h) == R.SMALL
    f3 = np.stack([np.repeat(frames[j][..., None], 3, axis=2) for j in (0, 1, 2)])
    comps = M.label_components(M.motion_mask(f3, k['ksize'], k['binary_thr'], (), k['extend']))
    x, y = where[1]
    small = [c for c in comps if c[1] >= x - 6 and c[1] + c[3] <= x + w + 6 and c[2] >= y - 3 and c[2] + c[4] <= y + h + 3]
    assert small and all(c[5] and (c[3] + 1) * (c[4] + 1) <= k['area_thr'] for c in small)
    assert not any(b[0] <= x and b[2] >= x + w and b[1] <= y and b[3] >= y + h for b in plain[1])
    # every box is a vv_mask_boxes box: inside the frame and not empty
    for b in plain:
        for x1, y1, x2, y2 in np.asarray(b).reshape(-1, 4):
            assert 0 <= x1 < x2 <= R.W and 0 <= y1 < y2 <= R.H
    # with the appearance boxes of the second run the motion box of the covered rectangle is gone from every frame that had one
    ap = R.appearance_boxes()
    covered = _restated_boxes(frames, fvi, ap)
    fewer = 0
    for i, (a, b, p) in enumerate(zip(ap, covered, plain)):
        assert a.shape == (1, 5) and a[0, 0] > 0 and a[0, 1] > 0 and a[0, 2] < R.W and a[0, 3] < R.H
        cx, cy = (a[0, 0] + a[0, 2]) / 2, (a[0, 1] + a[0, 3]) / 2       # the centre of the covered rectangle
        hit = {tuple(q) for q in np.asarray(p).reshape(-1, 4) if q[0] <= cx <= q[2] and q[1] <= cy <= q[3]}
        assert len(hit) <= 1
        assert [tuple(q) for q in np.asarray(b).reshape(-1, 4)] == [tuple(q) for q in np.asarray(p).reshape(-1, 4) if tuple(q) not in hit], i
        fewer += len(hit)
    assert fewer >= 4 and sum(len(b) > 0 for b in covered) >= 2          # boxes disappear, and motion boxes remain behind slot 0
