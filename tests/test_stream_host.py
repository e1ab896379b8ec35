"""Host side of the frame-by-frame scorer (vec_vad_amd/stream.py, stream.py): the ring schedule against ``vad_datasets.context_range``
and ``calc_optical_flow.flow_pairs``, the ``[mi355x] stream_max_boxes`` key, and the numpy restatement of the masked score reduction
that tests/test_gpu_stream.py holds ``vv_stream_scores`` against.  No GPU."""
import os

import numpy as np
import pytest

from stream_restatement import BIG, stream_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFN = 4                                   # context_frame_num of the configuration


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


# ---- schedule ------------------------------------------------------------------------------------------------------------------------
def test_ring_sizes_are_the_window_plus_the_look_ahead():
    from vec_vad_amd.stream import RingSchedule, flow_ring_frames, ring_frames
    assert ring_frames(CFN) == CFN + 2 == 6                # 5 frames of the raw window + the look-ahead frame
    assert flow_ring_frames(0) == 1 and flow_ring_frames(4) == 5
    s = RingSchedule(CFN, 4)
    assert (s.T, s.Tf, s.R, s.Rf) == (5, 5, 6, 5)


# ``context_range`` is the oracle, and it has two limits of its own that the schedule does not have: it refuses a video border inside the
# first ``context_frame_num`` frames of a split, and a window that reaches into a third video (a video shorter than the window that is
# followed by another one).  So the videos run back to back through ONE schedule, and the oracle reads them as splits it accepts: every
# short video is the last of its split.
SPLITS = {'short-last': [(5, n) for n in range(2, 9)], 'mixed': [(8, 4, 7, 5, 6, 4, 2), (4, 3), (6, 8, 5, 2), (7, 3)]}


@pytest.mark.parametrize('context_of_num', [0, 4])
@pytest.mark.parametrize('splits', list(SPLITS.values()), ids=list(SPLITS))
def test_schedule_matches_context_range_and_flow_pairs(splits, context_of_num):
    """Back-to-back videos of 2 to 8 frames through ``RingSchedule`` with a model of the two rings (slot -> frame): every issued
    frame's raw window, flow window and flow pair are the batch route's; every frame is issued exactly once and in order; a pair's
    frames are in the ring when it is issued; no slot is overwritten while a window or pair still to be issued names it."""
    from calc_optical_flow import flow_pairs
    from vad_datasets import context_range
    from vec_vad_amd.stream import RingSchedule
    assert sorted({n for split in splits for n in split}) == list(range(2, 9))
    sched = RingSchedule(CFN, context_of_num)
    ring, flow_ring, flow_made_from, issued = {}, {}, {}, []
    base = 0                                                                       # frames before the split: ring entries are base + index
    for lengths in splits:
        fvi = [v + 1 for v, n in enumerate(lengths) for _ in range(n)]
        total = len(fvi)

        def window(g, num):
            return [base + f for f in context_range(g, 'predict', num, total, fvi)]

        def pair_of(g):
            return tuple(base + f for f in flow_pairs(fvi, [g])[0])

        def check(issue, s0, n):
            g = s0 + issue['frame']
            pair = pair_of(g)
            assert tuple(base + s0 + f for f in issue['pair_frames']) == pair
            assert all(f in ring.values() for f in pair), (g, pair, ring)          # not issued before its pair's frames are there
            assert tuple(ring[s] for s in issue['pair_slots']) == pair
            # the flow of g is written now; the field it replaces must not be named by a window still to be issued (g and later)
            old = flow_ring.get(issue['flow_slot'])
            assert old is None or all(old not in window(t, context_of_num) for t in range(g, s0 + n)), (g, old)
            flow_ring[issue['flow_slot']] = base + g
            flow_made_from[base + g] = tuple(ring[s] for s in issue['pair_slots'])
            want_raw = window(g, CFN)
            assert [base + s0 + f for f in issue['raw_frames']] == want_raw
            assert [ring[s] for s in issue['raw_slots']] == want_raw
            want_flow = window(g, context_of_num)
            assert [base + s0 + f for f in issue['flow_frames']] == want_flow
            assert [flow_ring[s] for s in issue['flow_slots']] == want_flow
            assert len(issue['raw_slots']) == CFN + 1 and len(issue['flow_slots']) == context_of_num + 1
            assert flow_made_from[base + g] == pair
            issued.append(base + g)

        s0 = 0
        for n in lengths:
            for k in range(n):
                slot, issue = sched.push()
                assert 0 <= slot < sched.R
                old = ring.get(slot)
                pending = range(s0 + max(k - 1, 0), s0 + n)                        # frames of this video that are still to be issued
                assert old is None or all(old not in set(window(t, CFN)) | set(pair_of(t)) for t in pending), (s0 + k, old)
                ring[slot] = base + s0 + k
                assert (issue is None) == (k == 0)
                if issue is not None:
                    check(issue, s0, n)
            check(sched.end_video(), s0, n)
            s0 += n
        base += total
    assert issued == list(range(base))                                             # every frame exactly once, in order
    assert sched.end_video() is None                                               # nothing pending between videos


def test_a_one_frame_video_raises_and_the_schedule_goes_on():
    from vec_vad_amd.stream import RingSchedule
    sched = RingSchedule(CFN, 0)
    assert sched.push() == (0, None)
    with pytest.raises(ValueError, match='one frame') as e:
        sched.end_video()
    assert '\n' not in str(e.value)
    assert sched.push() == (0, None)                       # the next video starts from an empty ring
    slot, issue = sched.push()
    assert slot == 1 and issue['frame'] == 0 and issue['pair_frames'] == (0, 0)
    assert sched.end_video()['pair_frames'] == (0, 1)


# ---- keys and defaults ----------------------------------------------------------------------------------------------------------------
def test_stream_max_boxes_in_the_stock_file_and_its_default(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'stream_max_boxes') and c['stream_max_boxes'] == 64
    assert _config_text().count('stream_max_boxes = 64') == 1
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('stream_max_boxes = 64', 'stream_max_boxes = 7'))
    assert T.read_config(str(p))['stream_max_boxes'] == 7
    # a file from before the key still parses, with the default
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith('stream_max_boxes')) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'stream_max_boxes') and c['stream_max_boxes'] == 64


@pytest.mark.parametrize('bad', ['0', '-3', 'many', '2.5', ''])
def test_bad_stream_max_boxes_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch, bad):
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
    open('config.cfg', 'w').write(_config_text().replace('stream_max_boxes = 64', 'stream_max_boxes = ' + bad))
    for call in (lambda: T.read_config('config.cfg'), lambda: STREAM.main('config.cfg'), lambda: StreamScorer.from_config('config.cfg')):
        with pytest.raises(ValueError, match='stream_max_boxes') as e:
            call()
        assert '\n' not in str(e.value)
    # the constructor's own argument, on a good configuration
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for v in (0, -1, 2.5, True, 'x'):
        with pytest.raises(ValueError, match='stream_max_boxes'):
            StreamScorer(c, None, None, None, (48, 72, 1), flownet2=object(), max_boxes=v)
    assert os.listdir('.') == ['config.cfg']               # nothing written either


# ---- score reduction -------------------------------------------------------------------------------------------------------------------
STATS = (3.0, 2.0, 10.0, 4.0)


def test_masked_score_reduction_on_hand_made_inputs():
    raw = np.array([5.0, 9.0, np.nan, 1e30, 7.0, np.nan], np.float32)
    of = np.array([14.0, 2.0, 1e30, np.nan, 18.0, np.nan], np.float32)
    keep = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    mask = np.array([1, 1, 1, 0, 1, 1], np.uint8)
    poison = np.full(6, 123.0)
    box, fs = stream_scores(raw, of, STATS, 1.0, 0.5, keep, 5, mask, poison, -BIG)
    # box 0: (5-3)/2 + 0.5 (14-10)/4 = 1.5; box 1: 3 - 1 = 2; box 2 not kept, box 3 outside the block; box 4: 2 + 1 = 3; slot 5 >= n
    assert box.tolist() == [1.5, 2.0, -BIG, -BIG, 3.0, 123.0] and fs == 3.0
    # max-accumulation into a cell that already holds more, and without the flow term
    box, fs = stream_scores(raw, None, STATS, 2.0, 0.5, keep, 2, mask, poison, 10.0)
    assert box.tolist() == [2.0, 6.0, 123.0, 123.0, 123.0, 123.0] and fs == 10.0
    # a block without a model: +BIG for every box that counts
    box, fs = stream_scores(raw, of, None, 1.0, 0.5, keep, 6, mask, poison, -BIG)
    assert box.tolist() == [BIG, BIG, -BIG, -BIG, BIG, BIG] and fs == BIG


def test_an_all_masked_frame_scores_minus_big():
    raw = np.array([np.nan, np.inf, 1e30, 4.0], np.float32)
    for keep, mask, n in (([0, 0, 0, 0], [1, 1, 1, 1], 4), ([1, 1, 1, 1], [0, 0, 0, 0], 4), ([1, 1, 1, 1], [1, 1, 1, 1], 0)):
        box, fs = stream_scores(raw, raw, STATS, 1.0, 1.0, np.array(keep, np.uint8), n, np.array(mask, np.uint8), np.full(4, 7.0), -BIG)
        assert fs == -BIG
        assert box.tolist() == ([-BIG] * 4 if n else [7.0] * 4)


# ---- the cells of a frame's boxes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('block_mode', [1, 5, 9])
def test_box_cells_under_the_test_rule_and_the_training_rule(block_mode):
    """``box_cells`` on hand-made boxes of a 96 x 144 mask in 48 x 48 cells: under the test rule the bits ``stream_boxes_restatement``
    sets for the same boxes, under the training rule every cell of ``calc_block_idx``; a box outside the grid is refused by both."""
    import stream_boxes_restatement as R
    from utils import calc_block_idx
    from vec_vad_amd.stream_front import box_cells
    grid = dict(grid_h=96, grid_w=144, hb=2, wb=3)
    boxes = np.array([[10, 10, 30, 30],       # well inside cell (0, 0)
                      [-3, 5, 40, 40],        # x1 < 0: the slice wraps to nothing, the box paints no pixel; its probes lie in the grid
                      [40, 4, 70, 20],        # centre x = 55 in column 1, left corner probe (40 + 55) / 2 = 47.5 in column 0: two cells
                      [24, 8, 72, 48]],       # centre (28, 48): x exactly on the boundary of columns 0 and 1
                     np.float64)
    h_step, w_step = grid['grid_h'] / grid['hb'], grid['grid_w'] / grid['wb']
    masks = R.stream_boxes(len(boxes), boxes, 0, len(boxes), 48, 72, block_mode=block_mode, **grid)[3]
    want = [[(r // grid['wb'], r % grid['wb']) for r in np.nonzero(masks[:, b])[0]] for b in range(len(boxes))]
    got = box_cells(boxes, h_step=h_step, w_step=w_step, block_mode=block_mode, painted_only=True, **grid)
    assert got == want and got[1] == [] and got[0] == [(0, 0)]
    assert (len(got[2]) == 2) == (block_mode > 1) and (0, 1) in got[3]
    train = box_cells(boxes, h_step=h_step, w_step=w_step, block_mode=block_mode, painted_only=False, **grid)
    assert train == [sorted(set(calc_block_idx(b[0], b[2], b[1], b[3], h_step, w_step, mode=block_mode))) for b in boxes]
    assert train[1] != [] and [train[i] for i in (0, 2, 3)] == [got[i] for i in (0, 2, 3)]
    outside = np.array([[10, 10, 30, 30], [100, 10, 200, 40]], np.float64)      # centre x = 150: column 3 of 3
    for painted_only in (True, False):
        with pytest.raises(IndexError, match='box 1 falls outside the 2x3 block grid'):
            box_cells(outside, h_step=h_step, w_step=w_step, block_mode=block_mode, painted_only=painted_only, **grid)
