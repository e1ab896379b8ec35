"""Host side of several cameras in one scorer (vec_vad_amd/multistream.py, stream.py): ``MultiSchedule`` against independent
``RingSchedule``s, the tick descriptor on a hand-made tick, the ``[mi355x] stream_cameras`` key, the refusal of the single-camera
features, the lockstep schedule of ``stream.camera_ticks`` and the C ABI's new symbols.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFN = 4                                   # context_frame_num of the configuration


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def _offset(issue, k, R, Rf):
    """A ``RingSchedule`` issue as camera ``k`` of shared rings must see it."""
    out = dict(issue, camera=k, flow_slot=issue['flow_slot'] + k * Rf)
    out['raw_slots'] = [s + k * R for s in issue['raw_slots']]
    out['flow_slots'] = [s + k * Rf for s in issue['flow_slots']]
    out['pair_slots'] = tuple(s + k * R for s in issue['pair_slots'])
    out['motion_slots'] = tuple(s + k * R for s in issue['motion_slots'])
    return out


# per call: ('push', flags) or ('end', cameras | None).  Camera 1 starts a tick late, camera 2 idles, videos end out of phase, camera 0
# ends alone while the others push on, an end of a camera without frames is skipped, and one end names every camera.
CALLS = [('push', (1, 0, 0)), ('push', (1, 1, 0)), ('push', (1, 1, 0)), ('end', [0]), ('push', (1, 1, 1)), ('push', (1, 1, 1)),
         ('push', (0, 1, 1)), ('end', [1, 2]), ('push', (1, 0, 1)), ('end', [1]), ('push', (1, 1, 1)), ('push', (1, 1, 1)),
         ('push', (1, 1, 1)), ('push', (1, 1, 1)), ('push', (1, 1, 1)), ('push', (1, 1, 1)), ('push', (1, 1, 1)), ('end', None)]


@pytest.mark.parametrize('context_of_num', [0, 4])
def test_multi_schedule_is_independent_ring_schedules_with_slot_offsets(context_of_num):
    from vec_vad_amd.multistream import MultiSchedule
    from vec_vad_amd.stream import RingSchedule
    ms = MultiSchedule(3, CFN, context_of_num)
    ones = [RingSchedule(CFN, context_of_num) for _ in range(3)]
    R, Rf = ones[0].R, ones[0].Rf
    assert (ms.T, ms.Tf, ms.R, ms.Rf) == (ones[0].T, ones[0].Tf, R, Rf)
    issued = 0
    for kind, arg in CALLS:
        if kind == 'push':
            want = []
            for k in range(3):
                if arg[k]:
                    slot, issue = ones[k].push()
                    want.append((k, k * R + slot, _offset(issue, k, R, Rf) if issue is not None else None))
            assert ms.push(arg) == want
            issued += sum(w[2] is not None for w in want)
        else:
            want = []
            for k in (range(3) if arg is None else arg):
                issue = ones[k].end_video()
                if issue is not None:
                    want.append((k, _offset(issue, k, R, Rf)))
            assert ms.end_video(arg) == want
            issued += len(want)
        assert [s.count for s in ms.cams] == [s.count for s in ones]
    assert issued == sum(sum(a) for kind, a in CALLS if kind == 'push')          # every pushed frame was issued exactly once
    with pytest.raises(ValueError, match='one flag per camera'):
        ms.push((1, 1))
    with pytest.raises(ValueError, match='cameras must lie in'):
        ms.end_video([3])


def test_a_one_frame_video_on_one_camera_raises_and_changes_no_schedule():
    from vec_vad_amd.multistream import MultiSchedule
    ms = MultiSchedule(3, CFN, 4)
    ms.push((1, 1, 1)), ms.push((1, 0, 1)), ms.push((1, 0, 0))
    assert [s.count for s in ms.cams] == [3, 1, 2]
    for cameras in (None, [0, 1], [2, 1]):
        with pytest.raises(ValueError, match='camera 1: a video that ends after one frame') as e:
            ms.end_video(cameras)
        assert '\n' not in str(e.value)
        assert [s.count for s in ms.cams] == [3, 1, 2]                             # cameras 0 and 2 were not ended either
    assert [k for k, _ in ms.end_video([0, 2])] == [0, 2] and [s.count for s in ms.cams] == [0, 1, 0]


# ---- the tick descriptor ---------------------------------------------------------------------------------------------------------------
def test_tick_descriptor_on_a_hand_made_tick():
    """Three cameras, cap 2, a 2x3 grid.  Camera 0 issues 3 boxes (two rounds), camera 1 is idle, camera 2 issues the last frame of a
    video with one box."""
    from calc_optical_flow import launch_tables
    from vec_vad_amd.multistream import MultiSchedule, TickLayout, tick_descriptor
    cams, cap, hb, wb = 3, 2, 2, 3
    ms = MultiSchedule(cams, CFN, 4)
    for _ in range(7):
        ms.push((1, 0, 1))
    (k0, _, i0), = [p for p in ms.push((1, 0, 0))]
    (k2, i2), = ms.end_video([2])
    assert (k0, k2) == (0, 2) and i0['frame'] == 6 and i2['frame'] == 6
    crops0 = np.array([[1, 2, 30, 40], [5, 6, 70, 80], [9, 10, 110, 120]], np.int32)
    crops2 = np.array([[3, 4, 50, 60]], np.int32)
    blocks0 = [[(0, 0)], [], [(0, 0), (1, 2)]]              # box 1 paints no pixel; box 2 (round 1, slot 0) lies in two cells
    blocks2 = [[(1, 1)]]
    lay = TickLayout(cams, cap, ms.T, ms.Tf, hb, wb)
    d, rounds, rows, used = tick_descriptor(lay, [(0, i0, crops0, blocks0), (2, i2, crops2, blocks2)])
    assert d.dtype == np.int32 and len(d) == lay.words(2) and (rounds, int(d[0]), int(d[1])) == (2, 2, cams)
    assert rows == [(0, 0), (1, 1), (1, 2)] and used == [[0, 1], [0, 2]]
    # the FlowNet2 launch tables: those of launch_tables for the issuing cameras, absolute slots, the tail at row -1
    pairs, out_rows = launch_tables([i0['pair_slots'], i2['pair_slots']], [i0['flow_slot'], i2['flow_slot']], cams)[0]
    assert np.array_equal(d[lay.h_pairs:lay.h_rows].reshape(cams, 2), pairs) and np.array_equal(d[lay.h_rows:lay.h_rows + cams], out_rows)
    assert pairs.tolist() == [[6 % 6, 7 % 6], [2 * 6 + 5, 2 * 6 + 0], [2 * 6 + 5, 2 * 6 + 0]]          # (t, t+1) | (t-1, t) of camera 2, repeated
    assert out_rows.tolist() == [6 % 5, 2 * 5 + 6 % 5, -1]
    want_n = [[2, 0, 1], [1, 0, 0]]                          # the idle camera has n = 0 in every round, camera 2 in its missing round
    for r in range(2):
        rnd = d[lay.head + r * lay.D:lay.head + (r + 1) * lay.D]
        assert rnd[:cams].tolist() == want_n[r]
        crops = rnd[lay.w_crops:lay.w_rwin].reshape(cams, cap, 4)
        assert np.array_equal(crops[0, :want_n[r][0]], crops0[r * cap:(r + 1) * cap])
        assert np.array_equal(rnd[lay.w_rwin:lay.w_fwin].reshape(cams, ms.T)[[0, 2]], [i0['raw_slots'], i2['raw_slots']])
        assert np.array_equal(rnd[lay.w_fwin:lay.w_fwin + cams * ms.Tf].reshape(cams, ms.Tf)[[0, 2]], [i0['flow_slots'], i2['flow_slots']])
        masks = rnd[lay.w_mask:].view(np.uint8)[:hb * wb * cams * cap].reshape(hb * wb, cams * cap)
        want = np.zeros((hb * wb, cams * cap), np.uint8)
        if r == 0:
            want[0 * wb + 0][0 * cap + 0] = 1                # camera 0, box 0, cell (0, 0)
            want[1 * wb + 1][2 * cap + 0] = 1                # camera 2, box 0, cell (1, 1)
            assert np.array_equal(crops[2, 0], crops2[0])
        else:
            want[0 * wb + 0][0 * cap + 0] = want[1 * wb + 2][0 * cap + 0] = 1      # camera 0, box 2 = slot 0 of round 1
        assert np.array_equal(masks, want), r
    assert min(i2['raw_slots']) >= 2 * ms.R and min(i2['flow_slots']) >= 2 * ms.Rf
    # a tick without boxes still has room for one round, and the tables
    d0, rounds0, rows0, used0 = tick_descriptor(lay, [(2, i2, crops2[:0], [])])
    assert (rounds0, rows0, used0, len(d0)) == (0, [], [], lay.words(1)) and d0[lay.h_rows:lay.h_rows + cams].tolist() == [10 + 1, -1, -1]
    for items in ([], [(2, i2, crops2, blocks2), (0, i0, crops0, blocks0)], [(3, i2, crops2, blocks2)]):
        with pytest.raises(ValueError, match='ascending camera order'):
            tick_descriptor(lay, items)
    # one camera: every round is the single-camera round -- n, 3 unused | crops [cap][4] | raw_win [T] | flow_win [Tf], padded to 4 |
    # masks [hb*wb][cap] bytes -- and the header's tables hold the issue's pair and row.  No round, one full round, two rounds.
    from vec_vad_amd.stream import RingSchedule
    cap, hb, wb = 2, 1, 2
    rs = RingSchedule(CFN, 4)
    for _ in range(8):
        _, issue = rs.push()
    T, Tf = rs.T, rs.Tf
    lay1 = TickLayout(1, cap, T, Tf, hb, wb)
    w_mask = (4 + 4 * cap + T + Tf + 3) // 4 * 4
    assert lay1.D == w_mask + (hb * wb * cap + 3) // 4
    all_crops = np.array([[1, 2, 30, 40], [5, 6, 70, 80], [9, 10, 110, 120]], np.int32)
    all_blocks = [[(0, 0)], [(0, 0), (0, 1)], []]
    for n in (0, 2, 3):
        crops, blocks = all_crops[:n], all_blocks[:n]
        d, rounds, rows, used = tick_descriptor(lay1, [(0, issue, crops, blocks)])
        assert rounds == (n + cap - 1) // cap and len(d) == lay1.words(rounds) and len(used) == rounds
        assert tuple(d[lay1.h_pairs:lay1.h_rows]) == issue['pair_slots'] and d[lay1.h_rows] == issue['flow_slot']
        for r in range(max(rounds, 1)):                      # no box: the words of one round are laid out, n = 0 and the windows in them
            m = min(n, (r + 1) * cap) - r * cap
            want = np.zeros(lay1.D, np.int32)
            want[0] = m
            want[4:4 + 4 * m] = crops[r * cap:r * cap + m].reshape(-1)
            want[4 + 4 * cap:4 + 4 * cap + T] = issue['raw_slots']
            want[4 + 4 * cap + T:4 + 4 * cap + T + Tf] = issue['flow_slots']
            masks = want[w_mask:].view(np.uint8)
            for b, cells in enumerate(blocks[r * cap:r * cap + m]):
                for hh, ww in cells:
                    masks[(hh * wb + ww) * cap + b] = 1
            assert np.array_equal(d[lay1.head + r * lay1.D:lay1.head + (r + 1) * lay1.D], want), (n, r)
        # fill_tick on a caller's zeroed buffer, as StreamFront calls it: the same words and lists, the words behind them untouched
        from vec_vad_amd.stream_front import fill_tick
        buf = np.zeros(len(d) + 5, np.int32)
        assert fill_tick(lay1, [(0, issue, crops, blocks)], lay1.rounds([(0, issue, crops, blocks)]), buf) == (rows, used)
        assert np.array_equal(buf, np.concatenate([d, np.zeros(5, np.int32)]))


def test_camera_ticks_deals_videos_round_robin_and_ends_cameras_together():
    import stream as STREAM
    videos = [[0, 1, 2], [3, 4], [5, 6], [7, 8, 9], [10, 11]]          # cameras 0: videos 0, 2, 4; camera 1: videos 1, 3
    assert list(STREAM.camera_ticks(videos, 2)) == [
        ('push', [0, 3]), ('push', [1, 4]), ('end', [1]), ('push', [2, 7]), ('end', [0]), ('push', [5, 8]), ('push', [6, 9]),
        ('end', [0, 1]), ('push', [10, None]), ('push', [11, None]), ('end', [0])]
    assert [a for kind, a in STREAM.camera_ticks(videos[:1], 3) if kind == 'push'] == [[0, None, None], [1, None, None], [2, None, None]]
    for n in (1, 2, 3, 7):                                            # every frame is pushed once, by camera v mod n, in video order
        seen = [[] for _ in range(n)]
        for kind, a in STREAM.camera_ticks(videos, n):
            if kind == 'push':
                for k, f in enumerate(a):
                    if f is not None:
                        seen[k].append(f)
        assert seen == [[f for v in videos[k::n] for f in v] for k in range(n)]


# ---- keys and refusals -------------------------------------------------------------------------------------------------------------------
def _no_gpu(monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    for name in ('set_device', 'current_device', 'is_available', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)


def test_stream_cameras_in_the_stock_file_and_its_default(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'stream_cameras') and c['stream_cameras'] == 1
    assert _config_text().count('\nstream_cameras = 1\n') == 1
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('\nstream_cameras = 1\n', '\nstream_cameras = 8\n'))
    assert T.read_config(str(p))['stream_cameras'] == 8
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith('stream_cameras')) + '\n')
    c = T.read_config(str(p))                                          # a file from before the key still parses, with the default
    assert not c['cp'].has_option('mi355x', 'stream_cameras') and c['stream_cameras'] == 1


@pytest.mark.parametrize('bad', ['0', '-1', '1.5', 'many'])
def test_bad_stream_cameras_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch, bad):
    import foreground as FG
    import stream as STREAM
    import train as T
    from vec_vad_amd.multistream import MultiStreamScorer
    _no_gpu(monkeypatch)
    monkeypatch.setattr(FG, 'load_bboxes', lambda *a, **k: pytest.fail('boxes were loaded'))
    monkeypatch.chdir(tmp_path)
    open('config.cfg', 'w').write(_config_text().replace('\nstream_cameras = 1\n', '\nstream_cameras = %s\n' % bad))
    for call in (lambda: T.read_config('config.cfg'), lambda: STREAM.main('config.cfg'), lambda: MultiStreamScorer.from_config('config.cfg')):
        with pytest.raises(ValueError, match='stream_cameras') as e:
            call()
        assert '\n' not in str(e.value)
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))                # the constructor's own argument, on a good configuration
    for v in (0, -1, 1.5, True, 'x'):
        with pytest.raises(ValueError, match='stream_cameras'):
            MultiStreamScorer(c, None, None, None, (48, 72, 1), v, flownet2=object())
    assert os.listdir('.') == ['config.cfg']


REFUSED = {'stream_boxes': ('stream_boxes = given', 'stream_boxes = motion'), 'stream_masks': ('stream_masks = off', 'stream_masks = on'),
           'stream_smooth': ('stream_smooth = off', 'stream_smooth = on'), 'stream_render': ('stream_render = off', 'stream_render = on'),
           'stream_tracks': ('stream_tracks = off', 'stream_tracks = on')}


@pytest.mark.parametrize('key', sorted(REFUSED))
def test_single_camera_features_are_refused_with_one_line_each(tmp_path, monkeypatch, key):
    import foreground as FG
    import stream as STREAM
    import train as T
    from vec_vad_amd.multistream import SINGLE_CAMERA_KEYS, MultiStreamScorer, check_single_camera_keys
    assert sorted(SINGLE_CAMERA_KEYS) == sorted(REFUSED)
    _no_gpu(monkeypatch)
    monkeypatch.setattr(FG, 'load_bboxes', lambda *a, **k: pytest.fail('boxes were loaded'))
    monkeypatch.chdir(tmp_path)
    off, on = REFUSED[key]
    text = _config_text()
    assert text.count('\n' + off + '\n') == 1
    open('config.cfg', 'w').write(text.replace('\n' + off + '\n', '\n' + on + '\n').replace('\nstream_cameras = 1\n', '\nstream_cameras = 2\n'))
    c = T.read_config('config.cfg')
    assert c['stream_cameras'] == 2
    calls = (lambda: check_single_camera_keys(c), lambda: STREAM.main('config.cfg'), lambda: MultiStreamScorer.from_config('config.cfg'),
             lambda: MultiStreamScorer(c, None, None, None, (48, 72, 1), 2, flownet2=object()))
    for call in calls:
        with pytest.raises(ValueError, match=re.escape('[mi355x] {} = '.format(key)) + '.*single-camera feature') as e:
            call()
        assert '\n' not in str(e.value)
    check_single_camera_keys(T.read_config(os.path.join(ROOT, 'config.cfg')))      # the stock file switches none of them on
    assert os.listdir('.') == ['config.cfg']


def test_new_symbols_are_exported_and_declared():
    from vec_vad_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'vecvad_hip.h')).read()
    for name in ('vv_stream_cut_multi', 'vv_stream_scores_multi'):
        assert name in _lib.EXPORTS
        assert re.search(r'^int %s\(' % name, header, re.M), name
