"""Host side of the per-pixel error mask of a stream ([mi355x] stream_maps; vec_vad_amd/stream.py, vv_stream_zpaint): the restatement
that tests/test_gpu_stream_maps.py holds the kernel against is itself checked on hand-made launches; the key; the refusal with several
cameras; the symbol.  No GPU."""
import os
import re

import numpy as np
import pytest

import stream_maps_restatement as R
import stream_masks_restatement as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = R.BIG
STATS = (3.25, 1.5, 0.75, 0.5)
W_RAW, W_OF = 1.0, 0.5


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def _maps(cap, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((cap, 32, 32)) * 0.01).astype(np.float32), (rng.random((cap, 32, 32)) * 0.002).astype(np.float32)


def _one(rect, h=70, w=90, flow=True):
    """One counted slot with the rectangle ``rect``: ``(mask, z)``."""
    e_raw, e_of = _maps(1)
    rects = np.array([rect], np.int32)
    got = R.launch(e_raw, e_of if flow else None, STATS, W_RAW, W_OF, [1], [1], 1, 0, rects, 1, None, h, w)
    return got, R.zmap(e_raw[0], e_of[0] if flow else None, STATS, W_RAW, W_OF)


def test_a_32_wide_rectangle_copies_the_map():
    for flow in (True, False):
        got, z = _one((5, 37, 11, 43), flow=flow)
        assert np.array_equal(_bits(got[5:37, 11:43]), _bits(z))
        outside = np.ones(got.shape, bool)
        outside[5:37, 11:43] = False
        assert (got[outside] == -BIG).all()
    e_raw, e_of = _maps(1)                                                # the expression, once, by hand on one pixel
    r, o = np.float64(np.float32(1024) * e_raw[0, 3, 4]), np.float64(np.float32(1024) * e_of[0, 3, 4])
    assert _one((5, 37, 11, 43))[0][5 + 3, 11 + 4] ==W_RAW * ((r - STATS[0]) / STATS[1]) + W_OF * ((o - STATS[2]) / STATS[3])


@pytest.mark.parametrize('side', [16, 48])
def test_a_shrunk_and_a_stretched_rectangle_pick_the_rows_patch_index_names(side):
    from vec_vad_amd.scoring import patch_index
    y0, x0 = 7, 9
    got, z = _one((y0, y0 + side, x0, x0 + side))
    idx = [patch_index(v, 0, side) for v in range(side)]
    assert idx == [((2 * v + 1) * 32) // (2 * side) for v in range(side)] and idx == sorted(idx) and idx[-1] == 31
    assert idx == list(range(1, 32, 2)) if side == 16 else (idx[0] == 0 and sorted(set(idx)) == list(range(32)))
    for y in range(side):
        for x in range(side):
            assert got[y0 + y, x0 + x] == z[idx[y], idx[x]]
    assert (got == -BIG).sum() == got.size - side * side


def test_two_overlapping_boxes_give_the_maximum():
    e_raw, e_of = _maps(2, seed=1)
    rects = np.array([[4, 36, 4, 36], [20, 52, 20, 52]], np.int32)
    got = R.launch(e_raw, e_of, STATS, W_RAW, W_OF, [1, 1], [1, 1], 2, 0, rects, 2, None, 60, 60)
    z = [R.zmap(e_raw[b], e_of[b], STATS, W_RAW, W_OF) for b in range(2)]
    assert np.array_equal(got[4:20, 4:36], z[0][:16]) and np.array_equal(got[36:52, 20:52], z[1][16:])
    assert np.array_equal(got[20:36, 20:36], np.maximum(z[0][16:, 16:], z[1][:16, :16]))
    assert (z[0][16:, 16:] > z[1][:16, :16]).any() and (z[0][16:, 16:] < z[1][:16, :16]).any()


def test_a_dropped_box_a_box_of_another_block_and_a_padded_slot_leave_no_trace():
    e_raw, e_of = _maps(5, seed=2)
    rects = np.array([[0, 32, 0, 32], [10, 40, 10, 50], [5, 25, 30, 60], [30, 50, 0, 20], [0, 50, 0, 60]], np.int32)
    keep, mask, n = [1, 0, 1, 1, 1], [1, 1, 0, 1, 1], 4                    # slot 1 dropped, slot 2 of another block, slot 4 >= n
    for b in (1, 2, 4):
        e_raw[b], e_of[b] = np.nan, np.inf
    got = R.launch(e_raw, e_of, STATS, W_RAW, W_OF, keep, mask, n, 0, rects, 5, None, 50, 60)
    want = R.launch(e_raw[[0, 3]], e_of[[0, 3]], STATS, W_RAW, W_OF, [1, 1], [1, 1], 2, 0, rects[[0, 3]], 2, None, 50, 60)
    assert np.isfinite(got).all() and np.array_equal(_bits(got), _bits(want))
    assert (got[0:32, 0:32] > -BIG).all() and (got[30:50, 0:20] > -BIG).all() and (got == -BIG).sum() == got.size - 32 * 32 - 20 * 20 + 2 * 20
    assert (R.launch(e_raw, e_of, STATS, W_RAW, W_OF, keep, mask, 0, 0, rects, 5, None, 50, 60) == -BIG).all()


def test_a_block_without_a_model_paints_big_and_launches_accumulate():
    e_raw, e_of = _maps(2, seed=3)
    rects = np.array([[2, 20, 3, 30], [10, 40, 12, 44]], np.int32)
    first = R.launch(None, None, None, W_RAW, W_OF, [1, 1], [1, 0], 2, 0, rects, 2, None, 45, 50)
    assert (first[2:20, 3:30] == BIG).all() and (first == BIG).sum() == 18 * 27 and (first[first != BIG] == -BIG).all()
    kw = [dict(e_raw=None, e_of=None, stats=None, w_raw=W_RAW, w_of=W_OF, keep=[1, 1], mask=[1, 0], n=2, slot0=0, rects=rects, n_host=2,
               boxes=None),
          dict(e_raw=e_raw, e_of=e_of, stats=STATS, w_raw=W_RAW, w_of=W_OF, keep=[1, 1], mask=[0, 1], n=2, slot0=0, rects=rects, n_host=2,
               boxes=None)]
    both = R.frame(kw, 45, 50)
    assert (both[2:20, 3:30] == BIG).all() and (np.abs(both[20:40, 12:44]) < BIG).all()
    assert np.array_equal(both, np.maximum(first, R.launch(h=45, w=50, **kw[1])))
    assert (R.frame([], 45, 50) == -BIG).all()


def test_rounds_and_device_rectangles():
    """Slot b of a round reads row slot0 + b of the frame's table; rows at or above n_host are Python's slicing of the device's boxes."""
    e_raw, e_of = _maps(2, seed=4)
    h, w = 40, 60
    boxes = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [3, 4, 35, 36], [-20, -10, 70, 45]], np.int32)       # x1, y1, x2, y2
    rects = np.zeros((4, 4), np.int32)
    rects[2] = (1, 2, 3, 4)                                                # a host row: used for slot 0 of the round when n_host = 3
    got = R.launch(e_raw, e_of, STATS, W_RAW, W_OF, [1, 1], [1, 1], 2, 2, rects, 2, boxes, h, w)
    want_rects = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [4, 36, 3, 35], [30, 40, 40, 60]], np.int32)
    assert np.array_equal(R.resolve(boxes, h, w)[2:], want_rects[2:])
    assert np.array_equal(got, R.launch(e_raw, e_of, STATS, W_RAW, W_OF, [1, 1], [1, 1], 2, 2, want_rects, 4, None, h, w))
    host = R.launch(e_raw, e_of, STATS, W_RAW, W_OF, [1, 1], [1, 1], 2, 2, rects, 3, boxes, h, w)
    assert (host[1:2, 3:4] > -BIG).all() and (host[4:30, 3:35] == -BIG).all()


@pytest.mark.parametrize('flow', [True, False])
def test_constant_maps_reproduce_the_painted_score_mask(flow):
    """e = c everywhere, so the cube's error sum is 1024 c: the fine mask is the score mask of the same boxes, to the bit."""
    h, w = 50, 64
    c_raw = np.array([3 / 1024, 5 / 4096, 16383 / 2 ** 24, 7 / 512], np.float32)      # at most 14 significant bits: 1024 c is exact
    c_of = np.array([1 / 2048, 9 / 8192, 3 / 256, 11 / 4096], np.float32)
    e_raw, e_of = np.broadcast_to(c_raw[:, None, None], (4, 32, 32)).copy(), np.broadcast_to(c_of[:, None, None], (4, 32, 32)).copy()
    rects = np.array([[0, 32, 0, 32], [10, 45, 20, 64], [5, 20, 5, 15], [30, 50, 0, 40]], np.int32)
    keep, mask, n = [1, 1, 0, 1], [1, 1, 1, 1], 4
    got = R.launch(e_raw, e_of if flow else None, STATS, W_RAW, W_OF, keep, mask, n, 0, rects, 4, None, h, w)
    sums_r, sums_o = (np.float32(1024) * c_raw).astype(np.float64), (np.float32(1024) * c_of).astype(np.float64)
    assert np.array_equal(sums_r, e_raw.astype(np.float64).reshape(4, -1).sum(1))      # the error sum of the cube, exactly
    score = W_RAW * ((sums_r - STATS[0]) / STATS[1])
    if flow:
        score = score + W_OF * ((sums_o - STATS[2]) / STATS[3])
    row = np.where(np.array(keep, bool) & np.array(mask, bool), score, -BIG)
    want, _ = SM.paint([row], n, rects, h, w)
    assert np.array_equal(_bits(got), _bits(want)) and (np.abs(got) < BIG).any()


# ---- the key -----------------------------------------------------------------------------------------------------------------------------
def test_stream_maps_in_the_stock_file_and_its_default(tmp_path):
    import train as T
    text = _config_text()
    assert text.count('\nstream_maps = off\n') == 1 and len(re.findall(r'^stream_maps\b', text, re.M)) == 1
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'stream_maps') and c['stream_maps'] is False
    p = tmp_path / 'config.cfg'
    p.write_text('\n'.join(l for l in text.splitlines() if not l.startswith('stream_maps')) + '\n')
    c = T.read_config(str(p))                                              # a file from before the key still parses, with the default
    assert not c['cp'].has_option('mi355x', 'stream_maps') and c['stream_maps'] is False
    p.write_text(text.replace('\nstream_maps = off\n', '\nstream_maps = on\n'))
    assert T.read_config(str(p))['stream_maps'] is True


def test_the_comment_of_the_key_says_what_it_leaves_alone():
    text = _config_text()
    comment = text[:text.index('\nstream_maps = off\n')].rsplit('\nstream_max_tracks', 1)[1]
    assert 'StreamResult.error_mask' in comment and 'costs' in comment and 'not on this one' in comment


# ---- several cameras ---------------------------------------------------------------------------------------------------------------------
def _no_gpu(monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    for name in ('set_device', 'current_device', 'is_available', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)


def test_stream_maps_with_several_cameras_is_refused_with_one_line(tmp_path, monkeypatch):
    import foreground as FG
    import stream as STREAM
    import train as T
    from vec_vad_amd.multistream import SINGLE_CAMERA_KEYS, MultiStreamScorer, check_single_camera_keys
    assert len(SINGLE_CAMERA_KEYS) == 5 and 'stream_maps' not in SINGLE_CAMERA_KEYS      # a check of its own
    _no_gpu(monkeypatch)
    monkeypatch.setattr(FG, 'load_bboxes', lambda *a, **k: pytest.fail('boxes were loaded'))
    monkeypatch.chdir(tmp_path)
    text = _config_text()
    open('config.cfg', 'w').write(text.replace('\nstream_maps = off\n', '\nstream_maps = on\n').replace('\nstream_cameras = 1\n',
                                                                                                       '\nstream_cameras = 2\n'))
    c = T.read_config('config.cfg')
    assert c['stream_cameras'] == 2 and c['stream_maps'] is True
    check_single_camera_keys(c)                                            # the five keys it knows are off
    calls = (lambda: STREAM.main('config.cfg'), lambda: MultiStreamScorer.from_config('config.cfg'),
             lambda: MultiStreamScorer(c, None, None, None, (48, 72, 1), 2, flownet2=object()))
    for call in calls:
        with pytest.raises(ValueError, match=re.escape('[mi355x] stream_maps = on') + '.*single-camera feature') as e:
            call()
        assert '\n' not in str(e.value)
    assert os.listdir('.') == ['config.cfg']


def test_the_symbol_is_exported_and_declared():
    from vec_vad_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'vecvad_hip.h')).read()
    assert 'vv_stream_zpaint' in _lib.EXPORTS
    assert re.search(r'^int vv_stream_zpaint\(', header, re.M)
    assert len(_lib._SIGS['vv_stream_zpaint'][1]) == header[header.index('\nint vv_stream_zpaint('):].split(';')[0].count(',') + 1
