"""Host side of the direct test path ([mi355x] direct_test): config keys and the pure bookkeeping of
vec_vad_amd/extract.py (chunk windows, table checks) and foreground.py (index lists of a cube store).  No GPU."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def test_config_without_the_new_keys_keeps_the_staged_path(tmp_path):
    import train as T
    lines = [l for l in _config_text().splitlines() if not l.startswith('direct_')]
    p = tmp_path / 'config.cfg'
    p.write_text('\n'.join(lines) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'direct_test')
    assert c['direct_test'] is False
    assert c['direct_frames_per_chunk'] == 64
    # the default store stays below 32 GB at the largest cube (5 raw uint8 + 5 flow float32 patches)
    assert c['direct_max_cubes'] == T.DIRECT_MAX_CUBES
    assert 28e9 < T.DIRECT_MAX_CUBES * (5 * 32 * 32 * 3 + 5 * 32 * 32 * 2 * 4) < 32e9


def test_stock_config_has_the_keys_and_leaves_the_path_off(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for k in ('direct_test', 'direct_frames_per_chunk', 'direct_max_cubes'):
        assert c['cp'].has_option('mi355x', k), k
    assert c['direct_test'] is False and c['direct_frames_per_chunk'] == 64 and c['direct_max_cubes'] == T.DIRECT_MAX_CUBES


def test_new_keys_parse(tmp_path):
    import train as T
    cfg = _config_text().replace('direct_test = False', 'direct_test = True')
    cfg = cfg.replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 2').replace('direct_max_cubes = 524288', 'direct_max_cubes = 10')
    p = tmp_path / 'config.cfg'
    p.write_text(cfg)
    c = T.read_config(str(p))
    assert c['direct_test'] is True and c['direct_frames_per_chunk'] == 2 and c['direct_max_cubes'] == 10


def test_chunk_windows_hold_each_frame_once_with_local_indices():
    """Two videos of 4 and 3 frames, 'predict' windows of 3 frames (context 2).  A chunk of frames 3..5 crosses the video border:
    frame 4 is the first of video 2, so its window repeats it; frame 3's window reaches back before the chunk."""
    from vad_datasets import context_range
    from vec_vad_amd.extract import chunk_windows
    fvi = [1, 1, 1, 1, 2, 2, 2]
    ranges = [context_range(i, 'predict', 2, len(fvi), fvi) for i in (3, 4, 5)]
    assert ranges == [[1, 2, 3], [4, 4, 4], [4, 4, 5]]
    used, win = chunk_windows(ranges)
    assert used == [1, 2, 3, 4, 5]                          # every needed frame once, ascending; frame 0 is not needed
    assert win.dtype == np.int32 and win.tolist() == [[0, 1, 2], [3, 3, 3], [3, 3, 4]]
    for r, w in zip(ranges, win):
        assert [used[k] for k in w] == r
    # the first frame of the whole set: the window repeats frame 0
    r0 = context_range(0, 'predict', 2, len(fvi), fvi)
    used0, win0 = chunk_windows([r0])
    assert r0 == [0, 0, 0] and used0 == [0] and win0.tolist() == [[0, 0, 0]]
    # a centred 'hard' window that repeats the last frame of a video
    rh = context_range(3, 'hard', 1, len(fvi), fvi)
    assert rh == [2, 3, 3]
    usedh, winh = chunk_windows([rh, context_range(4, 'hard', 1, len(fvi), fvi)])
    assert usedh == [2, 3, 4, 5] and winh.tolist() == [[0, 1, 1], [2, 2, 3]]
    # windows of one frame (no context)
    used1, win1 = chunk_windows([[7], [9]])
    assert used1 == [7, 9] and win1.tolist() == [[0], [1]]


def test_block_groups_index_lists_and_offsets():
    from foreground import block_groups
    # 4 frames; cubes 0,1 in frame 0, none in frame 1, cube 2 in frame 2 (lies in two blocks), cube 3 in frame 3
    cube_frame = [0, 0, 2, 3]
    cube_blocks = [[(0, 0)], [(1, 1)], [(0, 1), (0, 0)], [(0, 0)]]
    g = block_groups(cube_frame, cube_blocks, 4)
    assert sorted(g) == [(None, 0, 0), (None, 0, 1), (None, 1, 1)]
    idx, off = g[(None, 0, 0)]
    assert idx.dtype == np.int64 and off.dtype == np.int32
    assert idx.tolist() == [0, 2, 3] and off.tolist() == [0, 1, 1, 2, 3]
    assert g[(None, 0, 1)][0].tolist() == [2] and g[(None, 0, 1)][1].tolist() == [0, 0, 0, 1, 1]
    assert g[(None, 1, 1)][0].tolist() == [1] and g[(None, 1, 1)][1].tolist() == [0, 1, 1, 1, 1]
    # ShanghaiTech: grouped by the scene of the frame as well
    g2 = block_groups(cube_frame, cube_blocks, 4, scene_idx=[1, 1, 2, 2])
    assert sorted(g2) == [(0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1)]
    assert g2[(0, 0, 0)][0].tolist() == [0] and g2[(1, 0, 0)][0].tolist() == [2, 3]
    assert g2[(1, 0, 0)][1].tolist() == [0, 0, 0, 1, 2]
    assert block_groups([], [], 3) == {}
    with pytest.raises(ValueError):
        block_groups([2, 1], [[(0, 0)], [(0, 0)]], 3)


def test_check_tables_refuses_what_the_kernels_would_skip_or_clamp():
    """Chunk of F = 4 frames of 72x80, a store of 6 cubes: the rules of include/vecvad_hip.h for crops, win and slot."""
    from vec_vad_amd.extract import check_tables
    crops = np.array([[0, 0, 80, 72], [10, 8, 42, 40], [79, 71, 80, 72]], np.int32)
    win = np.array([[0, 0, 1], [1, 2, 3], [3, 3, 3]], np.int32)
    slot = np.array([5, -1, 0], np.int32)
    check_tables(crops, win, 4, 72, 80)
    check_tables(crops, win, 4, 72, 80, slot, 6)
    check_tables(np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32), 4, 72, 80, np.zeros(0, np.int32), 6)

    def bad(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    for c in (bad(crops, (1, 2), 81), bad(crops, (1, 3), 73), bad(crops, (1, 0), -1), bad(crops, (1, 1), -1),
              bad(crops, (1, 2), 10), bad(crops, (1, 3), 8)):                     # past an edge, negative, empty
        with pytest.raises(ValueError, match='crop 1'):
            check_tables(c, win, 4, 72, 80, slot, 6)
    for w in (bad(win, (2, 1), 4), bad(win, (2, 1), -1)):
        with pytest.raises(ValueError, match='window 2'):
            check_tables(crops, w, 4, 72, 80, slot, 6)
    with pytest.raises(ValueError, match='box 0 names slot 6'):
        check_tables(crops, win, 4, 72, 80, bad(slot, 0, 6), 6)
    with pytest.raises(ValueError, match='same slot'):
        check_tables(crops, win, 4, 72, 80, bad(slot, 1, 5), 6)
    with pytest.raises(ValueError, match='one entry per crop'):
        check_tables(crops, win, 4, 72, 80, slot[:2], 6)
    with pytest.raises(ValueError, match='one row per crop'):
        check_tables(crops, win[:2], 4, 72, 80)
    check_tables(crops, win, 4, 72, 80, np.array([-1, -1, -3], np.int32), 6)     # skipped boxes may repeat a negative slot
