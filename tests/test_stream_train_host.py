"""Host side of training from pushed frames (vec_vad_amd/stream_train.py, stream_train.py): the numpy restatement of
``vv_stream_append`` on hand-made rounds, the meta rows of a collected store against ``foreground.block_groups``, the ``[mi355x]
collect_max_cubes`` key and the refusals that come before any GPU work.  No GPU."""
import os
import re

import numpy as np
import pytest

from stream_train_restatement import stream_append

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def _no_gpu(monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    for name in ('set_device', 'current_device', 'is_available', 'current_stream', 'synchronize'):
        monkeypatch.setattr(torch.cuda, name, touched)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def test_restated_append_on_hand_made_rounds():
    """cap 5, capacity 7, two cells: the launch sequence tests/test_gpu_stream_train.py runs on the device, by hand."""
    cap, capacity = 5, 7
    raw = np.arange(cap * 4, dtype=np.uint8).reshape(cap, 4) + 1
    flow = np.arange(cap * 2, dtype=np.float32).reshape(cap, 2) + 0.5
    flow[1] = np.nan                                                   # an unkept slot of the first round
    masks = np.array([[1, 0, 1, 0, 1], [0, 1, 1, 0, 0]], np.uint8)
    boxes = np.arange(cap * 4, dtype=np.int32).reshape(cap, 4) * 3
    S = dict(raw=np.full((capacity, 4), 201, np.uint8), flow=np.full((capacity, 2), -7.5, np.float32),
             meta=np.full((capacity, 2), -9, np.int32), mbox=np.full((capacity, 4), -9, np.int32), cells=np.full((capacity, 2), 77, np.uint8))

    def run(keep, n, frame, slot0, cursor, bx=boxes):
        return stream_append(raw, flow, np.array(keep, np.uint8), n, masks, bx, frame, slot0, cursor, S['raw'], S['flow'], S['meta'],
                             S['mbox'], S['cells'])

    cur = run([1, 0, 1, 1, 0], 5, 10, 0, 0)
    assert cur == 3 and S['meta'][:3].tolist() == [[10, 0], [10, 2], [10, 3]] and (S['meta'][3:] == -9).all()
    assert np.array_equal(S['raw'][:3], raw[[0, 2, 3]]) and np.array_equal(S['flow'][:3], flow[[0, 2, 3]]) and (S['raw'][3:] == 201).all()
    assert np.array_equal(S['mbox'][:3], boxes[[0, 2, 3]]) and S['cells'][:3].tolist() == [[1, 0], [1, 1], [0, 0]]
    cur = run([1, 1, 1, 1, 1], 3, 11, 5, cur, None)                    # without boxes: zeros
    assert cur == 6 and S['meta'][3:6].tolist() == [[11, 5], [11, 6], [11, 7]] and (S['mbox'][3:6] == 0).all()
    assert np.isnan(S['flow'][4]).all() and np.isfinite(S['flow'][[0, 1, 2, 3, 5]]).all()      # slot 1 is kept now: its bytes travel
    cur = run([1, 1, 1, 1, 1], 4, 12, 0, cur)                          # cube 6 is written, three cubes fall past the capacity
    assert cur == 10 and S['meta'][6].tolist() == [12, 0] and np.array_equal(S['raw'][6], raw[0])
    before = {k: v.copy() for k, v in S.items()}
    assert run([1, 1, 1, 1, 1], 0, 13, 0, cur) == 10                   # n = 0
    assert run([1, 1, 0, 1, 1], 9, 14, 0, cur) == 14                   # at or past the capacity: only the cursor moves; n clamped to cap
    assert run([1, 1, 1, 1, 1], -3, 15, 0, 2) == 2                     # n clamped to 0
    assert all(np.array_equal(before[k].view(np.uint8), S[k].view(np.uint8)) for k in S)


# ---- meta rows to groups -----------------------------------------------------------------------------------------------------------------
def test_meta_rows_give_the_groups_of_block_groups():
    """A 2x3 grid, 6 frames: frame 0 with two cubes, frame 1 with a box in two blocks, frame 2 without a kept cube, frame 3 with one
    cube, frames 4 and 5 empty at the end."""
    import foreground as FG
    from vec_vad_amd.stream_train import meta_groups
    hb, wb, n_frames = 2, 3, 6
    cube_frame = [0, 0, 1, 1, 3]
    cube_blocks = [[(0, 0)], [(1, 2)], [(0, 1), (0, 2)], [(0, 0)], [(1, 2), (0, 0)]]
    meta = np.array([[f, b] for f, b in zip(cube_frame, [0, 3, 1, 64, 2])], np.int32)
    cells = np.zeros((len(cube_frame), hb * wb), np.uint8)
    for s, blocks in enumerate(cube_blocks):
        for hi, wi in blocks:
            cells[s, hi * wb + wi] = 1
    got, want = meta_groups(meta, cells, n_frames, wb), FG.block_groups(cube_frame, cube_blocks, n_frames)
    assert sorted(got) == sorted(want) == [(None, 0, 0), (None, 0, 1), (None, 0, 2), (None, 1, 2)]
    for k in want:
        assert got[k][0].dtype == np.int64 and got[k][1].dtype == np.int32
        assert np.array_equal(got[k][0], want[k][0]) and np.array_equal(got[k][1], want[k][1]), k
    assert got[(None, 0, 0)][0].tolist() == [0, 3, 4] and got[(None, 0, 0)][1].tolist() == [0, 1, 2, 2, 3, 3, 3]
    assert got[(None, 0, 1)][0].tolist() == got[(None, 0, 2)][0].tolist() == [2]         # one cube named by two lists
    # no cube at all: no group
    assert meta_groups(np.zeros((0, 2), np.int32), np.zeros((0, hb * wb), np.uint8), n_frames, wb) == {}
    with pytest.raises(ValueError, match='frame order'):
        meta_groups(meta[::-1], cells[::-1], n_frames, wb)


# ---- keys and refusals -------------------------------------------------------------------------------------------------------------------
def test_collect_max_cubes_in_the_stock_file_and_its_default(tmp_path):
    import train as T
    from vec_vad_amd.stream_train import COLLECT_MAX_CUBES
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'collect_max_cubes') and c['collect_max_cubes'] == COLLECT_MAX_CUBES == 65536
    assert _config_text().count('\ncollect_max_cubes = 65536\n') == 1
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('\ncollect_max_cubes = 65536\n', '\ncollect_max_cubes = 9\n'))
    assert T.read_config(str(p))['collect_max_cubes'] == 9
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith('collect_max_cubes')) + '\n')
    c = T.read_config(str(p))                                          # a file from before the key still parses, with the default
    assert not c['cp'].has_option('mi355x', 'collect_max_cubes') and c['collect_max_cubes'] == 65536


def test_the_new_key_quotes_no_existing_setting():
    """Tests switch keys by replacing ``key = value`` in the file's text: the lines this key added hold no such text of another key."""
    lines = _config_text().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith('; stream_train.py'))
    added = '\n'.join(lines[first:])
    found = re.findall(r'\b\w+ = \S+', added)
    assert found == ['collect_max_cubes = 65536'], found


@pytest.mark.parametrize('bad', ['0', '-1', '1.5', 'many'])
def test_bad_collect_max_cubes_is_refused_before_the_gpu_is_touched(tmp_path, monkeypatch, bad):
    import foreground as FG
    import stream_train as ST
    import train as T
    from vec_vad_amd.stream_train import StreamCollector
    _no_gpu(monkeypatch)
    monkeypatch.setattr(FG, 'load_bboxes', lambda *a, **k: pytest.fail('boxes were loaded'))
    monkeypatch.chdir(tmp_path)
    open('config.cfg', 'w').write(_config_text().replace('\ncollect_max_cubes = 65536\n', '\ncollect_max_cubes = %s\n' % bad))
    for call in (lambda: T.read_config('config.cfg'), lambda: ST.main('config.cfg')):
        with pytest.raises(ValueError, match='collect_max_cubes') as e:
            call()
        assert '\n' not in str(e.value)
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))                # the constructor's own argument, on a good configuration
    for v in (0, -1, 1.5, True, 'many'):
        with pytest.raises(ValueError, match='collect_max_cubes') as e:
            StreamCollector(c, (48, 72, 1), flownet2=object(), max_cubes=v)
        assert '\n' not in str(e.value)
    with pytest.raises(ValueError, match='stream_max_boxes'):
        StreamCollector(c, (48, 72, 1), flownet2=object(), max_boxes=0)
    with pytest.raises(ValueError, match='stream_boxes'):
        StreamCollector(c, (48, 72, 1), flownet2=object(), boxes='found')
    with pytest.raises(ValueError, match='1 or 3 channels'):
        StreamCollector(c, (48, 72, 2), flownet2=object())
    assert os.listdir('.') == ['config.cfg']


def test_shanghaitech_and_a_world_above_one_are_refused_before_the_gpu_is_touched(tmp_path, monkeypatch):
    import foreground as FG
    import stream_train as ST
    import train as T
    from vec_vad_amd.stream_train import StreamCollector
    _no_gpu(monkeypatch)
    monkeypatch.setattr(FG, 'load_bboxes', lambda *a, **k: pytest.fail('boxes were loaded'))
    monkeypatch.chdir(tmp_path)
    open('config.cfg', 'w').write(_config_text().replace('dataset_name = UCSDped2', 'dataset_name = ShanghaiTech'))
    c = T.read_config('config.cfg')
    assert c['dataset_name'] == 'ShanghaiTech'
    for call in (lambda: ST.main('config.cfg'), lambda: StreamCollector(c, (48, 72, 3), flownet2=object())):
        with pytest.raises(NotImplementedError, match='ShanghaiTech') as e:
            call()
        assert str(e.value) == T.DIRECT_TRAIN_SHANGHAI and '\n' not in str(e.value)
    open('config.cfg', 'w').write(_config_text())
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='world of 2') as e:
        ST.main('config.cfg')
    assert '\n' not in str(e.value)
    monkeypatch.setenv('WORLD_SIZE', '1')
    open('config.cfg', 'w').write(_config_text().replace('\nstream_boxes = given\n', '\nstream_boxes = motion\n').replace(
        'foreground_extraction_mode = obj_det_with_motion', 'foreground_extraction_mode = simple_patch'))
    assert T.read_config('config.cfg')['mode_fg'] == 'simple_patch'
    with pytest.raises(ValueError, match='obj_det_with_motion') as e:
        ST.main('config.cfg')
    assert '\n' not in str(e.value)
    assert os.listdir('.') == ['config.cfg']


# ---- the symbol --------------------------------------------------------------------------------------------------------------------------
def test_the_new_symbol_is_exported_declared_and_built():
    from vec_vad_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'vecvad_hip.h')).read()
    assert 'vv_stream_append' in _lib.EXPORTS
    assert re.search(r'^int vv_stream_append\(', header, re.M)
    assert os.path.join(build.CSRC, 'vv_stream_collect.hip') in build.sources()
    assert not build.needs_build()                                     # the library on disk was built from these sources, for gfx950
    assert '--offload-arch=gfx950' in build.FLAGS
    _lib.lib().vv_stream_append                                        # bound: AttributeError if the library lacks it


def test_refused_calls_return_bad_arg_without_a_launch():
    """The refusals come before the launch, so they can be asked for without a GPU: the pointers are never followed."""
    from vec_vad_amd import _lib
    f = _lib.lib().vv_stream_append
    p, q = 4096, 8192

    def call(raw_slots=p, flow_slots=p, keep=p, n=p, cap=5, rb=16, fb=32, masks=p, cells=2, boxes=None, cin=p, cout=q, capacity=7,
             raw_store=p, flow_store=p, meta=p, mbox=p, mcells=p):
        return f(raw_slots, flow_slots, keep, n, cap, rb, fb, masks, cells, boxes, 0, 0, cin, cout, capacity, raw_store, flow_store, meta,
                 mbox, mcells, None)

    bad = [dict(cap=0), dict(cap=-1), dict(cells=-1), dict(capacity=-1), dict(rb=-1), dict(fb=-4), dict(n=None), dict(keep=None),
           dict(cin=None), dict(cout=None), dict(raw_slots=None), dict(flow_slots=None), dict(raw_store=None), dict(flow_store=None),
           dict(meta=None), dict(mbox=None), dict(mcells=None), dict(masks=None), dict(cout=p)]
    for kw in bad:
        assert call(**kw) == 1, kw                                     # VV_ERR_BAD_ARG
