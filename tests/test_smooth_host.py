"""Host side of the spatio-temporal mask smoothing ([mi355x] smooth_masks): the numpy restatement the GPU tests compare the kernels with
(tests/smooth_restatement.py) against an independent brute-force 3-D window loop on dyadic inputs (every sum exact in any order, so
``np.array_equal`` must hold), the consequences of the definition, the three config keys and the lists the scoring calls keep.  No GPU."""
import os

import numpy as np
import pytest

import smooth_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ('smooth_masks', 'smooth_frames', 'smooth_pixels')
BIG = 100000.0
VIDEOS = [0, 0, 0, 1, 2, 2, 2]
WINDOWS = [(1, 1), (3, 3), (5, 9), (1, 27), (15, 1)]


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def dyadic_volume():
    """float64 [7,11,13]: quarters in [-2, 2] inside random boxes over a -BIG background; frame 2 is empty, frame 4 holds a +BIG box."""
    rng = np.random.default_rng(5)
    m = np.full((7, 11, 13), -BIG)
    for f in range(7):
        if f == 2:
            continue
        for _ in range(3):
            y0, x0 = int(rng.integers(0, 9)), int(rng.integers(0, 11))
            y1, x1 = y0 + int(rng.integers(1, 6)), x0 + int(rng.integers(1, 7))
            m[f, y0:y1, x0:x1] = np.maximum(m[f, y0:y1, x0:x1], rng.integers(-8, 9, (min(y1, 11) - y0, min(x1, 13) - x0)) / 4.0)
    m[4, 3:6, 2:5] = BIG
    return m


@pytest.fixture(scope='module')
def volume():
    m = dyadic_volume()
    m.setflags(write=False)
    return m


@pytest.mark.parametrize('kt,ks', WINDOWS)
def test_restatement_equals_the_brute_force_window_on_dyadic_inputs(volume, kt, ks):
    S, fmax = R.smooth(volume, VIDEOS, kt, ks)
    want = R.brute(volume, VIDEOS, kt, ks)
    assert S.dtype == np.float64 and np.array_equal(S, want)
    assert np.array_equal(fmax, want.reshape(7, -1).max(axis=1))
    assert np.array_equal(S != -BIG, volume != -BIG)                       # the support is preserved
    assert fmax[2] == -BIG and (S[2] == -BIG).all()                        # a frame without a box keeps -BIG
    if (kt, ks) == (1, 1):
        assert np.array_equal(S, volume)                                   # identity
    else:
        assert not np.array_equal(S, volume)


def test_a_big_box_floods_its_neighbourhood_and_videos_do_not_mix(volume):
    S, _ = R.smooth(volume, VIDEOS, 5, 9)
    # the box (frame 4, rows 3..5, columns 2..4) is reached by the windows of rows 0..9, columns 0..8 of frames 4, 5, 6 (its video)
    reach = np.zeros(volume.shape, bool)
    reach[4:7, 0:10, 0:9] = True
    painted = volume != -BIG
    assert (painted & reach)[5:].any() and (painted & ~reach)[4:].any()
    # a window holds at most 5 * 81 pixels of at least -2 each: a mean of at least (1e5 - 2 * 404) / 405 > 100 where it holds the box
    assert (S[painted & reach] > 100).all() and (S[painted & ~reach] <= 2.0).all()
    alone, _ = R.smooth(volume[3:4], [1], 5, 9)
    assert np.array_equal(S[3], alone[0])                                  # a one-frame video sees only itself


def test_real_values_depend_on_the_order_so_the_order_is_pinned():
    rng = np.random.default_rng(0)
    m = rng.standard_normal((3, 9, 9))
    S, _ = R.smooth(m, [0, 0, 0], 3, 3)
    other = R.brute(m, [0, 0, 0], 3, 3)
    assert np.abs(S - other).max() < 1e-13 and not np.array_equal(S, other)
    # the X pass of one row by hand, left to right from +0.0
    A = R._shifted_sum(m, 2, 1)
    assert A[0, 0, 0] == (0.0 + m[0, 0, 0]) + m[0, 0, 1] and A[0, 0, 4] == ((0.0 + m[0, 0, 3]) + m[0, 0, 4]) + m[0, 0, 5]


def test_the_three_keys_parse_with_defaults_and_bad_windows_are_rejected(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    for key in KEYS:
        assert c['cp'].has_option('mi355x', key), key
    assert c['smooth_masks'] is False and c['smooth_frames'] == 5 and c['smooth_pixels'] == 9
    text = _config_text()
    assert 'Untuned' in text and 'floods' in text                          # what the stock file must say about the defaults and +BIG
    p = tmp_path / 'config.cfg'
    p.write_text(text.replace('smooth_masks = False', 'smooth_masks = True').replace('smooth_frames = 5', 'smooth_frames = 33')
                 .replace('smooth_pixels = 9', 'smooth_pixels = 1'))
    c = T.read_config(str(p))
    assert c['smooth_masks'] is True and c['smooth_frames'] == 33 and c['smooth_pixels'] == 1
    p.write_text('\n'.join(l for l in text.splitlines() if not l.startswith(KEYS)) + '\n')      # a file from before the keys
    c = T.read_config(str(p))
    assert not any(c['cp'].has_option('mi355x', k) for k in KEYS)
    assert c['smooth_masks'] is False and c['smooth_frames'] == 5 and c['smooth_pixels'] == 9
    for key, stock in (('smooth_frames', 5), ('smooth_pixels', 9)):
        for bad in ('0', '2', '4', '34', '35', '-3', '5.5'):
            p.write_text(text.replace('%s = %d' % (key, stock), '%s = %s' % (key, bad)))
            with pytest.raises(ValueError):
                T.read_config(str(p))


def test_bad_windows_are_refused_before_the_gpu_is_touched(tmp_path, monkeypatch):
    import torch
    import test as S

    def touched(*a, **k):
        raise AssertionError('the GPU was touched')

    monkeypatch.setattr(torch.cuda, 'set_device', touched)
    monkeypatch.chdir(tmp_path)
    open('config.cfg', 'w').write(_config_text().replace('smooth_masks = False', 'smooth_masks = True')
                                  .replace('smooth_pixels = 9', 'smooth_pixels = 8'))
    with pytest.raises(ValueError, match='smooth_pixels must be an odd integer in 1..33, got 8'):
        S.main('config.cfg')


def test_smooth_window_and_host_tensors():
    import torch
    from vec_vad_amd import scoring, _lib
    assert [scoring.smooth_window('k', v) for v in (1, 3, 33, 5.0)] == [1, 3, 33, 5]
    for bad in (0, 2, 34, 35, -1, 2.5, True):
        with pytest.raises(ValueError, match='k must be an odd integer in 1..33'):
            scoring.smooth_window('k', bad)
    with pytest.raises(_lib.VecVadHipError, match='device-resident'):
        scoring.smooth_masks(torch.zeros((2, 3, 4), dtype=torch.float64), [0, 0], 3, 3)


def test_mask_lists_keep_the_groups_only_with_the_key_on():
    import test as S
    gt = lambda i: None                                                    # noqa: E731  -- any ground-truth source
    out = object()
    # what the function returns today, with the key off
    assert S._mask_lists(None, None) == (None, None, None) and S._mask_lists('d', None) == ([], None, None)
    assert S._mask_lists('d', S.PixelEval(device_masks=True)) == (None, [], None)
    assert S._mask_lists(None, S.PixelEval(device_masks=True)) == (None, None, None)
    assert S._mask_lists('d', S.PixelEval(gt, out=out)) == ([], [], None)
    assert S._mask_lists(None, S.PixelEval(maps=True, error_dir='e')) == (None, [], [])
    assert S._mask_lists('d', S.PixelEval(maps=True)) == ([], None, None)
    assert S.PixelEval().groups is None and S.PixelEval(gt, out=out, keep_groups=False).groups is None
    # with it on, the device groups are kept whatever else is asked for
    on = S.PixelEval(keep_groups=True)
    assert on.groups == [] and S._mask_lists(None, on) == (None, [], None) and S._mask_lists('d', on) == ([], [], None)
    assert S._mask_lists('d', S.PixelEval(device_masks=True, keep_groups=True)) == (None, [], None)


def test_smooth_stage_refuses_an_indexer_of_another_length():
    import test as S
    with pytest.raises(ValueError, match='indexes 3 frames, 4 test frames are scored'):
        S._smooth_stage([], [1, 1, 2], 4, 5, 6, 5, 9, 64, 'cpu')
