"""Host side of the per-pixel anomaly maps ([mi355x] pixel_maps): the config key, and the numpy restatements
(tests/pixel_maps_restatement.py) the GPU tests compare the kernels with -- the index formula of the fine masks and the k-th largest
value against the criterion it stands for."""
import os

import numpy as np
import pytest

import pixel_maps_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config_text():
    return open(os.path.join(ROOT, 'config.cfg')).read()


def test_pixel_maps_defaults_to_false_and_parses(tmp_path):
    import train as T
    c = T.read_config(os.path.join(ROOT, 'config.cfg'))
    assert c['cp'].has_option('mi355x', 'pixel_maps') and c['pixel_maps'] is False
    p = tmp_path / 'config.cfg'
    p.write_text(_config_text().replace('pixel_maps = False', 'pixel_maps = True'))
    assert T.read_config(str(p))['pixel_maps'] is True
    # a file from before the key
    p.write_text('\n'.join(l for l in _config_text().splitlines() if not l.startswith('pixel_maps')) + '\n')
    c = T.read_config(str(p))
    assert not c['cp'].has_option('mi355x', 'pixel_maps') and c['pixel_maps'] is False
    p.write_text(_config_text().replace('pixel_maps = False', 'pixel_maps = perhaps'))
    with pytest.raises(ValueError):
        T.read_config(str(p))


def test_pixel_eval_defaults_reproduce_the_object_without_maps():
    import test as S
    p = S.PixelEval()
    assert p.maps is False and p.error_dir is None and p.out_fine is None
    assert S._mask_lists('somewhere', p) == ([], None, None) and S._mask_lists(None, None) == (None, None, None)
    with pytest.raises(ValueError, match='out_fine'):
        S.PixelEval(gt=lambda i: None, out=object(), maps=True)
    # maps with neither a directory nor a ground truth have nothing to be formed for
    assert S._mask_lists(None, S.PixelEval(maps=True)) == (None, None, None)
    assert S._mask_lists(None, S.PixelEval(maps=True, error_dir='e')) == (None, [], [])


@pytest.mark.parametrize('lo', [0, 7])
def test_patch_index_stays_in_range_is_monotone_and_the_identity_at_32(lo):
    for n in list(range(1, 100)) + [240, 360, 1000]:
        v = np.arange(lo, lo + n)
        i = R.patch_index(v, lo, lo + n)
        assert i.min() >= 0 and i.max() <= 31, n
        assert (np.diff(i) >= 0).all(), n
        if n == 32:
            assert np.array_equal(i, np.arange(32))
        if n >= 32:
            assert np.array_equal(np.unique(i), np.arange(32)), n       # every source pixel is shown
        else:
            assert len(np.unique(i)) == n, n                            # no source pixel is shown twice
        # the nearest source pixel: the centre of frame pixel t lies inside source pixel i's span of the rectangle
        c = (2 * (v - lo) + 1) * 32
        assert (c >= i * 2 * n).all() and (c < (i + 1) * 2 * n).all()
    assert R.patch_index(5, 5, 6) == 16                                 # one pixel: the middle of the patch


def test_patch_index_of_the_package_is_the_restatement():
    from vec_vad_amd import scoring
    for lo, hi in ((0, 1), (3, 20), (10, 42), (0, 240)):
        v = np.arange(lo, hi)
        assert np.array_equal(scoring.patch_index(v, lo, hi), R.patch_index(v, lo, hi))
    assert scoring.PATCH == R.PATCH and scoring.BIG == R.BIG


def test_kth_largest_agrees_with_a_threshold_sweep():
    rng = np.random.default_rng(41)
    seen_bg = 0
    for trial in range(60):
        h, w = rng.integers(1, 9), rng.integers(1, 9)
        mask = np.round(rng.standard_normal((h, w)) * 2, 0)             # few values: ties across the k-th place
        mask[rng.random((h, w)) < 0.3] = -R.BIG
        gt = (rng.random((h, w)) < (0.0, 0.5, 1.0)[trial % 3]).astype(np.uint8) * 255
        for pct in (1, 40, 100):
            want = R.kth_by_sweep(mask, gt, pct)
            assert R.kth_largest(mask, gt, pct) == want, (trial, pct)
            seen_bg += want == -R.BIG
    assert seen_bg
    assert R.kth_largest(np.zeros((0, 0)), np.zeros((0, 0), np.uint8), 40) == -R.BIG


def test_a_constant_map_paints_the_painted_mask():
    import test as S
    rng = np.random.default_rng(2)
    h, w, n = 37, 53, 9
    from vec_vad_amd import scoring
    x0, y0 = rng.uniform(-6, w, n), rng.uniform(-6, h, n)
    boxes = np.stack([x0, y0, x0 + rng.uniform(0.3, 40, n), y0 + rng.uniform(0.3, 40, n)], 1)
    scores = np.round(rng.standard_normal(n) * 3, 1)
    rects = scoring.box_rects(boxes, h, w)
    z = np.broadcast_to(scores[:, None, None], (n, 32, 32))
    fine = R.paint_error_masks(z, np.array([0, 4, 4, n]), rects, h, w)
    for f, sl in enumerate((slice(0, 4), slice(4, 4), slice(4, n))):
        assert np.array_equal(fine[f], S.paint_frame(scores[sl], boxes[sl], h, w))
