"""CPU: the host side of ``[mi355x] render`` -- the float64 restatement of the flow colouring against the images the reference's
``flow_to_image`` made (tests/golden/flow_color.npz, written by tests/golden/make_flow_color_golden.py), the colour wheel of the
restatement and of the kernel file against the reference's table, the default colour table, the config keys and the bindings."""
import os
import re

import numpy as np
import pytest

from _util import load_golden, small_config
import render_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_equals_the_reference_images_at_every_element():
    g = load_golden('flow_color')
    for name in ('a', 'b', 'zero'):
        img, rad, unknown = R.flow_parts(g['flow_' + name])
        assert img.dtype == np.uint8 and np.array_equal(img, g['img_' + name]), name
        assert np.array_equal(R.flow_color(g['flow_' + name][None])[0], img)
    assert np.array_equal(R.flow_color(g['flow_batch']), g['img_batch'])
    assert (g['img_zero'] == 255).all()
    # what the fixture is there for: the cut of the wheel, the zero vector, the unknown pixel, one maximum per image, no NaN
    for name in ('a', 'b'):
        fl, img = g['flow_' + name], g['img_' + name]
        (yp, xp), (ym, xm), (yz, xz), (yu, xu) = (tuple(g[k]) for k in ('pos_plus', 'pos_minus', 'pos_zero', 'pos_unknown'))
        assert tuple(fl[yp, xp]) == tuple(fl[ym, xm]) == (2.5, 0.0) and np.signbit(fl[ym, xm, 1]) and not np.signbit(fl[yp, xp, 1])
        assert not np.array_equal(img[yp, xp], img[ym, xm])
        assert tuple(fl[yz, xz]) == (0.0, 0.0) and tuple(img[yz, xz]) == (255, 255, 255)
        assert fl[yu, xu, 0] == 1e9 and tuple(img[yu, xu]) == (0, 0, 0)
    for fl in [g['flow_a'], g['flow_b']] + list(g['flow_batch']):
        assert fl.dtype == np.float32 and not np.isnan(fl).any()
        _, rad, _ = R.flow_parts(fl)
        assert int((np.abs(rad - 1) < 1e-5).sum()) == 1
    assert len({float(np.abs(f).max()) for f in g['flow_batch']}) == 3


def test_wheels_equal_the_reference_table():
    want = load_golden('flow_color')['wheel']
    assert want.shape == (55, 3)
    assert np.array_equal(R.wheel(), want)
    src = open(os.path.join(ROOT, 'vec_vad_amd', 'csrc', 'vv_render.hip')).read()
    table = src[src.index('fc_wheel[FC_NCOLS][3] = {'):]
    table = table[:table.index('};')]
    rows = re.findall(r'\{(\d+), (\d+), (\d+)\}', table)
    assert np.array_equal(np.array(rows, np.float64), want)


def test_restated_overlay_by_hand():
    """One 3 x 4 grey frame: a painted 2 x 2 block, a box outline over part of it, a ground-truth pixel."""
    lut = np.zeros((256, 3), np.uint8)
    lut[:, 0] = np.arange(256)
    lut[:, 2] = 255 - np.arange(256)
    frames = np.full((1, 3, 4, 1), 100, np.uint8)
    mask = np.full((1, 3, 4), R.UNPAINTED)
    mask[0, :2, :2] = 0.5                                    # level floor(0.5 * 255) = 127
    gt = np.zeros((1, 3, 4), np.uint8)
    gt[0, 2, 3] = 7
    out = R.overlay(frames, mask, np.array([[0, 3, 1, 3]], np.int32), np.array([2.0]), [0, 1], 0.0, 1.0, 128, gt=gt, lut=lut)
    blend = [(100 * 128 + c * 128 + 128) >> 8 for c in (127, 0, 128)]
    assert out[0, 0, 0].tolist() == blend and out[0, 1, 0].tolist() == blend
    for y in range(3):                                       # the box is 3 x 2: all of it is outline, score 2 >= hi -> level 255
        assert out[0, y, 1].tolist() == [255, 0, 0] and out[0, y, 2].tolist() == [255, 0, 0]
    assert out[0, 2, 0].tolist() == [100, 100, 100] and out[0, 0, 3].tolist() == [100, 100, 100]
    assert out[0, 2, 3].tolist() == [255, 255, 255]
    assert R.level(100000.0, -3.0, 9.0) == 255 and R.level(-3.0, -3.0, 9.0) == 0 and R.level(9.0, -3.0, 9.0) == 255


def test_colormap_is_a_stable_integer_ramp():
    from vec_vad_amd.render import colormap
    lut = colormap()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and np.array_equal(lut, colormap())
    assert [lut[i].tolist() for i in (0, 63, 64, 127, 128, 191, 192, 255)] == [
        [0, 0, 128], [0, 252, 254], [0, 255, 255], [252, 255, 3], [255, 255, 0], [255, 129, 0], [255, 127, 0], [255, 1, 0]]
    assert len({tuple(c) for c in lut}) == 256
    want = np.zeros((256, 3), np.int64)                       # the formula of the docstring
    for i in range(256):
        s, t = divmod(i, 64)
        want[i] = [(0, 4 * t, 128 + 2 * t), (4 * t, 255, 255 - 4 * t), (255, 255 - 2 * t, 0), (255, 127 - 2 * t, 0)][s]
    assert np.array_equal(lut, want)


BAD = [('render_source = score', 'render_source = fine', "render_source must be 'score' or 'smooth', got 'fine'"),
       ('render_alpha = 50', 'render_alpha = 101', 'render_alpha must be an integer percent in 0..100, got 101'),
       ('render_alpha = 50', 'render_alpha = -1', 'render_alpha must be an integer percent'),
       ('render_alpha = 50', 'render_alpha = 0.5', 'invalid literal'),
       ('render_range = auto', 'render_range = 1', 'render_range must be .auto. or two finite numbers'),
       ('render_range = auto', 'render_range = 2,1', 'render_range must be'),
       ('render_range = auto', 'render_range = 1,1', 'render_range must be'),
       ('render_range = auto', 'render_range = a,b', 'render_range must be'),
       ('render_range = auto', 'render_range = 0,inf', 'render_range must be'),
       ('render_range = auto', 'render_range = nan,1', 'render_range must be'),
       ('render_range = auto', 'render_range = 0,1,2', 'render_range must be'),
       ('render_every = 1', 'render_every = 0', 'render_every must be a frame stride >= 1, got 0'),
       ('render_every = 1', 'render_every = -2', 'render_every must be'),
       ('render_flow_max = 0', 'render_flow_max = -1', 'render_flow_max must be a finite radius >= 0'),
       ('render_flow_max = 0', 'render_flow_max = nan', 'render_flow_max must be'),
       ('render_flow_max = 0', 'render_flow_max = inf', 'render_flow_max must be'),
       ('render = False', 'render = perhaps', 'Not a boolean'),
       ('render_boxes = True', 'render_boxes = 2', 'Not a boolean'),
       ('render_flow = False', 'render_flow = si', 'Not a boolean')]


def test_render_keys_defaults_and_refusals(tmp_path, monkeypatch):
    import train as T
    monkeypatch.chdir(tmp_path)
    cfg = small_config()
    c = T.read_config('config.cfg')
    assert {k: v for k, v in c.items() if k.startswith('render')} == dict(
        render=False, render_source='score', render_alpha=50, render_range='auto', render_every=1, render_boxes=True, render_flow=False,
        render_flow_max=0.0)
    stripped = '\n'.join(l for l in cfg.splitlines() if not l.startswith('render'))      # a config from before the keys: the defaults
    open('config.cfg', 'w').write(stripped)
    assert {k: v for k, v in T.read_config('config.cfg').items() if k.startswith('render')} == {
        k: v for k, v in c.items() if k.startswith('render')}
    for old, new, text in BAD:                               # checked with the stage off
        assert cfg.count(old) == 1, old
        open('config.cfg', 'w').write(cfg.replace(old, new))
        with pytest.raises(ValueError, match=text) as e:
            T.read_config('config.cfg')
        assert '\n' not in str(e.value), new
    open('config.cfg', 'w').write(cfg.replace('render_range = auto', 'render_range = -2.5, 7').replace('render_alpha = 50', 'render_alpha = 100')
                                  .replace('render_flow_max = 0', 'render_flow_max = 12.5').replace('render_every = 1', 'render_every = 3'))
    c = T.read_config('config.cfg')
    assert c['render_range'] == (-2.5, 7.0) and c['render_alpha'] == 100 and c['render_flow_max'] == 12.5 and c['render_every'] == 3


def test_render_source_smooth_needs_smooth_masks(tmp_path, monkeypatch):
    import train as T
    monkeypatch.chdir(tmp_path)
    cfg = small_config().replace('render_source = score', 'render_source = smooth')
    open('config.cfg', 'w').write(cfg.replace('render = False', 'render = True'))
    with pytest.raises(ValueError, match='render_source = smooth needs smooth_masks = True') as e:
        T.read_config('config.cfg')
    assert '\n' not in str(e.value)
    open('config.cfg', 'w').write(cfg.replace('render = False', 'render = True').replace('smooth_masks = False', 'smooth_masks = True'))
    c = T.read_config('config.cfg')
    assert c['render'] and c['render_source'] == 'smooth' and c['smooth_masks']


def test_new_symbols_are_bound():
    from vec_vad_amd import _lib, render
    l = _lib.lib()
    for name in ('vv_flow_color', 'vv_flow_color_work', 'vv_render_overlay'):
        assert name in _lib.EXPORTS and hasattr(l, name)
    assert l.vv_flow_color_work(3, 24, 40) == 3 * 4 and l.vv_flow_color_work(1, 240, 360) == 22 * 4      # one partial per 4096 pixels
    assert l.vv_flow_color_work(0, 5, 5) == 0 and l.vv_flow_color_work(2, 0, 7) == 0
    assert l.vv_flow_color_work(-1, 1, 1) == -1 and l.vv_flow_color_work(1, 65536, 32768) == -1
    assert callable(render.flow_color) and callable(render.overlay) and render.UNPAINTED == -100000.0
