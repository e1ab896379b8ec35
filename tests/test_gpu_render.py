"""Pictures on the GPU ([mi355x] render): ``render.flow_color`` / vv_flow_color against the images the reference's ``flow_to_image`` made
(tests/golden/flow_color.npz) and against the float64 restatement, ``render.overlay`` / vv_render_overlay against the restatement bit for
bit (tests/render_restatement.py), then the script level (``test.main`` staged, direct and direct in parts).

The bar of the flow colouring: every byte within 1 level of the float64 result -- the kernel works in float32, an error of ~1e-5 in a
colour in 0..1 against steps of 1/255, and the mapping is continuous but for the branch at ``rad <= 1``: pixels whose float64 normalised
radius lies within 1e-5 of 1 (at most 2 per image; the pixel of the largest radius is one) are left out, no other."""
import glob
import os
import sys
import zipfile

import numpy as np
import pytest
import torch

from _util import load_golden, small_config
import render_restatement as R

pytestmark = pytest.mark.gpu

BIG = 100000.0
SENT = 0x5A                                    # sentinel behind / all over an output
GUARD = 4096                                   # guard bytes behind the work buffer
OK, BAD_ARG = 0, 1


# ---- vv_flow_color ------------------------------------------------------------------------------------------------------------------
def check_flow(got, flow, maxrad=0.0, want=None, what=''):
    """``got`` uint8 [h,w,3] against the float64 image of ``flow`` (``want``: the reference's own image, which the restatement equals)
    under the bar of the module docstring."""
    img, rad, unknown = R.flow_parts(flow, maxrad)
    if want is not None:
        assert np.array_equal(img, want)
    band = np.abs(rad - 1) < 1e-5
    diff = np.abs(got.astype(np.int64) - img.astype(np.int64)).max(axis=2)
    print('%s: %d of %d bytes differ, largest difference %d outside the band of %d pixels (%d inside)' % (
        what, int((got != img).sum()), img.size, int(diff[~band].max(initial=0)), int(band.sum()), int(diff[band].max(initial=0))))
    assert got.dtype == np.uint8 and got.shape == img.shape
    assert int(band.sum()) <= 2
    assert (diff[~band] <= 1).all()
    assert (got[unknown] == 0).all()


def raw_flow_color(flow, maxrad=0.0):
    """vv_flow_color through ctypes: a work buffer of exactly the reported size with guard bytes behind it, a sentinel image behind the
    output."""
    from vec_vad_amd import _lib
    l = _lib.lib()
    n, h, w, _ = flow.shape
    nb = int(l.vv_flow_color_work(n, h, w))
    assert nb == n * ((h * w + 4095) // 4096) * 4
    work = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.full((n + 1, h, w, 3), SENT, dtype=torch.uint8, device='cuda')
    rc = l.vv_flow_color(flow.data_ptr(), n, h, w, maxrad, out.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == OK, rc
    torch.cuda.synchronize()
    assert bool((work[nb:] == 0xA5).all()), 'the kernels wrote behind the work buffer'
    assert bool((out[-1] == SENT).all())
    return out[:-1]


@pytest.mark.parametrize('name', ['a', 'b', 'zero'])
def test_flow_color_against_the_reference_images(name):
    from vec_vad_amd import render
    g = load_golden('flow_color')
    flow, want = g['flow_' + name], g['img_' + name]
    dev = torch.from_numpy(flow).cuda()
    got = render.flow_color(dev)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape and got.is_cuda
    check_flow(got.cpu().numpy(), flow, want=want, what=name)
    raw = raw_flow_color(dev[None])
    assert torch.equal(raw[0], got) and torch.equal(render.flow_color(dev[None])[0], got)
    assert torch.equal(render.flow_color(dev), got)                        # run to run
    assert torch.equal(dev.cpu(), torch.from_numpy(flow))                  # the input is not written
    got = got.cpu().numpy()
    if name == 'zero':
        assert (got == 255).all()
    else:                                                                  # the cut of the wheel, the zero vector, the unknown pixel: exact
        for key in ('pos_plus', 'pos_minus', 'pos_unknown', 'pos_zero'):
            y, x = g[key]
            assert got[y, x].tolist() == want[y, x].tolist(), key
        assert got[tuple(g['pos_plus'])].tolist() != got[tuple(g['pos_minus'])].tolist()


def test_flow_color_batch_is_image_by_image():
    from vec_vad_amd import render
    g = load_golden('flow_color')
    flow = torch.from_numpy(g['flow_batch']).cuda()
    got = render.flow_color(flow)
    for k in range(3):
        check_flow(got[k].cpu().numpy(), g['flow_batch'][k], want=g['img_batch'][k], what='batch[%d]' % k)
        assert torch.equal(render.flow_color(flow[k]), got[k]) and torch.equal(render.flow_color(flow[k:k + 1])[0], got[k])
    assert torch.equal(raw_flow_color(flow), got)
    assert torch.equal(render.flow_color(flow.flip(0)), got.flip(0))       # an image does not see its neighbours
    big = torch.from_numpy(np.tile(g['flow_b'], (3, 2, 1))).cuda()         # 144 x 128: more than one partial (4096 pixels) per image
    both = torch.stack([big, big * 0.5])
    out = render.flow_color(both)
    assert torch.equal(out[0], out[1])                                     # a scaled field has the same picture: powers of two are exact
    one = render.flow_color(torch.from_numpy(g['flow_b']).cuda())          # checked against the reference above; the tiles share its maximum
    assert all(torch.equal(out[0][y:y + 48, x:x + 64], one) for y in (0, 48, 96) for x in (0, 64))


def test_flow_color_fixed_radius_nan_and_small_shapes():
    from vec_vad_amd import render
    g = load_golden('flow_color')
    flow = g['flow_a'].copy()
    dev = torch.from_numpy(flow).cuda()
    for maxrad in (4.0, 11.5, 100.0):                                      # below the largest radius (rad > 1 for many pixels) and above it
        got = render.flow_color(dev, maxrad)
        check_flow(got.cpu().numpy(), flow, maxrad, what='maxrad %g' % maxrad)
        assert torch.equal(raw_flow_color(dev[None], maxrad)[0], got)
    assert int((R.flow_parts(flow, 4.0)[1] > 1).sum()) > 100
    from vec_vad_amd import _lib                                            # a fixed radius needs no work buffer
    out = torch.full((1, 24, 40, 3), SENT, dtype=torch.uint8, device='cuda')
    assert _lib.lib().vv_flow_color(dev.data_ptr(), 1, 24, 40, 4.0, out.data_ptr(), None, torch.cuda.current_stream().cuda_stream) == OK
    assert torch.equal(out[0], render.flow_color(dev, 4.0))
    nan = flow.copy()                                                      # NaN pixels: unknown, not the whole image black
    nan[2, 3, 0] = np.nan
    nan[5, 30, 1] = np.nan
    nan[20, 20] = np.nan
    nan[tuple(g['pos_max'])] = np.nan                                      # the pixel of the largest radius: the maximum is another's now
    for maxrad in (0.0, 6.0):
        got = render.flow_color(torch.from_numpy(nan).cuda(), maxrad).cpu().numpy()
        check_flow(got, nan, maxrad, what='NaN pixels, maxrad %g' % maxrad)
        assert (got[np.isnan(nan).any(axis=2)] == 0).all() and (got != 0).any()
    # one pixel, and nothing at all
    one = torch.tensor([[[[3.0, -4.0]]]], device='cuda')
    assert tuple(render.flow_color(one).shape) == (1, 1, 1, 3)             # its own maximum: rad is within rounding of 1, no byte to compare
    check_flow(render.flow_color(one, 10.0)[0].cpu().numpy(), one[0].cpu().numpy(), 10.0, what='1 x 1')
    assert render.flow_color(torch.zeros((1, 1, 1, 2), device='cuda')).flatten().tolist() == [255, 255, 255]
    assert render.flow_color(torch.tensor([[[[1e9, 0.0]]]], device='cuda')).flatten().tolist() == [0, 0, 0]
    assert tuple(render.flow_color(torch.zeros((0, 5, 7, 2), device='cuda')).shape) == (0, 5, 7, 3)
    assert tuple(render.flow_color(torch.zeros((2, 0, 7, 2), device='cuda')).shape) == (2, 0, 7, 3)
    assert tuple(raw_flow_color(torch.zeros((0, 5, 7, 2), device='cuda')).shape) == (0, 5, 7, 3)


def test_flow_color_refusals_write_nothing():
    from vec_vad_amd import _lib, render
    l = _lib.lib()
    flow = torch.ones((2, 5, 7, 2), device='cuda')
    out = torch.full((2, 5, 7, 3), SENT, dtype=torch.uint8, device='cuda')
    work = torch.full((64,), SENT, dtype=torch.uint8, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def call(f=flow.data_ptr(), n=2, h=5, w=7, maxrad=0.0, o=out.data_ptr(), wk=work.data_ptr()):
        return l.vv_flow_color(f, n, h, w, maxrad, o, wk, st)

    for kw in (dict(f=None), dict(o=None), dict(wk=None), dict(n=-1), dict(h=-5), dict(w=-7), dict(h=65536, w=32768), dict(maxrad=float('nan')),
               dict(f=flow.data_ptr() + 4), dict(wk=work.data_ptr() + 2), dict(o=None, maxrad=3.0)):
        assert call(**kw) == BAD_ARG, kw
    assert call(n=0, f=None, o=None, wk=None) == OK and call(h=0, f=None, o=None, wk=None) == OK and call(w=0) == OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((work == SENT).all())
    for kw, text in ((dict(flow=flow.double()), 'flow must be a float32 .n,h,w,2. tensor'), (dict(flow=flow[..., :1]), 'flow must be a float32'),
                     (dict(flow=flow[0, 0]), 'flow must be a float32'), (dict(flow=flow, maxrad=float('nan')), 'maxrad must be a number'),
                     (dict(flow=[1.0]), 'flow must be a float32')):
        with pytest.raises(ValueError, match=text) as e:
            render.flow_color(**kw)
        assert '\n' not in str(e.value)
    with pytest.raises(_lib.VecVadHipError, match='device-resident'):
        render.flow_color(flow.cpu())


# ---- vv_render_overlay --------------------------------------------------------------------------------------------------------------
LO, HI = -1.0, 2.0
_cases = {}


def overlay_case(h, w, c):
    """Two frames.  Frame 0 has no box; frame 1 has more boxes than one LDS pass holds (256), among them overlapping ones, boxes on the
    frame border, one clipped to empty by ``box_rects``, an empty one, boxes one pixel wide / high / in all, and scores at, below and above
    both ends of the range and at +BIG.  The masks hold the same kinds of value; the ground truth touches the border and has a one-pixel
    region.  Built once per shape, read-only."""
    if (h, w, c) in _cases:
        return _cases[h, w, c]
    from vec_vad_amd import scoring
    rng = np.random.default_rng(1000 * h + 10 * w + c)
    frames = rng.integers(0, 256, (2, h, w, c), dtype=np.uint8)
    mask = np.full((2, h, w), -BIG)
    gt = np.zeros((2, h, w), np.uint8)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    if h * w == 1:
        mask[1] = 0.25
        gt[0] = 1
        rects = np.array([[0, 1, 0, 1], [0, 0, 0, 1], [0, 1, 0, 1]], np.int32)
        scores = np.array([0.5, 9.0, -0.5])
    else:
        for f in range(2):
            for _ in range(5):
                y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
                y1, x1 = min(h, y0 + int(rng.integers(1, h // 2 + 2))), min(w, x0 + int(rng.integers(1, w // 2 + 2)))
                mask[f, y0:y1, x0:x1] = np.maximum(mask[f, y0:y1, x0:x1], 1.5 * rng.standard_normal((y1 - y0, x1 - x0)))
        mask[0, 0, :6] = [LO, HI, BIG, LO - 1e-9, HI + 3.0, np.nextafter(HI, 0)]
        mask[1, h - 1, w - 3:] = [LO, HI, BIG]
        gt[0, :4, :5] = 1                                                  # touches two borders
        gt[0, h - 2:, w // 2:] = 200                                       # ... and the other two
        gt[1, 10, 20] = 255                                                # one pixel
        gt[1, 5:9, 25:33] = 3
        gt[1, 6, 27] = 0                                                   # a hole: its neighbours are boundary pixels
        special = np.array([[2, 12, 3, 20], [6, 16, 10, 30], [0, h, 0, w], [h - 3, h, w - 4, w], [3, 15, 7, 8], [9, 10, 2, 30], [4, 5, 4, 5],
                            [5, 5, 3, 9], [7, 3, 3, 9]], np.int32)
        clipped = scoring.box_rects(np.array([[w + 4.5, 3.2, w + 20.0, 9.9], [0.0, h - 2.5, 6.2, h + 7.0]]), h, w)
        assert clipped[0, 3] <= clipped[0, 2] and tuple(clipped[1]) == (h - 2, h, 0, 7)      # clipped to empty; clipped at the lower border
        rnd = np.zeros((260, 4), np.int32)
        rnd[:, 0] = rng.integers(0, h, 260)
        rnd[:, 1] = np.minimum(h, rnd[:, 0] + rng.integers(1, 6, 260))
        rnd[:, 2] = rng.integers(0, w, 260)
        rnd[:, 3] = np.minimum(w, rnd[:, 2] + rng.integers(1, 8, 260))
        rects = np.concatenate([special, clipped, rnd, [[0, h, 0, w], [1, h - 1, 1, w - 1]]]).astype(np.int32)
        scores = 1.5 * rng.standard_normal(len(rects))
        scores[:8] = [BIG, LO, HI, LO - 0.5, HI + 0.5, 0.0, 1.0, 7.0]
        scores[-2:] = [1.25, HI + 4.0]                                     # staged in the second LDS pass: the frame's border and the ring inside it
        assert len(rects) > 256 + 2
    off = np.array([0, 0, len(rects)], np.int32)
    for a in (frames, mask, gt, lut, rects, scores, off):
        a.setflags(write=False)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in dict(frames=frames, mask=mask, gt=gt, rects=rects, scores=scores).items()}
    _cases[h, w, c] = (dict(frames=frames, mask=mask, gt=gt, lut=lut, rects=rects, scores=scores, off=off), dev)
    return _cases[h, w, c]


def overlay_want(h, w, c, alpha, with_gt, bgr=True):
    key = ('want', h, w, c, alpha, with_gt, bgr)
    if key not in _cases:
        host, _ = overlay_case(h, w, c)
        want = R.overlay(host['frames'], host['mask'], host['rects'], host['scores'], host['off'], LO, HI, alpha,
                         gt=host['gt'] if with_gt else None, lut=host['lut'], bgr=bgr)
        want.setflags(write=False)
        _cases[key] = want
    return _cases[key]


def raw_overlay(dev, host, c, bgr, alpha, with_gt, lo=LO, hi=HI):
    from vec_vad_amd import _lib
    n, h, w = host['mask'].shape
    out = torch.full((n + 1, h, w, 3), SENT, dtype=torch.uint8, device='cuda')
    lut = torch.from_numpy(host['lut'].copy()).cuda()
    off = torch.from_numpy(host['off'].copy()).cuda()
    rc = _lib.lib().vv_render_overlay(dev['frames'].data_ptr(), c, bgr, dev['mask'].data_ptr(), dev['gt'].data_ptr() if with_gt else None,
                                      dev['rects'].data_ptr(), dev['scores'].data_ptr(), off.data_ptr(), len(host['rects']), lut.data_ptr(),
                                      lo, hi, alpha, n, h, w, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == OK, rc
    torch.cuda.synchronize()
    assert bool((out[-1] == SENT).all())
    return out[:-1]


@pytest.mark.parametrize('with_gt', [False, True], ids=['no-gt', 'gt'])
@pytest.mark.parametrize('alpha', [0, 128, 256])
@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('h,w', [(19, 37), (1, 1)], ids=['19x37', '1x1'])
def test_overlay_and_the_raw_abi_equal_the_restatement(h, w, c, alpha, with_gt):
    from vec_vad_amd import render
    host, dev = overlay_case(h, w, c)
    want = torch.from_numpy(overlay_want(h, w, c, alpha, with_gt).copy())
    got = render.overlay(dev['frames'], dev['mask'], dev['rects'], dev['scores'], host['off'], LO, HI, alpha,
                         gt=dev['gt'] if with_gt else None, lut=host['lut'])
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, h, w, 3) and got.is_cuda
    print('%d x %d, c %d, alpha %d, gt %s: %d of %d bytes differ from the restatement' % (h, w, c, alpha, with_gt, int((got.cpu() != want).sum()),
                                                                                        want.numel()))
    assert torch.equal(got.cpu(), want)
    assert torch.equal(raw_overlay(dev, host, c, 1, alpha, with_gt), got)
    for k in ('frames', 'mask', 'gt', 'rects', 'scores'):                  # no input is written
        assert torch.equal(dev[k].cpu(), torch.from_numpy(host[k].copy())), k
    if alpha == 0 and not with_gt and h > 1:                               # frame 0 has no box: alpha 0 returns the frame
        base = host['frames'][0] if c == 1 else host['frames'][0][..., ::-1]
        assert np.array_equal(got[0].cpu().numpy(), np.broadcast_to(base, (h, w, 3)))
    if c == 1:                                                             # [n,h,w] is [n,h,w,1]
        assert torch.equal(render.overlay(dev['frames'][..., 0], dev['mask'], dev['rects'], dev['scores'], host['off'], LO, HI, alpha,
                                          gt=dev['gt'] if with_gt else None, lut=host['lut']), got)


def test_overlay_channel_order_no_boxes_and_default_table():
    from vec_vad_amd import render
    h, w = 19, 37
    host, dev = overlay_case(h, w, 3)
    rgb = render.overlay(dev['frames'], dev['mask'], dev['rects'], dev['scores'], host['off'], LO, HI, 128, lut=host['lut'], bgr=False)
    assert torch.equal(rgb.cpu(), torch.from_numpy(overlay_want(h, w, 3, 128, False, bgr=False).copy()))
    assert torch.equal(raw_overlay(dev, host, 3, 0, 128, False), rgb)
    assert not torch.equal(rgb, render.overlay(dev['frames'], dev['mask'], dev['rects'], dev['scores'], host['off'], LO, HI, 128, lut=host['lut']))
    # zero boxes: empty tensors, and an offset table that names none of the boxes given
    none = R.overlay(host['frames'], host['mask'], np.zeros((0, 4), np.int32), np.zeros(0), [0, 0, 0], LO, HI, 77, gt=host['gt'],
                     lut=render.colormap())
    for rects, scores in ((np.zeros((0, 4), np.int32), np.zeros(0)), (dev['rects'], dev['scores'])):
        got = render.overlay(dev['frames'], dev['mask'], rects, scores, [0, 0, 0], LO, HI, 77, gt=dev['gt'])      # lut=None: colormap()
        assert torch.equal(got.cpu(), torch.from_numpy(none))
    # the second frame alone, which owns all the boxes
    one = render.overlay(dev['frames'][1:], dev['mask'][1:], dev['rects'], dev['scores'], [0, len(host['rects'])], LO, HI, 128, lut=host['lut'])
    assert torch.equal(one[0].cpu(), torch.from_numpy(overlay_want(h, w, 3, 128, False)[1].copy()))
    assert tuple(render.overlay(dev['frames'][:0], dev['mask'][:0], dev['rects'], dev['scores'], [0], LO, HI, 128).shape) == (0, h, w, 3)


def test_overlay_refusals_return_the_codes_stated_and_write_nothing():
    from vec_vad_amd import _lib, render
    l = _lib.lib()
    h, w = 19, 37
    host, dev = overlay_case(h, w, 3)
    out = torch.full((2, h, w, 3), SENT, dtype=torch.uint8, device='cuda')
    lut = torch.from_numpy(host['lut'].copy()).cuda()
    off = torch.from_numpy(host['off'].copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    P = dict(frames=dev['frames'].data_ptr(), c=3, bgr=1, mask=dev['mask'].data_ptr(), gt=dev['gt'].data_ptr(), rects=dev['rects'].data_ptr(),
             scores=dev['scores'].data_ptr(), off=off.data_ptr(), m=len(host['rects']), lut=lut.data_ptr(), lo=LO, hi=HI, alpha=128, n=2, h=h, w=w,
             out=out.data_ptr())

    def call(**kw):
        a = dict(P)
        a.update(kw)
        return l.vv_render_overlay(a['frames'], a['c'], a['bgr'], a['mask'], a['gt'], a['rects'], a['scores'], a['off'], a['m'], a['lut'], a['lo'],
                                   a['hi'], a['alpha'], a['n'], a['h'], a['w'], a['out'], st)

    for kw in (dict(frames=None), dict(mask=None), dict(lut=None), dict(out=None), dict(rects=None), dict(scores=None), dict(off=None),
               dict(rects=P['rects'] + 4), dict(c=2), dict(c=0), dict(c=4), dict(alpha=-1), dict(alpha=257), dict(hi=LO), dict(hi=LO - 1.0),
               dict(hi=float('nan')), dict(lo=float('nan')), dict(n=-1), dict(h=-1), dict(w=-1), dict(m=-1), dict(h=65536, w=32768)):
        assert call(**kw) == BAD_ARG, kw
    assert call(n=0, frames=None, mask=None, out=None, lut=None) == OK and call(h=0, frames=None, mask=None, out=None) == OK and call(w=0) == OK
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert call(m=0, rects=None, scores=None, off=None, gt=None) == OK     # zero boxes: the three tables are not looked at
    torch.cuda.synchronize()
    assert torch.equal(out, render.overlay(dev['frames'], dev['mask'], [], [], [0, 0, 0], LO, HI, 128, lut=host['lut']))
    a = dict(frames=dev['frames'], mask=dev['mask'], rects=dev['rects'], scores=dev['scores'], frame_off=host['off'], lo=LO, hi=HI, alpha=128)
    for kw, text in ((dict(hi=LO), 'the range must have lo < hi'), (dict(alpha=300), 'alpha must be an integer in 0..256, got 300'),
                     (dict(alpha=1.5), 'alpha must be an integer'), (dict(frames=dev['frames'].float()), 'frames must be a uint8'),
                     (dict(frames=dev['frames'][..., :2]), 'with c in .1, 3., got'), (dict(mask=dev['mask'].float()), 'mask must be a float64'),
                     (dict(mask=dev['mask'][:1]), 'mask must be a float64 .2,19,37. tensor'), (dict(mask=dev['mask'].cpu()), 'mask must be a float64'),
                     (dict(gt=dev['gt'][:, :5]), 'gt must be a uint8 .2,19,37. tensor'), (dict(gt=dev['gt'].bool()), 'gt must be a uint8'),
                     (dict(lut=np.zeros((256, 3))), 'lut must be a uint8 .256,3. table'), (dict(lut=np.zeros((255, 3), np.uint8)), 'lut must be'),
                     (dict(rects=dev['rects'][:5]), 'rectangle entries for'), (dict(frame_off=[0, 1]), 'frame_off must be 3 non-decreasing offsets'),
                     (dict(frame_off=[0, 5, 3]), 'frame_off must be'), (dict(frame_off=[0, 0, 10 ** 6]), 'frame_off must be')):
        b = dict(a)
        b.update(kw)
        with pytest.raises(ValueError, match=text) as e:
            render.overlay(**b)
        assert '\n' not in str(e.value)
    with pytest.raises(_lib.VecVadHipError, match='device-resident'):
        render.overlay(**dict(a, frames=dev['frames'].cpu()))


# ---- script level -------------------------------------------------------------------------------------------------------------------
TEST_VIDEOS = (7, 5)
N_TEST = sum(TEST_VIDEOS)
RES = 'results/UCSDped2/'
TAIL = 'obj_det_with_motion_SelfComplete'
H, W = 240, 360


def _tree():
    return sorted(os.path.relpath(os.path.join(d, f), 'results') for d, _, files in os.walk('results') for f in files)


def _content(path):
    """What a file holds: its bytes; for an .npz the bytes of every member (the archive itself carries the time it was written)."""
    if path.endswith('.npz'):
        with zipfile.ZipFile(path) as z:
            return {n: z.read(n) for n in z.namelist()}
    return open(path, 'rb').read()


def _others():
    return {p: _content(os.path.join('results', p)) for p in _tree() if not p.startswith('UCSDped2/render/')}


def _pngs(frames=range(N_TEST)):
    from PIL import Image
    assert sorted(os.listdir(RES + 'render')) == sorted('%d.png' % f for f in frames)
    return {f: np.array(Image.open(RES + 'render/%d.png' % f)) for f in frames}


def _clear():
    for p in glob.glob(RES + '*.np?') + glob.glob(RES + 'score_mask*/*') + glob.glob(RES + 'render/*'):
        os.remove(p)
    for d in glob.glob(RES + 'score_mask*') + glob.glob(RES + 'render'):
        os.rmdir(d)


def _direct(text, parts=False):
    text = text.replace('direct_test = False', 'direct_test = True').replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 5')
    return text.replace('direct_max_cubes = 524288', 'direct_max_cubes = 3') if parts else text


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    """The synthetic tree, trained once; one cube per launch on every route, so that a part of 3 cubes launches the shapes the whole set
    does and the cube scores are equal bit for bit between the routes (as in tests/test_gpu_smooth.py)."""
    import train as T
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from synthetic_tree import make_tree
    root = tmp_path_factory.mktemp('pictures')
    back = os.getcwd()
    os.chdir(root)
    try:
        make_tree({'train': (4, 3), 'test': TEST_VIDEOS}, 3)
        cfg = small_config().replace('score_batch = 2048', 'score_batch = 1')
        assert all(k in cfg for k in ('render = False', 'render_source = score', 'render_every = 1', 'render_flow = False', 'render_boxes = True',
                                      'render_alpha = 50', 'render_range = auto', 'render_flow_max = 0', 'save_score_masks = True'))
        T.main('config.cfg')
        before = set(_tree())
    finally:
        os.chdir(back)
    return dict(root=str(root), cfg=cfg, before=before)


@pytest.fixture
def recorded(monkeypatch):
    """Every ``render.overlay`` / ``render.flow_color`` call of a run: (arguments on the host, result on the host)."""
    from vec_vad_amd import render
    calls = dict(overlay=[], flow=[])
    overlay, flow_color = render.overlay, render.flow_color

    def host(v):
        return v.cpu().numpy() if torch.is_tensor(v) else v

    def rec_overlay(frames, mask, rects, scores, frame_off, lo, hi, alpha, gt=None, lut=None, bgr=True):
        out = overlay(frames, mask, rects, scores, frame_off, lo, hi, alpha, gt=gt, lut=lut, bgr=bgr)
        calls['overlay'].append((dict(frames=host(frames), mask=host(mask), rects=host(rects), scores=host(scores), off=np.asarray(host(frame_off)),
                                      lo=lo, hi=hi, alpha=alpha, gt=host(gt), lut=host(lut), bgr=bgr), host(out)))
        return out

    def rec_flow(flow, maxrad=0.0):
        out = flow_color(flow, maxrad)
        calls['flow'].append((host(flow), maxrad, host(out)))
        return out

    monkeypatch.setattr(render, 'overlay', rec_overlay)
    monkeypatch.setattr(render, 'flow_color', rec_flow)
    return calls


def _frames_of(calls, chunk=64, every=1):
    """frame -> (call, row) for the overlay calls of a run in chunks of ``chunk`` frames."""
    where, k = {}, 0
    for a in range(0, N_TEST, chunk):
        sel = [f for f in range(a, min(a + chunk, N_TEST)) if f % every == 0]
        if sel:
            for row, f in enumerate(sel):
                where[f] = (calls[k], row)
            k += 1
    assert k == len(calls)
    return where


def test_main_render_off_and_on_staged_direct_and_in_parts(tree, recorded, monkeypatch, capsys):
    import train as T
    import test as S
    from PIL import Image
    from vec_vad_amd import render
    monkeypatch.chdir(tree['root'])
    cfg = tree['cfg']
    names = ['frame_scores_%s.npy' % TAIL, 'raw2flow_%s_frame_results.npz' % TAIL] + ['score_mask/%d' % f for f in range(N_TEST)]
    pngs = ['render/%d.png' % f for f in range(N_TEST)]

    def written(*lists):
        return sorted(tree['before'] | {'UCSDped2/' + p for l in lists for p in l})

    # ---- key off: the files and the lines of a run before the key existed, and nothing of the render module is called
    open('config.cfg', 'w').write(cfg)
    S.main('config.cfg')
    off_out = capsys.readouterr().out
    assert 'ender' not in off_out and _tree() == written(names) and not recorded['overlay'] and not recorded['flow']
    base = _others()
    fs = np.load(RES + names[0])
    masks = np.stack([torch.load(RES + 'score_mask/%d' % f, weights_only=False) for f in range(N_TEST)])
    grey = np.stack([np.array(Image.open(p)) for p in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test0??/*.tif'))])
    gts = np.stack([np.array(Image.open(p).convert('L')) for p in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test*_gt/*.bmp'))])
    assert masks.shape == grey.shape == gts.shape == (N_TEST, H, W) and gts.any()

    # ---- key on, staged route: one picture per frame, every other file as before
    on = cfg.replace('render = False', 'render = True')
    _clear()
    open('config.cfg', 'w').write(on)
    assert T.read_config('config.cfg')['render']
    S.main('config.cfg')
    out = capsys.readouterr().out
    assert out.replace('Rendered %d frames to results/UCSDped2/render\n' % N_TEST, '') == off_out
    assert _tree() == written(names, pngs)
    assert _others() == base
    staged = _pngs()
    (args, res), = recorded['overlay']                                      # one chunk of 64 holds the 12 frames
    assert not recorded['flow'] and res.shape == (N_TEST, H, W, 3)
    for f in range(N_TEST):
        assert staged[f].dtype == np.uint8 and np.array_equal(staged[f], res[f]), f
    # what the stage handed to render.overlay: the decoded frames (BGR), the values of the score_mask files, the ground truth, the range
    assert args['bgr'] and np.array_equal(args['frames'], np.repeat(grey[..., None], 3, axis=3))
    assert args['mask'].dtype == np.float64 and np.array_equal(args['mask'], masks)
    assert np.array_equal(args['gt'], gts) and args['alpha'] == 128 and np.array_equal(args['lut'], render.colormap())
    sc = args['scores']
    assert len(sc) == args['off'][-1] > N_TEST and args['off'][0] == 0 and (args['lo'], args['hi']) == (sc[np.abs(sc) < BIG].min(), sc[np.abs(sc) < BIG].max())
    assert np.array_equal(masks.reshape(N_TEST, -1).max(axis=1), fs)
    for f in (0, 5, 11):                                                    # the rectangles and scores paint the mask files; the picture is the restatement's
        sl = slice(args['off'][f], args['off'][f + 1])
        painted = np.full((H, W), -BIG)
        for (y0, y1, x0, x1), s in zip(args['rects'][sl], sc[sl]):
            painted[y0:y1, x0:x1] = np.maximum(painted[y0:y1, x0:x1], s)
        assert np.array_equal(painted, masks[f])
        want = R.overlay(args['frames'][f:f + 1], masks[f:f + 1], args['rects'][sl], sc[sl], [0, sl.stop - sl.start], args['lo'], args['hi'], 128,
                         gt=gts[f:f + 1], lut=args['lut'])
        assert np.array_equal(staged[f], want[0]), f
    assert (staged[1][gts[1] != 0] == 255).any() and not np.array_equal(staged[0], np.repeat(grey[0][..., None], 3, axis=2))

    # ---- the direct route and the direct route in parts: the same pictures, and the same other files but for the cube files
    for route, text in (('direct', _direct(on)), ('parts', _direct(on, parts=True))):
        _clear()
        del recorded['overlay'][:]
        open('config.cfg', 'w').write(text)
        c = T.read_config('config.cfg')
        assert c['render'] and c['direct_test'] and c['direct_max_cubes'] == (3 if route == 'parts' else 524288)
        S.main('config.cfg')
        capsys.readouterr()
        assert len(recorded['overlay']) == 3                               # chunks of 5 frames
        got = _pngs()
        for f in range(N_TEST):
            assert np.array_equal(got[f], staged[f]), (route, f)
        assert _others() == base, route

    # ---- render_every = 3, no boxes, another range and weight
    _clear()
    del recorded['overlay'][:]
    open('config.cfg', 'w').write(_direct(on).replace('render_every = 1', 'render_every = 3'))
    S.main('config.cfg')
    assert 'Rendered 4 frames' in capsys.readouterr().out
    third = _pngs(range(0, N_TEST, 3))
    assert all(np.array_equal(third[f], staged[f]) for f in third)
    assert [len(a['frames']) for a, _ in recorded['overlay']] == [2, 2]     # frames 0, 3 | 6, 9 | none of 10, 11: only the picked frames are decoded
    _clear()
    del recorded['overlay'][:]
    open('config.cfg', 'w').write(on.replace('render_boxes = True', 'render_boxes = False').replace('render_range = auto', 'render_range = -1,0.5')
                                  .replace('render_alpha = 50', 'render_alpha = 100').replace('render_every = 1', 'render_every = 5'))
    S.main('config.cfg')
    capsys.readouterr()
    plain = _pngs(range(0, N_TEST, 5))
    (args, _), = recorded['overlay']
    assert len(args['scores']) == 0 and (args['lo'], args['hi'], args['alpha']) == (-1.0, 0.5, 256) and args['off'].tolist() == [0, 0, 0, 0]
    for k, f in enumerate(range(0, N_TEST, 5)):
        want = R.overlay(args['frames'][k:k + 1], masks[f:f + 1], np.zeros((0, 4), np.int32), np.zeros(0), [0, 0], -1.0, 0.5, 256, gt=gts[f:f + 1],
                         lut=args['lut'])
        assert np.array_equal(plain[f], want[0]), f


def test_main_render_smooth_source_and_flow_panel(tree, request, monkeypatch, capsys):
    import test as S
    from vec_vad_amd.render import flow_color          # the function itself, before the recorder wraps the module's attribute
    recorded = request.getfixturevalue('recorded')
    monkeypatch.chdir(tree['root'])
    on = tree['cfg'].replace('render = False', 'render = True')
    # ---- render_source = smooth: the values of the score_mask_smooth files, with chunks of 5 frames (the temporal halo crosses them)
    _clear()
    open('config.cfg', 'w').write(_direct(on).replace('render_source = score', 'render_source = smooth').replace('smooth_masks = False', 'smooth_masks = True'))
    S.main('config.cfg')
    capsys.readouterr()
    smoothed = np.stack([torch.load(RES + 'score_mask_smooth/%d' % f, weights_only=False) for f in range(N_TEST)])
    plain = np.stack([torch.load(RES + 'score_mask/%d' % f, weights_only=False) for f in range(N_TEST)])
    assert not np.array_equal(smoothed, plain)
    where = _frames_of(recorded['overlay'], chunk=5)
    got = _pngs()
    ranges = set()
    for f in range(N_TEST):
        (args, res), row = where[f]
        assert np.array_equal(args['mask'][row], smoothed[f]) and np.array_equal(got[f], res[row]), f
        ranges.add((args['lo'], args['hi']))
    sc = np.concatenate([a['scores'] for a, _ in recorded['overlay']])
    assert ranges == {(sc[np.abs(sc) < BIG].min(), sc[np.abs(sc) < BIG].max())}      # the range of the cube scores, for this source too

    # ---- render_flow on the flow files: the picture, then the colour image of the frame's flow file
    score_pngs = None
    for text in (on, _direct(on)):
        _clear()
        del recorded['overlay'][:], recorded['flow'][:]
        open('config.cfg', 'w').write(text.replace('render_flow = False', 'render_flow = True').replace('render_every = 1', 'render_every = 4'))
        S.main('config.cfg')
        capsys.readouterr()
        got = _pngs(range(0, N_TEST, 4))
        where = _frames_of(recorded['overlay'], chunk=5 if 'direct_test = True' in text else 64, every=4)
        flows = {f: np.load(p) for f, p in enumerate(sorted(glob.glob('optical_flow/UCSDped2/Test/Test0??/*.npy')))}
        assert [m for _, m, _ in recorded['flow']] == [0.0] * len(recorded['overlay'])      # one call per chunk, render_flow_max as maxrad
        for f in range(0, N_TEST, 4):
            (args, res), row = where[f]
            assert got[f].shape == (H, 2 * W, 3) and np.array_equal(got[f][:, :W], res[row])
            assert np.array_equal(got[f][:, W:], flow_color(torch.from_numpy(flows[f]).cuda()).cpu().numpy())      # an image is coloured on its own
            img, rad, _ = R.flow_parts(flows[f])
            band = np.abs(rad - 1) < 1e-5
            assert band.sum() <= 2 and (np.abs(got[f][:, W:].astype(int) - img.astype(int)).max(axis=2)[~band] <= 1).all()
        if score_pngs is None:
            score_pngs = got
        else:
            assert all(np.array_equal(got[f], score_pngs[f]) for f in got)


@pytest.fixture(scope='module')
def net():
    from FlowNet2_src import FlowNet2
    torch.manual_seed(0)
    return FlowNet2().cuda().eval()


def test_main_render_flow_recomputed_equals_the_flow_files(tree, net, monkeypatch, capsys):
    """``render_flow`` with ``direct_flow`` at one pair per launch against the panel made from the flow files that
    ``calc_optical_flow(pairs_per_launch=1)`` wrote with the same network."""
    import shutil
    import calc_optical_flow as COF
    import test as S
    from vad_datasets import unified_dataset_interface
    monkeypatch.chdir(tree['root'])
    keep = 'flow_kept/Test'                                                 # the synthetic flow files come back afterwards
    shutil.copytree('optical_flow/UCSDped2/Test', keep)
    try:
        ds = unified_dataset_interface('UCSDped2', os.path.join('raw_datasets', 'UCSDped2'), context_frame_num=1, mode='test', border_mode='hard')
        COF.calc_optical_flow(ds, flownet2=net, log=lambda *a: None, pairs_per_launch=1)
        on = _direct(tree['cfg']).replace('render = False', 'render = True').replace('render_flow = False', 'render_flow = True')
        on = on.replace('render_every = 1', 'render_every = 3').replace('render_flow_max = 0', 'render_flow_max = 3.5')
        _clear()
        open('config.cfg', 'w').write(on)
        S.main('config.cfg')
        files = _pngs(range(0, N_TEST, 3))
        _clear()
        open('config.cfg', 'w').write(on.replace('direct_flow = False', 'direct_flow = True').replace('direct_flow_pairs = 4', 'direct_flow_pairs = 1'))
        shutil.move('optical_flow/UCSDped2/Test', 'flow_kept/Test.net')      # nothing under it is read now
        S.main('config.cfg', flownet2=net)
        capsys.readouterr()
        direct = _pngs(range(0, N_TEST, 3))
        for f in files:
            assert files[f].shape == (H, 2 * W, 3) and np.array_equal(direct[f], files[f]), f
        assert len({files[f][:, W:].tobytes() for f in files}) == len(files)      # the panels show flows, each its own
    finally:
        for d in ('optical_flow/UCSDped2/Test', 'flow_kept/Test.net'):
            if os.path.isdir(d):
                shutil.rmtree(d)
        shutil.move(keep, 'optical_flow/UCSDped2/Test')
