"""Spatio-temporal smoothing of score masks on the GPU ([mi355x] smooth_masks): ``scoring.smooth_masks`` and the raw ABI
(vv_smooth_masks) against the plain-numpy restatement (tests/smooth_restatement.py) on real-valued masks, then the script level
(``test.main`` staged, direct and direct in parts).  The summation order is part of the contract, so every comparison is exact:
``torch.equal`` / ``np.array_equal``, no tolerance anywhere."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from _util import small_config
import pixel_maps_restatement as PR
import smooth_restatement as R

pytestmark = pytest.mark.gpu

BIG = 100000.0
SIZES = [(37, 53), (5, 7), (1, 1)]            # no multiple of the 32 x 32 tile and more than one tile; narrower than a window of 9; one pixel
VIDEOS = [0, 0, 0, 1, 2, 2, 2, 2, 3]          # one-frame videos (3 and 8); with kt = 3 a video border lies inside every window around it
SENT = 3.0                                    # sentinel behind every output
GUARD = 4096                                  # guard bytes behind the work buffer


def _volume(h, w):
    """float64 [9,h,w], normal-distributed values in random boxes over -BIG.  Frame 1: nothing painted; 2: fully painted; 3: a one-frame
    video; 4: a +BIG box among the others; 5: ties (two boxes of one constant, one of which repeats a value of frame 4)."""
    rng = np.random.default_rng(1000 * h + w)
    m = np.full((len(VIDEOS), h, w), -BIG)
    for f in range(len(VIDEOS)):
        if f == 1:
            continue
        if f == 2:
            m[f] = rng.standard_normal((h, w))
            continue
        for _ in range(4):
            y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            y1, x1 = min(h, y0 + int(rng.integers(1, h // 2 + 2))), min(w, x0 + int(rng.integers(1, w // 2 + 2)))
            m[f, y0:y1, x0:x1] = np.maximum(m[f, y0:y1, x0:x1], rng.standard_normal((y1 - y0, x1 - x0)))
    m[4, h // 3:h // 3 + 3, w // 3:w // 3 + 4] = BIG
    m[5, :h // 2 + 1, :w // 3 + 1] = 0.625
    m[5, h // 2:, w // 2:] = 0.625
    return m


_cache = {}


def volume(h, w):
    """The volume of a size on the host (read-only) and on the device, built once."""
    if (h, w) not in _cache:
        m = _volume(h, w)
        m.setflags(write=False)
        _cache[h, w] = (m, torch.from_numpy(m.copy()).cuda())
    return _cache[h, w]


def reference(h, w, kt, ks):
    """The restatement of a volume and a pair of windows, computed once and left unchanged."""
    key = (h, w, kt, ks)
    if key not in _cache:
        S, fmax = R.smooth(volume(h, w)[0], VIDEOS, kt, ks)
        S.setflags(write=False)
        fmax.setflags(write=False)
        _cache[key] = (S, fmax)
    return _cache[key]


def raw_call(masks, vid, f0, f1, kt, ks, want_fmax=True):
    """vv_smooth_masks through ctypes with a work buffer of exactly the size the companion reports, guard bytes behind it and a sentinel
    frame / entry behind both outputs: (smoothed [f1-f0,h,w], fmax [f1-f0] | None), after checking that none of them was touched."""
    from vec_vad_amd import _lib
    l = _lib.lib()
    F, h, w = masks.shape
    nb = int(l.vv_smooth_masks_work(F, h, w, kt, ks))
    assert nb >= F * h * w * 10 and nb % 8 == 0
    work = torch.full((nb + GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.full((f1 - f0 + 1, h, w), SENT, dtype=torch.float64, device='cuda')
    fmax = torch.full((f1 - f0 + 1,), SENT, dtype=torch.float64, device='cuda')
    vid = torch.tensor(list(vid), dtype=torch.int32, device='cuda')
    rc = l.vv_smooth_masks(masks.data_ptr(), vid.data_ptr(), F, h, w, f0, f1, kt, ks, out.data_ptr(), fmax.data_ptr() if want_fmax else None,
                           work.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((work[nb:] == 0xA5).all()), 'the kernels wrote behind the work buffer'
    assert bool((out[-1] == SENT).all()) and float(fmax[-1]) == SENT
    if not want_fmax:
        assert bool((fmax == SENT).all())
    return out[:-1], fmax[:-1] if want_fmax else None


@pytest.mark.parametrize('kt', [1, 3, 33])
@pytest.mark.parametrize('ks', [1, 3, 9, 33])
@pytest.mark.parametrize('h,w', SIZES, ids=['37x53', '5x7', '1x1'])
def test_smooth_masks_and_the_raw_abi_equal_the_restatement(h, w, ks, kt):
    from vec_vad_amd import scoring
    host, dev = volume(h, w)
    want, want_max = (torch.from_numpy(a.copy()) for a in reference(h, w, kt, ks))
    S, fmax = scoring.smooth_masks(dev, VIDEOS, kt, ks)
    assert S.dtype == fmax.dtype == torch.float64 and tuple(S.shape) == dev.shape and tuple(fmax.shape) == (len(VIDEOS),)
    differ = int((S.cpu() != want).sum())
    print('h x w %d x %d, windows (%d, %d): %d of %d values differ from the restatement' % (h, w, kt, ks, differ, want.numel()))
    assert torch.equal(S.cpu(), want) and torch.equal(fmax.cpu(), want_max)
    assert torch.equal(fmax, S.reshape(len(VIDEOS), -1).amax(dim=1))       # the maximum is exact
    assert torch.equal(S != -BIG, dev != -BIG)                             # the support is preserved
    assert float(fmax[1]) == -BIG                                          # a frame without a painted pixel
    assert bool((S[2] != -BIG).all())                                      # a fully painted frame stays fully painted
    assert torch.equal(dev.cpu(), torch.from_numpy(host.copy()))           # the input is not written
    if kt == ks == 1:
        assert torch.equal(S, dev)                                         # identity
    r_S, r_max = raw_call(dev, VIDEOS, 0, len(VIDEOS), kt, ks)
    assert torch.equal(r_S, S) and torch.equal(r_max, fmax)


def test_real_values_pin_the_order_and_big_boxes_flood():
    """The inputs are such that the order matters (another order gives other bits), and a +BIG box raises what its windows reach."""
    host, dev = volume(37, 53)
    want, _ = reference(37, 53, 3, 9)
    other = R.brute(host[6:8], [0, 0], 3, 9)
    mine, _ = R.smooth(host[6:8], [0, 0], 3, 9)
    assert not np.array_equal(other, mine) and np.abs(other - mine).max() < 1e-12
    box = np.zeros(host.shape, bool)
    box[4:8, max(0, 12 - 4):12 + 3 + 4, max(0, 17 - 4):17 + 4 + 4] = True   # windows (3, 9) around the box at rows 12..14, columns 17..20 of frame 4, video 2: frames 4, 5 reach it
    box[6:] = False
    painted = host != -BIG
    assert (painted & box).any() and (want[painted & box] > 100).all() and (want[painted & ~box] < 100).all()


def test_lo_hi_cut_the_halo_off_both_ends():
    from vec_vad_amd import scoring
    _, dev = volume(37, 53)
    for kt, ks in ((3, 9), (5, 3)):
        rt = kt // 2
        want, want_max = (torch.from_numpy(a.copy()).cuda() for a in reference(37, 53, kt, ks))
        full, full_max = scoring.smooth_masks(dev, VIDEOS, kt, ks)
        S, fmax = scoring.smooth_masks(dev, VIDEOS, kt, ks, lo=2, hi=7)      # the ends of the buffer serve as halo only
        assert tuple(S.shape) == (5, 37, 53) and torch.equal(S, full[2:7]) and torch.equal(fmax, full_max[2:7])
        a, b = 3, 6                                                        # a chunk with exactly its halo, as _smooth_stage cuts it
        out = torch.full((b - a, 37, 53), SENT, dtype=torch.float64, device='cuda')
        S, fmax = scoring.smooth_masks(dev[a - rt:b + rt], VIDEOS[a - rt:b + rt], kt, ks, lo=rt, hi=rt + b - a, out=out)
        assert S is out and torch.equal(S, want[a:b]) and torch.equal(fmax, want_max[a:b])
        r_S, r_max = raw_call(dev[a - rt:b + rt].contiguous(), VIDEOS[a - rt:b + rt], rt, rt + b - a, kt, ks)
        assert torch.equal(r_S, want[a:b]) and torch.equal(r_max, want_max[a:b])
        r_S, none = raw_call(dev, VIDEOS, 2, 7, kt, ks, want_fmax=False)    # fmax == NULL: the masks alone
        assert none is None and torch.equal(r_S, want[2:7])
        S, fmax = scoring.smooth_masks(dev, VIDEOS, kt, ks, lo=4, hi=4)      # nothing asked for
        assert tuple(S.shape) == (0, 37, 53) and tuple(fmax.shape) == (0,)


def test_one_frame_and_video_indices_of_any_integer_kind():
    from vec_vad_amd import scoring
    host, dev = volume(37, 53)
    for f in (0, 1, 4):
        want, want_max = R.smooth(host[f:f + 1], [7], 33, 9)
        S, fmax = scoring.smooth_masks(dev[f:f + 1], np.array([7], np.int64), 33, 9)
        assert np.array_equal(S.cpu().numpy(), want) and np.array_equal(fmax.cpu().numpy(), want_max)
    # the same videos under other names: only equality of the indices counts
    S, fmax = scoring.smooth_masks(dev, torch.tensor([5, 5, 5, -2, 9, 9, 9, 9, 0]), 3, 3)
    assert np.array_equal(S.cpu().numpy(), reference(37, 53, 3, 3)[0]) and np.array_equal(fmax.cpu().numpy(), reference(37, 53, 3, 3)[1])


def test_bad_arguments_and_no_ops_return_the_codes_stated():
    from vec_vad_amd import _lib
    l = _lib.lib()
    OK, BAD = 0, 1
    F, h, w = 4, 5, 7
    m = torch.full((F, h, w), 9.0, dtype=torch.float64, device='cuda')
    out = torch.full((F, h, w), 9.0, dtype=torch.float64, device='cuda')
    fm = torch.full((F,), 9.0, dtype=torch.float64, device='cuda')
    vid = torch.zeros(F, dtype=torch.int32, device='cuda')
    work = torch.full((int(l.vv_smooth_masks_work(F, h, w, 3, 3)),), 9, dtype=torch.uint8, device='cuda')
    M, V, O, X, W, st = m.data_ptr(), vid.data_ptr(), out.data_ptr(), fm.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream

    def call(masks=M, v=V, F=F, h=h, w=w, f0=0, f1=F, kt=3, ks=3, o=O, x=X, wk=W):
        return l.vv_smooth_masks(masks, v, F, h, w, f0, f1, kt, ks, o, x, wk, st)

    for kw in (dict(masks=None), dict(v=None), dict(o=None), dict(wk=None),                  # NULL pointers (fmax alone may be NULL)
               dict(F=-1, f1=-1), dict(F=-1, f0=0, f1=0), dict(h=-5), dict(w=-7), dict(f0=-1),   # negative sizes
               dict(h=65536, w=32768), dict(h=46341, w=46341),                                  # h * w >= 2^31
               dict(f0=3, f1=2), dict(f1=F + 1), dict(f0=F + 1, f1=F + 1),                     # f0 > f1, f1 > F
               dict(kt=2), dict(ks=4), dict(kt=0), dict(ks=0), dict(kt=-3), dict(ks=-1), dict(kt=35), dict(ks=35), dict(kt=34), dict(ks=99)):
        assert call(**kw) == BAD, kw
    for kw in (dict(kt=2), dict(ks=0), dict(ks=35), dict(h=65536, w=32768), dict(F=-1), dict(h=-1), dict(w=-1)):
        a = dict(F=F, h=h, w=w, kt=3, ks=3)
        a.update(kw)
        assert l.vv_smooth_masks_work(a['F'], a['h'], a['w'], a['kt'], a['ks']) == -1, kw
    # nothing to do: F == 0 or f0 == f1, whatever the pointers
    assert call(F=0, f0=0, f1=0) == OK and call(masks=None, v=None, F=0, f0=0, f1=0, o=None, x=None, wk=None) == OK
    assert call(f0=2, f1=2) == OK and call(masks=None, v=None, f0=F, f1=F, o=None, x=None, wk=None) == OK
    assert l.vv_smooth_masks_work(0, h, w, 3, 3) == 0
    torch.cuda.synchronize()
    assert bool((m == 9.0).all()) and bool((out == 9.0).all()) and bool((fm == 9.0).all()) and bool((work == 9).all())   # nothing was launched
    # frames of no pixels: nothing to filter (NULL maps allowed), the maxima are the background
    assert call(masks=None, v=None, h=0, f0=1, f1=3, o=None, wk=None) == OK and call(masks=None, v=None, w=0, o=None, x=None, wk=None) == OK
    torch.cuda.synchronize()
    assert fm.tolist() == [-BIG, -BIG, 9.0, 9.0] and bool((out == 9.0).all())
    # the widest windows are taken
    assert call(kt=33, ks=33, wk=torch.empty(int(l.vv_smooth_masks_work(F, h, w, 33, 33)), dtype=torch.uint8, device='cuda').data_ptr()) == OK
    torch.cuda.synchronize()
    assert bool((out == 9.0).all()) and fm.tolist() == [9.0] * 4           # the mean of nines is nine: every partial sum of them is exact


def test_wrapper_refusals_are_one_line_value_errors():
    from vec_vad_amd import scoring, _lib
    m = torch.zeros((3, 4, 5), dtype=torch.float64, device='cuda')
    for kw, text in ((dict(smooth_frames=2), 'smooth_frames must be an odd integer in 1..33, got 2'),
                     (dict(smooth_pixels=35), 'smooth_pixels must be an odd integer in 1..33, got 35'),
                     (dict(smooth_pixels=0), 'smooth_pixels must be an odd integer'),
                     (dict(masks=m.float()), 'masks must be a float64 .F,h,w. tensor'),
                     (dict(masks=m[0]), 'masks must be a float64 .F,h,w. tensor'),
                     (dict(video_idx=[0, 0]), 'video_idx must name the video of each of the 3 frames'),
                     (dict(video_idx=[0.5, 0, 0]), 'video_idx must name the video'),
                     (dict(lo=2, hi=1), 'do not lie in the buffer of 3 frames'), (dict(hi=4), 'do not lie in the buffer'),
                     (dict(lo=-1), 'do not lie in the buffer'),
                     (dict(out=torch.zeros((3, 4, 5), device='cuda')), 'out must be a contiguous float64 .3,4,5. tensor'),
                     (dict(lo=1, out=torch.zeros((3, 4, 5), dtype=torch.float64, device='cuda')), 'out must be a contiguous float64 .2,4,5.')):
        a = dict(masks=m, video_idx=[0, 0, 0], smooth_frames=3, smooth_pixels=3)
        a.update(kw)
        with pytest.raises(ValueError, match=text) as e:
            scoring.smooth_masks(**a)
        assert '\n' not in str(e.value)
    with pytest.raises(_lib.VecVadHipError, match='device-resident'):
        scoring.smooth_masks(m.cpu(), [0, 0, 0], 3, 3)


# ---- script level -------------------------------------------------------------------------------------------------------------------
TEST_VIDEOS = (7, 5)
N_TEST = sum(TEST_VIDEOS)
RES = 'results/UCSDped2/'
TAIL = 'obj_det_with_motion_SelfComplete'


def _masks(d):
    assert sorted(os.listdir(d)) == sorted(str(f) for f in range(N_TEST))
    return [torch.load(os.path.join(d, str(f)), weights_only=False) for f in range(N_TEST)]


def _tree():
    return sorted(os.path.relpath(os.path.join(d, f), 'results') for d, _, files in os.walk('results') for f in files)


def _npz_equal(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True) for k in a)


def test_main_smooth_masks_staged_direct_and_in_parts(tmp_path, monkeypatch, capsys):
    import train as T
    import test as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    from synthetic_tree import make_tree
    monkeypatch.chdir(tmp_path)
    make_tree({'train': (4, 3), 'test': TEST_VIDEOS}, 3)                   # the first box of a frame fails the motion test: two are cut
    # one cube per launch on every route: a part of 3 cubes then launches the shapes the whole set does, so the cube scores -- and with
    # them every smoothed value -- are equal bit for bit between the routes (as in tests/test_gpu_regions.py)
    cfg = small_config().replace('score_batch = 2048', 'score_batch = 1').replace('pixel_criterion = False', 'pixel_criterion = True')
    assert 'save_score_masks = True' in cfg and 'smooth_masks = False' in cfg and 'smooth_frames = 5' in cfg and 'smooth_pixels = 9' in cfg
    open('config.cfg', 'w').write(cfg)
    names = ['frame_scores_%s.npy' % TAIL, 'pixel_scores_%s.npy' % TAIL]
    npzs = ['raw2flow_%s_frame_results.npz' % TAIL, 'raw2flow_%s_pixel_results.npz' % TAIL]
    s_names = ['frame_scores_smooth_%s.npy' % TAIL, 'pixel_scores_smooth_%s.npy' % TAIL]
    s_npzs = ['raw2flow_%s_frame_smooth_results.npz' % TAIL, 'raw2flow_%s_pixel_smooth_results.npz' % TAIL]
    mask_files = ['score_mask/%d' % f for f in range(N_TEST)]

    def clear():
        for p in glob.glob(RES + '*.np?') + glob.glob(RES + 'score_mask*/*'):
            os.remove(p)
        for d in glob.glob(RES + 'score_mask*'):
            os.rmdir(d)

    def unsmoothed():
        return ([open(RES + p, 'rb').read() for p in names], [dict(np.load(RES + p)) for p in npzs], _masks(RES + 'score_mask'))

    def same_unsmoothed(a, b):
        return a[0] == b[0] and all(_npz_equal(x, y) for x, y in zip(a[1], b[1])) and \
            all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[2], b[2]))

    def smoothed():
        return [np.load(RES + p) for p in s_names], [dict(np.load(RES + p)) for p in s_npzs], _masks(RES + 'score_mask_smooth')

    def direct(text, parts=False):
        text = text.replace('direct_test = False', 'direct_test = True').replace('direct_frames_per_chunk = 64', 'direct_frames_per_chunk = 5')
        return text.replace('direct_max_cubes = 524288', 'direct_max_cubes = 3') if parts else text

    T.main('config.cfg')
    before = set(_tree())                                                  # whatever training leaves under results/

    def written(*lists):
        return sorted(before | {'UCSDped2/' + p for l in lists for p in l})

    # ---- key off: the files of a run before the key existed, and no other
    S.main('config.cfg')
    off_out = capsys.readouterr().out
    assert 'smooth' not in off_out
    assert _tree() == written(names, npzs, mask_files)
    base = unsmoothed()
    fs, ps = np.load(RES + names[0]), np.load(RES + names[1])
    painted = np.stack(base[2])                                            # the host-painted score_mask files
    assert painted.shape == (N_TEST, 240, 360) and painted.dtype == np.float64
    video = np.repeat(np.arange(1, len(TEST_VIDEOS) + 1), TEST_VIDEOS)
    from PIL import Image
    gts = [np.array(Image.open(p).convert('L')) for p in sorted(glob.glob('raw_datasets/UCSDped2/Test/Test*_gt/*.bmp'))]
    assert len(gts) == N_TEST
    on = cfg.replace('smooth_masks = False', 'smooth_masks = True').replace('test_foreground_saved = False', 'test_foreground_saved = True')

    # ---- windows (1, 1): the smooth files hold the values of the unsmoothed ones
    clear()
    open('config.cfg', 'w').write(on.replace('smooth_frames = 5', 'smooth_frames = 1').replace('smooth_pixels = 9', 'smooth_pixels = 1'))
    c = T.read_config('config.cfg')
    assert c['smooth_masks'] and (c['smooth_frames'], c['smooth_pixels']) == (1, 1)
    S.main('config.cfg')
    printed = capsys.readouterr().out
    assert 'Frame-level AUC of the smoothed masks (1 frames x 1 x 1 pixels) is ' in printed
    assert 'Pixel-level AUC of the smoothed masks (overlap 40%) is ' in printed
    assert _tree() == written(names, npzs, mask_files, s_names, s_npzs, [m.replace('mask/', 'mask_smooth/') for m in mask_files])
    assert same_unsmoothed(unsmoothed(), base)
    (fs1, ps1), npz1, masks1 = smoothed()
    assert fs1.dtype == ps1.dtype == np.float64 and np.array_equal(fs1, fs) and np.array_equal(ps1, ps)
    assert all(type(a) is np.ndarray and a.dtype == np.float64 and a.flags['C_CONTIGUOUS'] and np.array_equal(a, b) for a, b in zip(masks1, base[2]))
    assert all(_npz_equal(a, b) for a, b in zip(npz1, base[1]))

    # ---- windows (5, 9): the restatement applied to the host-painted score_mask files
    want, want_max = R.smooth(painted, video, 5, 9)
    want_ps = np.array([PR.kth_largest(m, g, 40) for m, g in zip(want, gts)])
    assert not np.array_equal(want, painted) and not np.array_equal(want_max, fs)
    got = {}
    for route, text in (('staged', on), ('direct', direct(on)), ('parts', direct(on, parts=True))):
        clear()
        open('config.cfg', 'w').write(text)
        c = T.read_config('config.cfg')
        assert c['smooth_masks'] and (c['smooth_frames'], c['smooth_pixels']) == (5, 9) and c['direct_test'] == (route != 'staged')
        assert c['direct_max_cubes'] == (3 if route == 'parts' else 524288)
        S.main('config.cfg')
        assert 'Frame-level AUC of the smoothed masks (5 frames x 9 x 9 pixels) is ' in capsys.readouterr().out
        assert same_unsmoothed(unsmoothed(), base), route                  # every file written today is written as before
        got[route] = smoothed()
        (fs5, ps5), _, masks5 = got[route]
        print(route, 'smoothed frame scores minus the host reference:', fs5 - want_max)
        assert np.array_equal(fs5, want_max) and np.array_equal(ps5, want_ps), route
        assert all(a.dtype == np.float64 and a.shape == (240, 360) and np.array_equal(a, b) for a, b in zip(masks5, want)), route
    for p in glob.glob('data/raw2flow/*foreground_test*'):
        os.remove(p)
    for route in ('direct', 'parts'):                                      # the same files on every route
        assert all(_npz_equal(a, b) for a, b in zip(got['staged'][1], got[route][1])), route
    assert sorted(got['staged'][1][0]) == sorted(base[1][0])               # the layout of the unsmoothed result files

    # ---- scores_saved = True: the smoothed results come from the saved vectors, nothing is scored
    for p in s_npzs:
        os.remove(RES + p)
    open('config.cfg', 'w').write(on.replace('scores_saved = False', 'scores_saved = True'))

    def scored(*a, **k):
        raise AssertionError('scores_saved = True must not score')

    for name in ('score_frames', 'score_direct', '_smooth_stage'):
        monkeypatch.setattr(S, name, scored)
    S.main('config.cfg')
    assert all(_npz_equal(dict(np.load(RES + p)), a) for p, a in zip(s_npzs, got['staged'][1]))
