"""Writes tests/golden/flow_color.npz: float32 flow fields, the uint8 images the reference's ``flowlib.flow_to_image`` makes of them and
the reference's colour wheel.  CPU only; run once, with the directory of the reference checkout that holds ``flowlib.py``:

    python tests/golden/make_flow_color_golden.py <reference dir>

``flowlib`` imports the ``png`` module, which it does not need for this and which may be absent: an empty stub stands in for it.  Only
the ``.npz`` is read by the tests.

Fields (float32): ``flow_a`` [24,40,2] and ``flow_b`` [48,64,2] -- smooth fields plus noise with one pixel of the largest radius, one
pixel at exactly (0, 0) (``pos_zero``), the pair (2.5, +0.0) / (2.5, -0.0) on either side of the cut of the wheel (``pos_plus`` /
``pos_minus``) and one unknown pixel (1e9, 0) (``pos_unknown``); ``flow_zero`` [24,40,2], all zero; ``flow_batch`` [3,24,40,2], three
fields with different maxima.  ``img_*``: the reference's image of each; ``wheel`` [55,3]: its colour wheel."""
import os
import sys
import types

import numpy as np

POS = dict(pos_zero=(3, 5), pos_plus=(10, 7), pos_minus=(10, 8), pos_unknown=(17, 30), pos_max=(20, 11))


def field(h, w, seed, scale):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u = scale * (np.cos(x / 7.0) + 0.5 * np.sin(y / 5.0)) + 0.3 * rng.standard_normal((h, w))
    v = scale * (np.sin(x / 9.0 + y / 11.0) - 0.25) + 0.3 * rng.standard_normal((h, w))
    fl = np.stack([u, v], axis=2).astype(np.float32)
    fl[POS['pos_zero']] = (0.0, 0.0)
    fl[POS['pos_plus']] = (2.5, 0.0)
    fl[POS['pos_minus']] = (2.5, -0.0)
    fl[POS['pos_max']] = (-1.75 * scale - 2.0, 2.5 * scale + 1.0)      # beyond every other radius: the one maximum
    return fl


def main(ref_dir):
    sys.modules.setdefault('png', types.ModuleType('png'))
    sys.path.insert(0, ref_dir)
    import flowlib

    a, b = field(24, 40, 1, 3.0), field(48, 64, 2, 5.0)
    for fl in (a, b):
        fl[POS['pos_unknown']] = (1e9, 0.0)
    batch = np.stack([field(24, 40, 10 + k, s) for k, s in enumerate((1.0, 4.0, 9.0))])
    flows = dict(flow_a=a, flow_b=b, flow_zero=np.zeros((24, 40, 2), np.float32), flow_batch=batch)
    out = {}
    for name, fl in flows.items():
        assert fl.dtype == np.float32 and not np.isnan(fl).any()
        one = fl if fl.ndim == 4 else fl[None]
        for f in one:                                        # the maximum radius is taken once
            known = (np.abs(f) <= 1e7).all(axis=2)
            r = np.where(known, np.sqrt((f.astype(np.float64) ** 2).sum(axis=2)), 0.0)
            assert name == 'flow_zero' or (r == r.max()).sum() == 1
        img = np.stack([flowlib.flow_to_image(f.copy()) for f in one])      # flow_to_image zeroes unknown pixels in place
        assert img.dtype == np.uint8
        out[name] = fl
        out['img' + name[4:]] = img if fl.ndim == 4 else img[0]
    assert (out['img_zero'] == 255).all()
    assert np.signbit(a[POS['pos_minus']][1]) and not np.signbit(a[POS['pos_plus']][1])
    out['wheel'] = np.asarray(flowlib.make_color_wheel(), np.float64)
    out.update({k: np.array(v, np.int32) for k, v in POS.items()})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'flow_color.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
