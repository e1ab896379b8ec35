"""Golden boxes of the 'simple_patch' foreground mode: runs the REAL reference ``fore_det/simple_patch.py:get_patch_loc`` (pure
numpy) for the three ``frame_size`` entries and the two grids of train.py:82 and stores the results as data.

    python tests/golden/make_simple_patch_golden.py <path of the reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
spec = importlib.util.spec_from_file_location('ref_simple_patch', os.path.join(sys.argv[1], 'fore_det', 'simple_patch.py'))
R = importlib.util.module_from_spec(spec)
spec.loader.exec_module(R)

out = {}
for name, (h, w) in (('UCSDped2', (240, 360)), ('avenue', (360, 640)), ('ShanghaiTech', (480, 856))):
    for h_num, w_num in ((3, 4), (6, 8)):
        out['%s_%dx%d' % (name, h_num, w_num)] = R.get_patch_loc(h, w, h_num, w_num)
np.savez(os.path.join(HERE, 'simple_patch_boxes.npz'), **out)
print({k: v.shape for k, v in out.items()})
