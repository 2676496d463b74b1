"""Generate tests/golden/conn_pinned.npz FROM THE REFERENCE (build container only; run it in its own interpreter, not after make_golden.py,
whose stand-ins set skimage.measure.label to None):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_conn_golden.py

The reference's own maggie/utils/metric.py (Conn) and maggie/utils/postprocessing.py (postprocess) run on the seeded inputs of
tests/conn_restatement.py (regenerated there, not stored). Stand-ins: cv2 is an empty module; skimage.measure.label is scipy.ndimage.label
with skimage's `connectivity` (1 -> cross, None / 2 -> 3x3 ones) and `return_num` (the same raster numbering). Conn's joblib pool runs
on threads: loky worker processes would re-import the module without the stand-ins.

Stored: 'conn.<case>' = [update() return, score, count, average()] and 'postprocess' = the post-processed planes."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import conn_restatement as R                                   # noqa: E402


def _label(image, background=None, return_num=False, connectivity=None):
    from scipy import ndimage
    st = ndimage.generate_binary_structure(2, 1) if connectivity == 1 else np.ones((3, 3), bool)
    lab, n = ndimage.label(np.asarray(image) != 0, structure=st)
    return (lab, n) if return_num else lab


def install_standins():
    sys.modules['cv2'] = types.ModuleType('cv2')
    sk = types.ModuleType('skimage')
    meas = types.ModuleType('skimage.measure')
    meas.label = _label
    sk.measure = meas
    sys.modules['skimage'] = sk
    sys.modules['skimage.measure'] = meas


def main():
    from oracle import ref_loader
    ref_loader.load_reference()                                # registers the reference's packages (and its own stand-ins for the model path)
    install_standins()                                         # metric.py / postprocessing.py bind these at import
    import importlib
    import joblib
    M = importlib.import_module('maggie.utils.metric')
    PP = importlib.import_module('maggie.utils.postprocessing')
    out = {}
    with joblib.parallel_backend('threading'):
        for key in R.CONN_CASES:
            pred, gt, tri = R.conn_inputs(key)
            for v in R.SPLIT_VALUES:                           # numpy 1 and numpy 2 threshold these planes alike
                assert not (pred == v).any() and not (gt == v).any(), key
            m = M.Conn()
            r = m.update(pred, gt, tri)
            out['conn.' + key] = np.asarray([r, m.score, m.count, m.average()], np.float64)
    alpha = R.postprocess_inputs()
    out['postprocess'] = np.asarray(PP.postprocess(alpha), np.float32)
    np.savez_compressed(os.path.join(HERE, 'conn_pinned.npz'), **out)
    print('wrote conn_pinned.npz', {k: (v.tolist() if v.size < 8 else v.shape) for k, v in out.items()})


if __name__ == '__main__':
    main()
