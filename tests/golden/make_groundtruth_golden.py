"""Generate tests/golden/groundtruth_pinned.npz FROM THE REFERENCE (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_groundtruth_golden.py

The reference's own maggie/dataloader/utils.py (gen_transition_gt, gen_diff_mask) is loaded from its file with a stand-in `cv2`:
getStructuringElement is oracle.region.ellipse_kernel, dilate / erode are the definition-level filters of tests/groundtruth_restatement.py
(OpenCV is not installed here). What this pins is therefore the reference's torch glue -- shapes, stacking order, the `masks` branch, the
dtype of the instance sum -- not OpenCV; the filters themselves are checked against scipy.ndimage in tests/test_groundtruth_cpu.py.

The datasets' statements around those two functions (him.py:157-196, vim.py:160-211) are the restated glue of groundtruth_restatement.py,
run here with the reference's functions in place of the restated ones, on the seeded inputs of `golden_inputs` (regenerated, not stored).

Stored: 'train' (him.py training item, with masks), 'diff' (vim.py training item) as packed bits with their shapes; 'eval' (trimap) as uint8;
'gen_transition_gt.dtype' / 'gen_diff_mask.dtype': what the reference's functions return."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import groundtruth_restatement as R                            # noqa: E402
from oracle import ref_loader                                  # noqa: E402
from oracle.region import ellipse_kernel                       # noqa: E402


def load_reference_utils():
    cv2 = types.ModuleType('cv2')
    cv2.MORPH_ELLIPSE = 2

    def get_structuring_element(shape, ksize):
        assert shape == cv2.MORPH_ELLIPSE and ksize[0] == ksize[1]
        return ellipse_kernel(int(ksize[0]))

    cv2.getStructuringElement = get_structuring_element
    cv2.dilate = lambda src, kernel, iterations=1: R.dilate(src, np.asarray(kernel), iterations)
    cv2.erode = lambda src, kernel, iterations=1: R.erode(src, np.asarray(kernel), iterations)
    saved = sys.modules.get('cv2')
    sys.modules['cv2'] = cv2
    try:
        spec = importlib.util.spec_from_file_location('_ref_dataloader_utils', os.path.join(ref_loader.REF_ROOT, 'maggie', 'dataloader', 'utils.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if saved is None:
            del sys.modules['cv2']
        else:
            sys.modules['cv2'] = saved
    return mod


def main():
    U = load_reference_utils()
    seen = {}

    def ref_transition(*a, **kw):
        r = U.gen_transition_gt(*a, **kw)
        seen['gen_transition_gt.dtype'] = str(r.dtype)
        return r

    def ref_diff(*a, **kw):
        r = U.gen_diff_mask(*a, **kw)
        seen['gen_diff_mask.dtype'] = str(r.dtype)
        return r

    R.gen_transition_gt, R.gen_diff_mask = ref_transition, ref_diff          # the restated glue now runs the reference's functions
    out = {}
    c = R.GOLDEN['train']
    alpha, mask = R.golden_inputs('train')
    t = R.him_train_item(alpha, mask, c['chosen_ids'], c['max_inst'], c['k_size'], c['iterations']).numpy()
    assert set(np.unique(t)) <= {0.0, 1.0} and t.dtype == np.float32
    out['train'], out['train.shape'] = np.packbits(t.astype(bool)), np.asarray(t.shape)
    tri = R.eval_item(R.golden_inputs('eval')).numpy()
    assert set(np.unique(tri)) <= {0.0, 1.0, 2.0} and tri.dtype == np.float32
    out['eval'] = tri.astype(np.uint8)
    c = R.GOLDEN['diff']
    d = R.vim_train_item(R.golden_inputs('diff'), c['chosen_ids'], c['max_inst'], c['k_size'], c['iterations']).numpy()
    assert set(np.unique(d)) <= {0.0, 1.0} and d.dtype == np.float32
    out['diff'], out['diff.shape'] = np.packbits(d.astype(bool)), np.asarray(d.shape)
    for k, v in seen.items():
        out[k] = np.asarray(v)
    path = os.path.join(HERE, 'groundtruth_pinned.npz')
    np.savez_compressed(path, **out)
    print('wrote groundtruth_pinned.npz', os.path.getsize(path), 'bytes', {k: (v.shape, str(v.dtype)) for k, v in out.items()}, seen)


if __name__ == '__main__':
    main()
