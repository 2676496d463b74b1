"""Generate tests/golden/affine_pinned.npz FROM THE REFERENCE (needs the reference's checkout beside this one, as make_crop_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_affine_golden.py

The reference's own `RandomAffine` (maggie/dataloader/transforms.py:926-963, with random_transform, apply_transforms_cv and channel_shift of
dataloader/utils.py) is loaded from its checkout with the stand-in `cv2` of tests/affine_restatement.py (geometry_restatement's plus warpAffine;
OpenCV is not a dependency of this project) and run through its `Compose` as him.py:49 / vim.py:55 wire it, on the seeded arrays of
`affine_restatement.GOLDEN` (regenerated, not stored) with the case's own `np.random.RandomState`. What this pins is the reference's draw order
and glue, not OpenCV: the skip draw, theta / shear / zoom / shear-form / intensity in that order, rotation . shear . zoom, the offset centre
with h and w swapped, the flipped matrix handed to cv2, linear for the 3-channel frames against nearest for the 2-D alphas, masks untouched, the
float64 channel shift clipped to each warped frame's own min / max.

The reference leaves the frames as float64 after the shift; the uint8 warp before it is recovered from the restatement and checked through
`clip(u8 + intensity, min, max) == reference frames` (with |intensity| < 8 and integer pixels, that equation has the one solution wherever the
clip is not active, and the restated warp is the reference's own call on the stand-in).

Stored per case: the uint8 warps of the frames and alphas (differences along the rows, `geometry_restatement.pack_rows`), `info` = (fired,
shear form, T, n), `intensity`, the per-frame `minmax`, the `matrix` handed to cv2 and a digest of the generator state afterwards. The
generator asserts that the restatement equals the reference, and that every property listed in WANTED is visible in the reference's outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import affine_restatement as A                                 # noqa: E402
import geometry_restatement as R                               # noqa: E402
import maskgen_restatement as M                                # noqa: E402
import make_maskgen_golden as MM                               # noqa: E402

WANTED = {'step skipped', 'shear form 0', 'shear form 1', 'clip T=3 n=2', 'masks untouched', 'alphas nearest, not linear', 'border corner 0',
          'clip active at the max', 'clip active at the min', 'h != w', 'fires at p = 0.1'}


def load_reference_transforms():
    saved = M.cv2_standin
    M.cv2_standin = A.cv2_standin                                          # the loader of make_maskgen_golden.py, over this stand-in
    try:
        sys.modules.pop('maggie.dataloader.utils', None)                   # random_transform lives there: bind it to THIS cv2 too
        return MM.load_reference_transforms()
    finally:
        M.cv2_standin = saved


def run_reference(T, name):
    c = A.GOLDEN[name]
    frames, alphas, masks = A.golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    sample = T.Compose([T.RandomAffine(rs, p=c['p'])])({'frames': frames.copy(), 'alphas': alphas.copy(), 'masks': masks.copy(), 'weights': None})
    return sample, rs


def main():
    T = load_reference_transforms()
    out, seen = {}, set()
    for name, c in A.GOLDEN.items():
        frames, alphas, masks = A.golden_inputs(name)
        ref, rs_ref = run_reference(T, name)
        mine, rs_mine = A.golden_run(name)
        assert np.array_equal(A.state_digest(rs_ref), A.state_digest(rs_mine)), '%s: the generator states differ' % name
        assert np.array_equal(ref['masks'], masks)
        seen.add('masks untouched')
        h, w = c['h'], c['w']
        assert (c['T'], c['n']) == (frames.shape[0], alphas.shape[0] // frames.shape[0])
        if not mine['fired']:
            assert ref['frames'].dtype == np.uint8 and np.array_equal(ref['frames'], frames) and np.array_equal(ref['alphas'], alphas)
            assert 'ignore_regions' not in ref
            hand = np.random.RandomState(c['rs_seed'])
            assert hand.rand() > c['p'] and np.array_equal(A.state_digest(hand), A.state_digest(rs_ref))       # one draw, nothing else
            seen.add('step skipped')
        else:
            u8, mm = mine['frames_u8'], A.minmax(mine['frames_u8'])
            assert ref['frames'].dtype == np.float64 and ref['alphas'].dtype == np.uint8
            assert np.array_equal(ref['frames'], mine['frames']) and np.array_equal(ref['alphas'], mine['alphas'])
            for t in range(c['T']):                                           # the float64 frames are the clipped shift of the stored uint8 warp
                assert np.array_equal(ref['frames'][t], np.clip(u8[t] + mine['intensity'], mm[t, 0], mm[t, 1]))
            assert mine['matrix'] is not None and abs(mine['intensity']) < 0.03 * 255
            if c['p'] < 1:
                seen.add('fires at p = 0.1')
            seen.add('shear form %d' % mine['form'])
            if (c['T'], c['n']) == (3, 2):
                seen.add('clip T=3 n=2')
            lin = np.stack([A.warpAffine(a, mine['matrix'], (w, h), flags=A.INTER_LINEAR) for a in alphas])
            assert not np.array_equal(lin, ref['alphas']) and set(np.unique(ref['alphas'])) <= set(np.unique(alphas)) | {0}
            seen.add('alphas nearest, not linear')
            assert frames.min() > 0 and min(u8[:, 0, 0].max(), u8[:, 0, -1].max(), u8[:, -1, 0].max(), u8[:, -1, -1].max()) == 0
            seen.add('border corner 0')
            shifted = u8.astype(np.float64) + mine['intensity']
            if (shifted > mm[:, 1].reshape(-1, 1, 1, 1)).any():
                assert mine['intensity'] > 0 and (ref['frames'] < shifted).any()
                seen.add('clip active at the max')
            if (shifted < mm[:, 0].reshape(-1, 1, 1, 1)).any():
                assert mine['intensity'] < 0 and (ref['frames'] > shifted).any()
                seen.add('clip active at the min')
            if h != w:
                # the swapped offset centre is visible: the reference's matrix is not the one centred on (w, h)
                fired, cvM, _, _ = A.draws(np.random.RandomState(c['rs_seed']), w, h, c['p'])
                assert fired and not np.array_equal(cvM, mine['matrix'])
                assert not np.array_equal(np.stack([A.warpAffine(x, cvM, (w, h)) for x in frames]), u8)
                seen.add('h != w')
            out[name + '.matrix'] = np.asarray(mine['matrix'], np.float64)
        out[name + '.frames'], out[name + '.alphas'] = R.pack_rows(mine['frames_u8']), R.pack_rows(ref['alphas'])
        assert np.array_equal(R.unpack_rows(out[name + '.frames']), mine['frames_u8'])
        out[name + '.info'] = np.asarray([int(mine['fired']), -1 if mine['form'] is None else mine['form'], c['T'], c['n']], np.int32)
        out[name + '.intensity'] = np.asarray([mine['intensity']], np.float64)
        out[name + '.minmax'] = A.minmax(mine['frames_u8'])
        out[name + '.state'] = A.state_digest(rs_ref)
    assert seen == WANTED, 'not visible: %s' % sorted(WANTED - seen)
    path = os.path.join(HERE, 'affine_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(HERE, 'geometry_pinned.npz')), size
    print('wrote affine_pinned.npz', size, 'bytes', len(out), 'arrays', sorted(seen))


if __name__ == '__main__':
    main()
