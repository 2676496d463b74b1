"""Generate tests/golden/geometry_pinned.npz FROM THE REFERENCE (needs the reference's checkout beside this one, as make_maskgen_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_geometry_golden.py

The reference's own transform classes (maggie/dataloader/transforms.py: Compose, ResizeShort, PaddingMultiplyBy, Stack, GenMaskFromAlpha,
DownUpMask, ToTensor, Normalize) are loaded from its checkout with a stand-in `cv2` -- resize (linear and nearest, planes and 3-channel frames),
copyMakeBorder and the mask operators, all from tests/geometry_restatement.py and tests/maskgen_restatement.py (OpenCV is not a dependency of this
project) -- and run as the evaluation datasets and the demo predictor wire them (him.py:36-65 with and without a mask directory,
demo/maggie_predictor.py:26-50) on the seeded arrays of `geometry_restatement.GOLDEN` (regenerated, not stored); `Load` is skipped and arrays are
passed. What this pins is the reference's glue, not OpenCV: the `int()` truncation of the size, the `ratio != 1` skip, linear for alphas against
nearest for masks, the padding side, ToTensor's `< 5` rule and GenMaskFromAlpha's misplaced interpolation argument.

The chain is run in two parts (the uint8 transforms through `Compose`, then ToTensor and Normalize called on the same dict, which is all
`Compose` does) so that the uint8 state can be recorded. The generator asserts that the restated chain equals the reference's output, that
every case is present and that the inputs make the padding, the `< 5` rule and the nearest / linear difference visible.

Stored per case: the uint8 frames and alphas after Stack (as differences along the rows, `geometry_restatement.pack_rows`), the masks (mask
directory: nearest; none: GenMaskFromAlpha + DownUpMask) as packed bits, the numbers of `transform_info`; the predictor's masks for two cases;
the normalised fp32 frames of one small case."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import geometry_restatement as R                               # noqa: E402
import groundtruth_restatement as G                            # noqa: E402
import maskgen_restatement as M                                # noqa: E402
import make_maskgen_golden as MM                               # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def load_reference_transforms():
    saved = M.cv2_standin
    M.cv2_standin = R.cv2_standin                                          # the loader of make_maskgen_golden.py, over this stand-in
    try:
        return MM.load_reference_transforms()
    finally:
        M.cv2_standin = saved


def run_reference(T, name, wiring):
    """`wiring`: 'masks' (him.py evaluation with a mask directory), 'no_masks' (without: the mask comes from the alphas) or 'predict'
    (maggie_predictor.py: the instance masks are both the alphas and the masks). Returns the uint8 state after the uint8 transforms and the
    dict after ToTensor + Normalize."""
    c = R.GOLDEN[name]
    frames, alphas, masks = R.golden_inputs(name)
    rs = np.random.RandomState(2023)
    steps = [T.ResizeShort(c['short'], transform_alphas=False), T.PaddingMultiplyBy(c['divisor'], transform_alphas=False), T.Stack()]
    if wiring == 'no_masks':
        steps += [T.GenMaskFromAlpha(), T.DownUpMask(rs, 0.125, 1.0)]
    sample = {'frames': [f.copy() for f in frames], 'masks': None if wiring == 'no_masks' else [m.copy() for m in masks], 'weights': None,
              'alphas': [m.copy() for m in masks] if wiring == 'predict' else [a.copy() for a in alphas]}
    sample = T.Compose(steps)(sample)
    u8 = {k: np.array(sample[k], copy=True) for k in ('frames', 'alphas', 'masks')}
    info = sample['transform_info']
    sample = T.Normalize(mean=MEAN, std=STD)(T.ToTensor()(sample))
    assert sample['transform_info'] is info
    return u8, sample, info


def main():
    T = load_reference_transforms()
    out, seen = {}, set()
    for name, c in R.GOLDEN.items():
        frames, alphas, masks = R.golden_inputs(name)
        u8, sample, info = run_reference(T, name, 'masks')
        rf, ra, rm, rinfo = R.resize_short_pad(frames, alphas, masks, c['short'], c['divisor'])
        assert info == rinfo and [d['name'] for d in info] == ['resize', 'padding'], (name, info)
        for key, mine in (('frames', rf), ('alphas', ra), ('masks', rm)):
            assert u8[key].dtype == np.uint8 and np.array_equal(u8[key], mine), '%s: restated %s differ from the reference' % (name, key)
        Tn, n = c['T'], c['n']
        ratio, (rh, rw), (ph, pw) = R.plan(c['h'], c['w'], c['short'], c['divisor'])
        assert rf.shape == (Tn, rh + ph, rw + pw, 3) and ra.shape == (Tn * n, rh + ph, rw + pw)
        # the tensor stage: ToTensor's `< 5` rule on the alphas (not on ori_alphas), Normalize on the frames
        assert np.array_equal(sample['alphas'].numpy().reshape(ra.shape), G.threshold(ra))
        assert np.array_equal(sample['ori_alphas'].numpy().reshape(alphas.shape), alphas)
        assert np.array_equal(sample['masks'].numpy().reshape(rm.shape), rm)
        image = sample['frames'].numpy()
        assert image.dtype == np.float32 and np.array_equal(image, R.normalized(rf))
        # visibility
        if ph or pw:
            seen.add('padding')
            assert rf[:, :rh, :rw].min() > 0 and (rf[:, rh:].max() if ph else 0) == 0 and (rf[:, :, rw:].max() if pw else 0) == 0
        if ((ra > 0) & (ra < 5)).any():
            seen.add('< 5 rule')
        if ratio != 1:
            lin = np.stack([np.pad(R.resize(m, (rw, rh)), ((0, ph), (0, pw))) for m in masks])
            assert not np.array_equal(lin, rm), '%s: nearest and linear masks agree' % name
            seen.add('nearest != linear')
        else:
            assert np.array_equal(rf[:, :rh, :rw], frames)
            seen.add('ratio 1')
        assert set(np.unique(rm)) <= {0, 255}
        # without a mask directory
        u8n, _, infon = run_reference(T, name, 'no_masks')
        gen = M.from_alpha(ra)
        assert infon == info and np.array_equal(u8n['masks'], gen) and np.array_equal(u8n['alphas'], ra) and set(np.unique(gen)) <= {0, 255}
        assert not np.array_equal(gen, rm)
        out[name + '.frames'], out[name + '.alphas'] = R.pack_rows(u8['frames']), R.pack_rows(u8['alphas'])
        assert np.array_equal(R.unpack_rows(out[name + '.frames']), rf) and np.array_equal(R.unpack_rows(out[name + '.alphas']), ra)
        out[name + '.masks'], out[name + '.genmasks'] = np.packbits(rm > 0), np.packbits(gen > 0)
        out[name + '.info'] = np.asarray([c['h'], c['w'], ratio, ph, pw], np.float64)
        assert tuple(info[0]['ori_size']) == (c['h'], c['w']) and info[0]['ratio'] == ratio and tuple(info[1]['pad_size']) == (ph, pw)
        if name == R.FP32_CASE:
            out[name + '.image'] = image
        if name in R.PREDICT_CASES:
            u8p, samplep, infop = run_reference(T, name, 'predict')
            assert infop == info and np.array_equal(u8p['frames'], rf) and np.array_equal(u8p['masks'], rm)
            assert np.array_equal(samplep['frames'].numpy(), image)
            out[name + '.predict_masks'] = np.packbits(samplep['masks'].numpy().reshape(rm.shape) > 0)
    wanted = {'padding', '< 5 rule', 'nearest != linear', 'ratio 1'}
    assert seen == wanted, 'not visible: %s' % sorted(wanted - seen)
    assert R.FP32_CASE + '.image' in out and all(n + '.predict_masks' in out for n in R.PREDICT_CASES)
    path = os.path.join(HERE, 'geometry_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 64 * 1024, size
    print('wrote geometry_pinned.npz', size, 'bytes', len(out), 'arrays', sorted(seen))


if __name__ == '__main__':
    main()
