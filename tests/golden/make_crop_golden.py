"""Generate tests/golden/crop_pinned.npz FROM THE REFERENCE (needs the reference's checkout beside this one, as make_geometry_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_crop_golden.py

The reference's own `RandomCropByAlpha` and `RandomHorizontalFlip` (maggie/dataloader/transforms.py:191-305) are loaded from its checkout with
the stand-in `cv2` of tests/geometry_restatement.py (copyMakeBorder, resize linear and nearest; OpenCV is not a dependency of this project) and
run through its `Compose` as him.py:44-45 wires them, on the seeded arrays of `crop_restatement.GOLDEN` (regenerated, not stored) with the
case's own `np.random.RandomState`. What this pins is the reference's draw order and glue, not OpenCV: the box with its `except`, the branch
draw, the window loop and how many randint pairs it consumes, the `min(x, w - cw)` clamp, the pad amounts, `crop_size` in cv2.resize's `dsize`
position, the flip draw and what it reverses.

The window the reference chose is not part of its output: it is recovered here by replaying the same calls on a second generator with the same
seed, and the replay is checked by comparing the generator states and by slicing the inputs at that window.

Stored per case: the uint8 frames and alphas (differences along the rows, `geometry_restatement.pack_rows`), the masks as packed bits,
`info` = (branch, x0, y0, pairs, flip, min_x, max_x, min_y, max_y) and a digest of the generator state afterwards. The generator asserts that
the restatement equals the reference, and that every property listed in WANTED is present and visible in the reference's outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import crop_restatement as C                                   # noqa: E402
import geometry_restatement as R                               # noqa: E402
import make_geometry_golden as MG                              # noqa: E402

WANTED = {'first window hits', 'first misses, second hits', 'three misses', 'empty alphas', 'mean != any', 'clip T=3 n=2', 'H == ch and W == cw',
          'clamped by W - cw', 'pad h > w', 'pad w > h, odd', 'non-square dsize', 'flip on', 'flip off', 'masks != alphas', 'crop branch',
          'padding branch'}


def run_reference(T, name):
    c = C.GOLDEN[name]
    frames, alphas, masks = C.golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    steps = [T.RandomCropByAlpha(c['crop'], rs, padding_prob=c['pp']), T.RandomHorizontalFlip(rs, c['fp'])]
    sample = T.Compose(steps)({'frames': frames.copy(), 'alphas': alphas.copy(), 'masks': masks.copy(), 'weights': None})
    return {k: np.ascontiguousarray(sample[k]) for k in ('frames', 'alphas', 'masks')}, rs


def main():
    T = MG.load_reference_transforms()
    out, seen = {}, set()
    for name, c in C.GOLDEN.items():
        frames, alphas, masks = C.golden_inputs(name)
        ref, rs_ref = run_reference(T, name)
        mine, rs_mine = C.golden_run(name)
        for key in ('frames', 'alphas', 'masks'):
            assert ref[key].dtype == np.uint8 and np.array_equal(ref[key], mine[key]), '%s: restated %s differ from the reference' % (name, key)
        assert np.array_equal(C.state_digest(rs_ref), C.state_digest(rs_mine)), '%s: the generator states differ' % name
        ch, cw = c['crop']
        P, H, W = alphas.shape
        flip = mine['flip']
        seen.add('flip on' if flip else 'flip off')
        unflipped = {k: (v[:, :, ::-1] if flip else v) for k, v in ref.items()}
        assert (c['T'], c['n']) == (frames.shape[0], P // frames.shape[0])
        assert not np.array_equal(masks, alphas) and not np.array_equal(ref['masks'], ref['alphas'])
        seen.add('masks != alphas')
        if flip:                                                              # visible: the output is not its own mirror image
            assert not np.array_equal(ref['frames'], ref['frames'][:, :, ::-1]) and not np.array_equal(ref['frames'], ref['frames'][..., ::-1])
        if (c['T'], c['n']) == (3, 2):
            seen.add('clip T=3 n=2')
        if mine['branch'] == 'crop':
            seen.add('crop branch')
            x0, y0 = mine['window']
            # the window recovered by the replay is the one the reference used: its output is that slice of the inputs
            assert np.array_equal(unflipped['frames'], frames[:, y0:y0 + ch, x0:x0 + cw]) and ref['frames'].shape == (c['T'], ch, cw, 3)
            assert np.array_equal(unflipped['alphas'], alphas[:, y0:y0 + ch, x0:x0 + cw])
            assert np.array_equal(unflipped['masks'], masks[:, y0:y0 + ch, x0:x0 + cw])
            hit = bool((ref['alphas'] > 127).any())
            count = C.bbox(alphas)[0]
            min_x, max_x, min_y, max_y = mine['box']
            if mine['pairs'] == 1 and hit and count:
                seen.add('first window hits')
            if mine['pairs'] == 2:
                assert hit and c['alphas'] == 'corners'
                # two pairs were consumed: replaying ONE pair and the flip draw leaves another state
                rs = np.random.RandomState(c['rs_seed'])
                rs.rand()
                hi_x, hi_y = max(max_x - cw, min_x + 1), max(max_y - ch, min_y + 1)
                w1 = (min(rs.randint(min_x, hi_x), W - cw), min(rs.randint(min_y, hi_y), H - ch))
                assert not (alphas[:, w1[1]:w1[1] + ch, w1[0]:w1[0] + cw] > 127).any() and w1 != (x0, y0)
                w2 = (min(rs.randint(min_x, hi_x), W - cw), min(rs.randint(min_y, hi_y), H - ch))
                rs.rand()
                assert w2 == (x0, y0) and np.array_equal(C.state_digest(rs), C.state_digest(rs_ref))
                seen.add('first misses, second hits')
            if mine['pairs'] == 3 and not hit and count:
                assert ref['alphas'].max() > 0                              # the miss is visible: something is there, nothing above 127
                seen.add('three misses')
            if count == 0:
                assert mine['box'] == (0, W, 0, H) and mine['pairs'] == 3 and not hit and alphas.max() > 0
                seen.add('empty alphas')
            if c['alphas'] == 'mean_vs_any':
                ly, lx = c['lone']
                any_box = np.where((alphas > 127).any(0))
                assert (alphas[:, ly, lx] > 127).sum() == 1 and P == 6 and any_box[0].max() == ly > max_y      # the box ignores it
                without = alphas.copy()
                without[:, ly, lx] = 0
                assert mine['pairs'] == 1 and hit and not (without[:, y0:y0 + ch, x0:x0 + cw] > 127).any()       # the hit test sees it, and only it
                seen.add('mean != any')
            if (H, W) == (ch, cw):
                assert (x0, y0) == (0, 0)
                seen.add('H == ch and W == cw')
            if count and min_x > W - cw:
                assert x0 == W - cw
                seen.add('clamped by W - cw')
            info = [0, x0, y0, mine['pairs'], int(flip), min_x, max_x, min_y, max_y]
        else:
            seen.add('padding branch')
            assert ref['frames'].shape == (c['T'], cw, ch, 3) and ref['alphas'].shape == (P, cw, ch)          # dsize = (ch, cw): ch wide, cw high
            if ch != cw:
                seen.add('non-square dsize')
            if H > W:
                seen.add('pad h > w')
                edge = unflipped['frames'][:, :, 0]
            else:
                assert (W - H) % 2 == 1
                seen.add('pad w > h, odd')
                edge = unflipped['frames'][:, 0]
            assert edge.max() == 0 and frames.min() > 0                       # the border is visible next to frames that are never 0
            lin = C.padresize(masks, c['crop'], flip, R.INTER_LINEAR)
            assert not np.array_equal(lin, ref['masks']) and set(np.unique(ref['masks'])) <= {0, 255}          # nearest, not linear
            info = [1, 0, 0, 0, int(flip)] + list(mine['box'])
        out[name + '.frames'], out[name + '.alphas'] = R.pack_rows(ref['frames']), R.pack_rows(ref['alphas'])
        assert np.array_equal(R.unpack_rows(out[name + '.frames']), ref['frames']) and np.array_equal(R.unpack_rows(out[name + '.alphas']), ref['alphas'])
        out[name + '.masks'] = np.packbits(ref['masks'] > 0)
        out[name + '.info'] = np.asarray(info, np.int32)
        out[name + '.state'] = C.state_digest(rs_ref)
    assert seen == WANTED, 'not visible: %s' % sorted(WANTED - seen)
    path = os.path.join(HERE, 'crop_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(HERE, 'geometry_pinned.npz')), size
    print('wrote crop_pinned.npz', size, 'bytes', len(out), 'arrays', sorted(seen))


if __name__ == '__main__':
    main()
