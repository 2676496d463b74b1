"""Generate tests/golden/maskgen_pinned.npz FROM THE REFERENCE (needs the reference's checkout beside this one, as make_groundtruth_golden.py does):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_maskgen_golden.py

The reference's own transform classes (maggie/dataloader/transforms.py: GenMaskFromAlpha, RandomBinarizedMask, DownUpMask, CutMask,
MaskDropout) are loaded from its checkout with a stand-in `cv2` -- threshold, dilate, erode, resize and the constants they name, all from
tests/maskgen_restatement.py (OpenCV is not a dependency of this project) -- and run as the datasets wire them (him.py:50-54, vim.py:58-66) on the seeded
planes of `maskgen_restatement.GOLDEN` (regenerated, not stored). What this pins is the reference's draw order and glue, not OpenCV.

Every branch of the chain must fire in some case, and the generator asserts it: the four morphology orders, down / up applied and skipped,
CutMask internal with overlapping rectangles, external, neither, a drop-out that zeroes a rectangle and one that skips a plane by its size
test -- each with a visible effect on the output where it has one.

Stored per case: the output as packed bits with its shape."""
import importlib
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import maskgen_restatement as M                                # noqa: E402
from maggie_amd.utils import maskgen                           # noqa: E402
from oracle import ref_loader                                  # noqa: E402


def load_reference_transforms():
    """maggie.dataloader.transforms of the reference. It imports cv2 / PIL / albumentations / imgaug / skimage at the top: cv2 is the stand-in of
    the restatement, the others (used by other classes only) are empty."""
    saved = {n: sys.modules.get(n) for n in ('cv2',)}
    sys.modules['cv2'] = M.cv2_standin()
    for name in ('albumentations', 'imgaug', 'imgaug.augmenters', 'imgaug.parameters', 'skimage', 'skimage.exposure'):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules['imgaug'].augmenters, sys.modules['imgaug'].parameters = sys.modules['imgaug.augmenters'], sys.modules['imgaug.parameters']
    sys.modules['skimage'].exposure = sys.modules['skimage.exposure']
    base = os.path.join(ref_loader.REF_ROOT, 'maggie')
    for name, path in (('maggie', base), ('maggie.dataloader', os.path.join(base, 'dataloader'))):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = [path]
            sys.modules[name] = pkg
    try:
        sys.modules.pop('maggie.dataloader.transforms', None)                # bind to THIS cv2
        return importlib.import_module('maggie.dataloader.transforms')
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def run_reference(T, name):
    """The reference's chain on the case's planes, as the datasets wire it; returns the masks and the state of both generators afterwards."""
    c = M.GOLDEN[name]
    planes = M.golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    random.seed(c['py_seed'])                                              # CutMask.external samples with the module-level `random`
    sample = {'alphas': planes.copy(), 'masks': planes.copy()}
    steps = []
    if c['video']:
        steps.append(T.GenMaskFromAlpha(1.0))
    steps += [T.RandomBinarizedMask(rs, binarize_max_k=c['max_k']), T.DownUpMask(rs, 0.125, c['p']), T.CutMask(rs)]
    if c['video']:
        steps.append(T.MaskDropout(rs))
    for step in steps:
        sample = step(sample)
    out = np.asarray(sample['masks'])
    assert out.dtype == np.uint8 and out.shape == planes.shape and set(np.unique(out)) <= {0, 255}
    return out


def restated(name, fired):
    """The same case through the product's draws and the restated operators, recording which branches fired and that each is visible."""
    c = M.GOLDEN[name]
    planes = M.golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    py = random.Random(c['py_seed'])
    draws = maskgen.draw_chain(rs, py, c['n'], c['H'], c['W'], c['max_k'], c['p'], dropout=c['video'], from_alpha=c['video'])
    for row in draws.morph.tolist():
        fired.add(M.ORDERS[row[3]])
    fired.update('downup' if a else 'no downup' for a in draws.downup.tolist())
    before = M.chain(planes, types.SimpleNamespace(morph=draws.morph, downup=draws.downup, cut=np.full_like(draws.cut, -1), ratio=draws.ratio))
    m = M.chain(planes, draws)
    live = [(p, r) for p, r in enumerate(draws.cut.tolist()) if r[0] >= 0]
    if not live:
        fired.add('cut neither')
    for p, (sp, dr, dc, sr, sc, h, w, _) in live:
        if sp == p:
            overlap = abs(dr - sr) < h and abs(dc - sc) < w and (dr, dc) != (sr, sc)
            if overlap and not np.array_equal(m[p], before[p]):
                fired.add('cut internal, overlapping')
        elif not np.array_equal(m[p], before[p]):
            fired.add('cut external')
    if c['video']:
        st = M.stats(m)
        sel = maskgen.draw_dropout(rs, st)
        after = M.drop(m, sel, st)
        for i, idx, ph, pw in sel.tolist():
            if i >= 0 and not np.array_equal(after[i], m[i]):
                fired.add('dropout zeroed')
            if i < 0 and st[-i - 1, 0] > 0:                                  # skipped although the plane is not empty: the size test
                fired.add('dropout skipped by size')
        m = after
    return m


WANTED = set(M.ORDERS) | {'downup', 'no downup', 'cut internal, overlapping', 'cut external', 'cut neither', 'dropout zeroed',
                          'dropout skipped by size'}


def main():
    T = load_reference_transforms()
    out, fired = {}, set()
    for name in M.GOLDEN:
        ref = run_reference(T, name)
        mine = restated(name, fired)
        assert np.array_equal(ref, mine), '%s: the product draws + restated operators differ from the reference in %d pixels' % (name, (ref != mine).sum())
        out[name], out[name + '.shape'] = np.packbits(ref > 0), np.asarray(ref.shape)
    assert fired == WANTED, 'branches not hit: %s' % sorted(WANTED - fired)
    path = os.path.join(HERE, 'maskgen_pinned.npz')
    np.savez_compressed(path, **out)
    print('wrote maskgen_pinned.npz', os.path.getsize(path), 'bytes', {k: v.shape for k, v in out.items()}, sorted(fired))


if __name__ == '__main__':
    main()
