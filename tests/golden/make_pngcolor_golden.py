"""Writes tests/golden/pngcolor_pinned.npz: a subset of the case list of tests/pngcolor_restatement.py -- each of the 15 (colour type, depth)
pairs, interlaced or not in turn, the grey-16 edge values, a short palette and a palette with tRNS -- with what live Pillow returns for them:
`file_<name>` the file's bytes, `rgb_<name>` convert("RGB"), `l_<name>` convert("L"). A different Pillow on another machine shows up as a
difference to this file. Run from the repository root: python tests/golden/make_pngcolor_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pngcolor_restatement as R                            # noqa: E402


def main():
    cases = R.small_cases()
    out = {}
    for name in R.golden_names(cases):
        d = cases[name]
        rgb, l = R.pillow(d)
        _, rrgb, rl = R.decode(d)
        assert np.array_equal(rgb, rrgb) and np.array_equal(l, rl), name
        out['file_' + name] = np.frombuffer(d, np.uint8)
        out['rgb_' + name] = rgb
        out['l_' + name] = l
    path = os.path.join(HERE, 'pngcolor_pinned.npz')
    np.savez_compressed(path, **out)
    print(path, len(out) // 3, 'files', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
