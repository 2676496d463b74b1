"""Generate tests/golden/background_pinned.npz from the NumPy restatement (tests/background_restatement.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_background_golden.py

For each case of CASES: the seeded clip (`<case>.fg`, (T, h, w, 3)), its alphas (`<case>.alphas`), the decoded background (`<case>.bg`), the
draws (`<case>.draws` = ksize or 0, x, y, fired, match_bg; `<case>.floats` = sigma or 0, ratio or 0), and what the chain
LoadRandomBackground -> HistogramMatching -> ComposeBackground makes of them: `<case>.frames`, the matched `<case>.fg_out` and the matched
window `<case>.bg_out`, and the curves `<case>.luts`. The histogram matching goes through the float32 frames (np.unique / np.interp), the
composite through the reference's literal expression; the generator asserts that the table forms give the same bytes. `versions` records the
NumPy version the file was made with: np.interp's arithmetic is what the fixture pins. No OpenCV and no skimage were involved: neither is
installed here, and the fixture was NOT compared with either."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import background_restatement as R                             # noqa: E402

# name: (T, h, w, bh, bw, kind of the background, (ksize, sigma) or None, x, y, (ratio, match_bg) or None, seed)
CASES = {
    'plain': (2, 9, 11, 20, 23, 'noise', None, 3, 4, None, 1),
    'blur_only': (1, 17, 19, 30, 33, 'ramp', (15, 3.0), 14, 13, None, 2),
    'match_fg': (3, 12, 21, 25, 40, 'band', None, 0, 0, (0.37, False), 3),
    'match_bg': (2, 16, 16, 33, 35, 'band', (25, 5.0), 19, 17, (0.4999, True), 4),
    'small_bg_wide_blur': (2, 4, 5, 5, 7, 'noise', (25, 1.5), 2, 1, (0.125, False), 5),
    'crosses_tiles': (1, 33, 65, 70, 131, 'ramp', (5, 1.0), 66, 37, (0.0, False), 6),
}


def run(case):
    T, h, w, bh, bw, kind, blur, x, y, hist, seed = case
    fg, alphas, bg = R.clip(T, h, w, seed), R.alphas(T, h, w, seed + 100), R.image(bh, bw, seed + 200, kind)
    frames, fg_out, bg_out = R.chain(fg, alphas, bg, blur, x, y, hist)
    win = R.window(bg, None if blur is None else R.taps(*blur), x, y, h, w)
    luts = R.luts(fg, win, hist)
    assert np.array_equal(R.apply_luts(fg, luts[0]), fg_out) and np.array_equal(R.apply_luts(win, luts[1]), bg_out)
    assert np.array_equal(R.compose_table(fg_out, alphas, bg_out), frames)
    return dict(fg=fg, alphas=alphas, bg=bg, frames=frames, fg_out=fg_out, bg_out=bg_out, luts=luts,
                draws=np.asarray([blur[0] if blur else 0, x, y, hist is not None, bool(hist and hist[1])], np.int32),
                floats=np.asarray([blur[1] if blur else 0.0, hist[0] if hist else 0.0], np.float64))


def main():
    out = {}
    for name, case in CASES.items():
        for k, v in run(case).items():
            out['%s.%s' % (name, k)] = v
    out['versions'] = np.asarray('numpy %s' % np.__version__)
    path = os.path.join(HERE, 'background_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200 * 1024, size
    print('wrote background_pinned.npz', size, 'bytes', len(out), 'arrays; numpy', np.__version__)


if __name__ == '__main__':
    main()
