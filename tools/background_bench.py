"""Device time of the background chain (maggie_amd.utils.background, csrc/background.hip) on one item: a clip of 8 frames of 1080 x 1920 over a
2160 x 3840 background, warm, draws resident on the device, every call bracketed by its own event pair, the candidates alternated call by call:
  * the window: the plain copy, and the blur with ksize 5, 15 and 25;
  * the histogram of the clip on noise and on a constant image (every lane hits one bin), and of the window;
  * the curves (one workgroup);
  * the composite without curves, with curves, and with the two extra outputs;
  * the chain `random_background`, matching fired (five launches and a fill) and not fired (two launches);
  * the NumPy / scipy restatement of the chain on the host (tests/background_restatement.py with the blur through scipy's integer correlation
    of the window plus its halo only -- the cheapest honest host form), timed with a host clock, a few repetitions.
Next to each device time: the bytes the launch must move (input once, output once) and the time those bytes take at the measured HBM copy rate
of 6.29 TB/s (MI355X; 8 TB/s is the datasheet's). The event pair also spans the host side of the call (the checks and the ctypes launches), so
a time near the launch overhead says little about the kernel. The tool first asserts that the device chain equals the host chain byte for byte.
usage: python tools/background_bench.py [reps] [host_reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import background_restatement as R
from _timing import timed
from maggie_amd.utils import background as B

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100
HOST_REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
T, H, W, BH, BW = 8, 1080, 1920, 2160, 3840
X, Y = 901, 517
HBM = 6.29e12


def host_window(bg, q, x, y, h, w):
    """The restated window through scipy on the window plus its halo (the whole-background blur of the reference would cost four times more)."""
    from scipy import ndimage
    if q is None:
        return np.ascontiguousarray(bg[y:y + h, x:x + w])
    r = len(q) // 2
    box = bg[y - r:y + h + r, x - r:x + w + r].astype(np.int64)            # X, Y leave room for the halo: no border inside the box
    s1 = ndimage.correlate1d(box, q.astype(np.int64), axis=1, mode='mirror')
    s2 = ndimage.correlate1d(s1, q.astype(np.int64), axis=0, mode='mirror')
    return ((s2[r:-r, r:-r] + 32768) >> 16).astype(np.uint8)


def host_chain(fg, a, bg, q, x, y, hist):
    win = host_window(bg, q, x, y, H, W)
    luts = R.luts(fg, win, hist)
    return R.compose_literal(R.apply_luts(fg, luts[0]), a, R.apply_luts(win, luts[1]))


def main():
    rng = np.random.default_rng(0)
    fg_h = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    a_h = rng.integers(0, 256, (T, H, W), dtype=np.uint8)
    bg_h = rng.integers(0, 256, (BH, BW, 3), dtype=np.uint8)
    fg, a, bg = (torch.from_numpy(v).to(dev) for v in (fg_h, a_h, bg_h))
    const = torch.full((T, H, W, 3), 131, dtype=torch.uint8, device=dev)
    hist = (0.3, False)
    hd = B.HistDraws(*hist).to(dev)
    draws = {ks: B.BackgroundDraws(None if ks == 0 else B.gaussian_taps(ks, 3.0), X, Y, H, W).to(dev) for ks in (0, 5, 15, 25)}

    got = B.random_background(fg, a, bg, draws[25], hd)
    want = host_chain(fg_h, a_h, bg_h, R.taps(25, 3.0), X, Y, hist)
    assert np.array_equal(got.cpu().numpy(), want), 'the device chain differs from the host chain'
    assert np.array_equal(B.blur_crop(bg, draws[25]).cpu().numpy(), R.window(bg_h, R.taps(25, 3.0), X, Y, H, W))
    print('device chain == host chain on %d frames of %d x %d over %d x %d' % (T, H, W, BH, BW))

    win = B.blur_crop(bg, draws[15])
    luts = B.match_luts(fg, win, hd)
    counts = torch.zeros((2, 3, 256), dtype=torch.int32, device=dev)
    B._run_hist(fg, T * H * W, counts[0])
    B._run_hist(win, H * W, counts[1])
    clip, frame = fg.numel(), win.numel()
    rows = [('window copy', lambda: B.blur_crop(bg, draws[0]), 2 * frame)]
    rows += [('window blur ksize %d' % ks, lambda ks=ks: B.blur_crop(bg, draws[ks]), 2 * frame) for ks in (5, 15, 25)]
    rows += [('histogram clip, noise', lambda: B.histograms(fg), clip), ('histogram clip, constant', lambda: B.histograms(const), clip),
             ('histogram window', lambda: B.histograms(win), frame),
             ('curves', lambda: B._run_luts(counts, hd), 2 * 3 * 256 * 4 + 1536),
             ('composite', lambda: B.compose(fg, a, win), 2 * clip + clip // 3 + frame),
             ('composite with curves', lambda: B.compose(fg, a, win, luts), 2 * clip + clip // 3 + frame),
             ('composite, curves, fg and bg out', lambda: B.compose(fg, a, win, luts, True), 3 * clip + clip // 3 + 2 * frame),
             ('chain, blur 25, matching fired', lambda: B.random_background(fg, a, bg, draws[25], hd), 0),
             ('chain, blur 25, not fired', lambda: B.random_background(fg, a, bg, draws[25], None), 0),
             ('chain, copy, not fired', lambda: B.random_background(fg, a, bg, draws[0], None), 0)]
    print('%d calls each' % REPS)
    print('%-36s %10s %10s %10s %10s %10s %12s' % ('launch', 'median us', 'min us', 'p25 us', 'p75 us', 'MB moved', 'us at HBM'))
    for (name, _, nbytes), (med, mn, lo, hi) in zip(rows, timed([r[1] for r in rows], REPS)):
        print('%-36s %10.1f %10.1f %10.1f %10.1f %10.2f %12.2f' % (name, med, mn, lo, hi, nbytes / 1e6, nbytes / HBM * 1e6))

    print('host restatement (NumPy / scipy), %d runs each, host clock' % HOST_REPS)
    for name, fn in (('host window blur ksize 25', lambda: host_window(bg_h, R.taps(25, 3.0), X, Y, H, W)),
                     ('host chain, blur 25, matching fired', lambda: host_chain(fg_h, a_h, bg_h, R.taps(25, 3.0), X, Y, hist)),
                     ('host chain, blur 25, not fired', lambda: host_chain(fg_h, a_h, bg_h, R.taps(25, 3.0), X, Y, None))):
        ts = []
        for _ in range(HOST_REPS):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        print('%-36s %10.1f ms median %10.1f ms min' % (name, np.median(ts) * 1e3, np.min(ts) * 1e3))


if __name__ == '__main__':
    main()
