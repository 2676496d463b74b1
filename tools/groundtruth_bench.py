"""Device time of the ground-truth maps (maggie_amd.utils.groundtruth, csrc/morph.hip) for one item of each kind against the plain
"read the uint8 planes once, write the fp32 maps once" HBM bound, with scipy.ndimage's footprint filters timed on the host beside them
(a stand-in for scale only: OpenCV's SIMD morphology, which the reference's loaders use, is faster than SciPy's and is not measured).
usage: python tools/groundtruth_bench.py [--no-cpu]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from scipy import ndimage

from _timing import timed
from maggie_amd.utils import groundtruth as G
from oracle.region import ellipse_kernel

dev = torch.device('cuda:0')
PEAK = 8000.0                                                     # GB/s, MI355X HBM3E
THREADS = min(16, os.cpu_count() or 1)


def soft(rs, H, W, cy=None, cx=None):
    yy, xx = np.mgrid[0:H, 0:W]
    ry, rx = rs.uniform(H / 10, H / 4), rs.uniform(W / 12, W / 5)
    cy = rs.uniform(0.2 * H, 0.8 * H) if cy is None else cy
    cx = rs.uniform(0.2 * W, 0.8 * W) if cx is None else cx
    d = (1.0 - np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)) * min(ry, rx)
    return np.clip(np.rint((0.5 + d / 6.0) * 255), 0, 255).astype(np.uint8)


def gpu_us(fn, reps=50):
    """Median and minimum over `reps` launches, each bracketed by its own event pair, after a warm-up."""
    return timed([fn], reps, warmup=5)[0][:2]


def scipy_ms(planes, k, n, erode=True):
    elem = ellipse_kernel(k).astype(bool)

    def one(p):
        d = e = p
        for _ in range(n):
            d = ndimage.maximum_filter(d, footprint=elem, mode='constant', cval=0)
            if erode:
                e = ndimage.minimum_filter(e, footprint=elem, mode='constant', cval=255)
        return d > e if erode else d > 0
    t = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        list(ex.map(one, list(planes)))
    return (time.perf_counter() - t) * 1e3


def main():
    cpu = '--no-cpu' not in sys.argv
    rs = np.random.RandomState(0)
    rows = []
    # image training item: 10 instance planes of 512 x 512, the worst draw (k = 4, 14 passes)
    img = np.stack([soft(rs, 512, 512) for _ in range(10)])[None]
    x = torch.from_numpy(img).to(dev)
    dr = G.draws(4, 14, 1)
    us = gpu_us(lambda: G.transition_gt(x, dr, thresh=5))
    rows.append(('image train item 10 x 512^2, k=4 n=14', img.size * 5, us, scipy_ms(img[0], 4, 14) if cpu else None))
    # the same on uniform noise: no tile is plain, every pass of every tile runs (the worst case for the kernel, not a matte)
    xn = torch.from_numpy(rs.randint(0, 256, size=img.shape).astype(np.uint8)).to(dev)
    us = gpu_us(lambda: G.transition_gt(xn, dr, thresh=5))
    rows.append(('  the same on uniform noise (no plain tile)', img.size * 5, us, None))
    # 16 such items in one launch (per-frame draws): per item
    x16 = x.expand(16, -1, -1, -1).contiguous()
    dr16 = G.draws(4, 14, 16)
    us = gpu_us(lambda: G.transition_gt(x16, dr16, thresh=5))
    rows.append(('  16 items in one launch, per item', img.size * 5, (us[0] / 16, us[1] / 16), None))
    # video training item: T = 8, 3 instances, 10 slots, 512 x 512, the worst draw (k = 4, 6 passes)
    T = 8
    cy, cx = rs.uniform(200, 300, 3), rs.uniform(200, 300, 3)
    clip = np.stack([np.stack([soft(np.random.RandomState(7 + j), 512, 512, cy[j] + 3 * t, cx[j] - 2 * t) for j in range(3)]) for t in range(T)])
    xc = torch.from_numpy(clip).to(dev)
    drc = G.draws(4, 6, T)
    us = gpu_us(lambda: G.diff_transition(xc, drc, None, n_slots=10))
    diffs = [(np.abs(clip[t].astype(np.int16) - clip[t - 1]) > 5).any(0).astype(np.uint8) * 255 for t in range(1, T)]
    rows.append(('video train item T=8, 3 inst -> 10 slots, 512^2, k=4 n=6', clip.size + T * 10 * 512 * 512 * 4, us,
                 scipy_ms(diffs, 4, 6, erode=False) if cpu else None))
    # evaluation frame: 5 instances at 1080 x 1920, k = 25, one pass
    ev = np.stack([soft(rs, 1080, 1920) for _ in range(5)])[None]
    xe = torch.from_numpy(ev).to(dev)
    us = gpu_us(lambda: G.trimap(xe))
    rows.append(('eval frame 5 x 1080 x 1920, k=25 n=1 (trimap)', ev.size * 5, us, scipy_ms(ev[0], 25, 1) if cpu else None))
    xn = torch.from_numpy(rs.randint(0, 256, size=ev.shape).astype(np.uint8)).to(dev)
    us = gpu_us(lambda: G.trimap(xn))
    rows.append(('  the same on uniform noise (no plain tile)', ev.size * 5, us, None))
    print('%-60s %10s %10s %10s %9s %12s' % ('workload', 'MB', 'median us', 'min us', '% of HBM', 'scipy ms (%d thr)' % THREADS))
    for name, nbytes, (med, mn), ms in rows:
        print('%-60s %10.1f %10.1f %10.1f %8.1f%% %12s' % (name, nbytes / 1e6, med, mn, 100.0 * nbytes / (med * 1e-6) / (PEAK * 1e9),
                                                            '-' if ms is None else '%.1f' % ms))


if __name__ == '__main__':
    main()
