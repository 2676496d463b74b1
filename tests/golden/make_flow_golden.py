"""Generate tests/golden/flow_pinned.npz (build container only; run it in its own interpreter):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flow_golden.py

(a) 'flow.<case>': fp64 flows of the small cases of tests/flow_restatement.py from an independent statement of the algorithm built on
    scipy.ndimage (correlate1d with 'mirror' / 'nearest' for every separable pass, map_coordinates for the sample of the second image's
    expansion, dense interpolation matrices for the resizes). The generator asserts that it equals the restatement to 1e-12 in fp64, that the
    fp32 restatement's rounded flow differs from the fp64 one's on at most 1e-4 of the pixels of every case (the largest one included), and that
    every moving case has a non-zero rounded flow on at least half of its pixels.
(b) 'messddt.<case>' = [update() return, score, count, average()] from THE REFERENCE's own maggie/utils/metric.py MESSDdt.update on the seeded
    inputs of flow_restatement.reduction_case. Stand-ins: cv2 is oracle/ref_loader.py's (it has no optical flow), skimage an empty module; `Pool` runs in-process; `calcOpticalFlow` hands
    back the case's integer-valued flows in the order the reference asks for them, and checks that the planes it is handed, cast as the
    reference casts them (`astype(np.uint8)`), are flow_restatement.gt_u8 of the ground truth."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import flow_restatement as R                                   # noqa: E402

STORED = ('40x36', '131x150', '131x150_still', '9x11')         # the flows small enough to store


# ---- (a) the scipy statement ---------------------------------------------------------------------------------------------------------------------------
def _gauss(n, sigma):
    if sigma <= 0:
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(n) - n // 2
    g = np.exp(-0.5 * (x / sigma) ** 2)
    return g / g.sum()


def _interp_matrix(n_src, n_dst):
    A = np.zeros((n_dst, n_src))
    for o in range(n_dst):
        f = (o + 0.5) * (n_src / n_dst) - 0.5
        i = int(np.floor(f))
        w = f - i
        if i < 0:
            i, w = 0, 0.0
        if i >= n_src - 1:
            i, w = n_src - 1, 0.0
        A[o, i] += 1 - w
        A[o, min(i + 1, n_src - 1)] += w
    return A


def _resize(a, h, w):
    return _interp_matrix(a.shape[0], h) @ (a @ _interp_matrix(a.shape[1], w).T)


def _polyexp(img):
    from scipy.ndimage import correlate1d
    x = np.arange(-7, 8, dtype=np.float64)
    g = _gauss(15, 1.5)
    basis = lambda X, Y: [np.ones_like(X), X, Y, X * X, Y * Y, X * Y]               # noqa: E731
    X, Y = np.meshgrid(x, x)
    B = np.stack([b.reshape(-1) for b in basis(X, Y)], 1)
    ig = np.linalg.inv(B.T @ (np.outer(g, g).reshape(-1, 1) * B))
    c = lambda ky, kx: correlate1d(correlate1d(img, ky, axis=0, mode='nearest'), kx, axis=1, mode='nearest')       # noqa: E731
    s = c(g, g)
    return (ig[1, 1] * c(g, x * g), ig[1, 1] * c(x * g, g), ig[0, 3] * s + ig[3, 3] * c(g, x * x * g), ig[0, 3] * s + ig[3, 3] * c(x * x * g, g),
            ig[5, 5] * c(x * g, x * g))


def _matrices(R0, R1, flow):
    from scipy.ndimage import map_coordinates
    H, W = R0[0].shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    px, py = xx + flow[..., 0], yy + flow[..., 1]
    inside = (np.floor(px) >= 0) & (np.floor(px) < W - 1) & (np.floor(py) >= 0) & (np.floor(py) < H - 1)
    S = [map_coordinates(r, [np.where(inside, py, 0), np.where(inside, px, 0)], order=1, mode='nearest') for r in R1]
    bx = np.where(inside, (R0[0] - S[0]) / 2, 0.0)
    by = np.where(inside, (R0[1] - S[1]) / 2, 0.0)
    axx = np.where(inside, (R0[2] + S[2]) / 2, R0[2])
    ayy = np.where(inside, (R0[3] + S[3]) / 2, R0[3])
    axy = np.where(inside, (R0[4] + S[4]) / 4, R0[4] / 2)

    def edge(n):
        s = np.ones(n)
        for i, v in enumerate(R.BORDER):
            if i < n:
                s[i] *= v
                s[n - 1 - i] *= v
        return s
    sc = np.outer(edge(H), edge(W))
    bx, by, axx, ayy, axy = (v * sc for v in (bx, by, axx, ayy, axy))
    bx = bx + axx * flow[..., 0] + axy * flow[..., 1]
    by = by + axy * flow[..., 0] + ayy * flow[..., 1]
    return [axx ** 2 + axy ** 2, (axx + ayy) * axy, ayy ** 2 + axy ** 2, axx * bx + axy * by, axy * bx + ayy * by]


def _update(M):
    from scipy.ndimage import correlate1d
    g = _gauss(11, 1.5)
    g11, g12, g22, h1, h2 = (correlate1d(correlate1d(m, g, axis=0, mode='nearest'), g, axis=1, mode='nearest') for m in M)
    det = g11 * g22 - g12 ** 2 + 1e-3
    return np.stack([(g22 * h1 - g12 * h2) / det, (g11 * h2 - g12 * h1) / det], -1)


def scipy_farneback(prev_u8, next_u8):
    from scipy.ndimage import correlate1d
    H, W = prev_u8.shape
    sizes, k = [(H, W)], 0
    while k < 5 and min(H, W) * 0.5 ** (k + 1) >= 32:
        k += 1
        sizes.append((int(np.rint(H * 0.5 ** k)), int(np.rint(W * 0.5 ** k))))          # np.rint: half to even
    flow = None
    for k in range(len(sizes) - 1, -1, -1):
        h, w = sizes[k]
        sigma = (2.0 ** k - 1) / 2
        g = _gauss(max(int(np.rint(5 * sigma)) | 1, 3), sigma)
        imgs = [_resize(correlate1d(correlate1d(u.astype(np.float64), g, axis=1, mode='mirror'), g, axis=0, mode='mirror'), h, w)
                for u in (prev_u8, next_u8)]
        flow = np.zeros((h, w, 2)) if flow is None else 2 * np.stack([_resize(flow[..., c], h, w) for c in (0, 1)], -1)
        R0, R1 = _polyexp(imgs[0]), _polyexp(imgs[1])
        flow = _update(_matrices(R0, R1, flow))
        flow = _update(_matrices(R0, R1, flow))
    return flow


def flow_fixtures():
    out = {}
    for name, (h, w, shift, seed) in R.FLOW_CASES.items():
        a, b = R.frame_pair(h, w, shift, seed)
        f64, f32 = R.farneback(a, b, np.float64), R.farneback(a, b, np.float32)
        flips = float((np.rint(f32) != np.rint(f64)).any(-1).mean())
        assert flips <= 1e-4, (name, flips)
        moving = float((np.rint(f64) != 0).any(-1).mean())
        assert moving >= 0.5 or not (shift[0] or shift[1]), (name, moving)
        if name in STORED:
            stated = scipy_farneback(a, b)
            dist = float(np.abs(stated - f64).max())
            assert dist <= 1e-12, (name, dist)
            out['flow.' + name] = stated
        print(name, 'fp32 vs fp64 max-abs %.3g' % np.abs(f32 - f64).max(), 'flips %.3g' % flips, 'moving %.3f' % moving,
              'scipy vs restatement %.3g' % (dist if name in STORED else float('nan')))
    prev, nxt = R.batch_pairs()
    for p, (a, b) in enumerate(zip(prev, nxt)):
        f64, f32 = R.farneback(a, b, np.float64), R.farneback(a, b, np.float32)
        flips = float((np.rint(f32) != np.rint(f64)).any(-1).mean())
        assert flips <= 1e-4, ('batch', p, flips)
    return out


# ---- (b) the reference's reduction -----------------------------------------------------------------------------------------------------------------------
class _InProcessPool(object):
    def __init__(self, n):
        pass

    def imap(self, fn, items):
        return [fn(i) for i in items]

    def close(self):
        pass


def reduction_fixtures():
    from oracle import ref_loader
    ref_loader.load_reference()                                # registers the reference's packages and its cv2 stand-in (no optical flow in it)
    for name in ('skimage', 'skimage.measure'):
        sys.modules.setdefault(name, types.ModuleType(name))
    import importlib
    M = importlib.import_module('maggie.utils.metric')
    M.Pool = _InProcessPool
    out = {}
    for name in R.REDUCTION_CASES:
        pred, gt, tri, flows = R.reduction_case(name)
        F, N = gt.shape[:2]
        u8 = R.gt_u8(gt)
        order = iter([(t, n) for n in range(N) for t in range(F - 1)])                # one instance after the other, its pairs in order

        def supplied(frames):
            t, n = next(order)
            assert np.array_equal(frames[0].astype(np.uint8), u8[t, n]) and np.array_equal(frames[1].astype(np.uint8), u8[t + 1, n])
            return flows[t, n].astype(np.float32)
        m = M.MESSDdt()
        m.calcOpticalFlow = supplied
        r = m.update(pred, gt, tri)
        assert next(order, None) is None
        out['messddt.' + name] = np.asarray([r, m.score, m.count, m.average()], np.float64)
        mine = R.messddt(pred, gt, tri, flows)
        print(name, out['messddt.' + name].tolist(), 'restated', mine)
    return out


def main():
    out = flow_fixtures()
    out.update(reduction_fixtures())
    np.savez_compressed(os.path.join(HERE, 'flow_pinned.npz'), **out)
    print('wrote flow_pinned.npz', os.path.getsize(os.path.join(HERE, 'flow_pinned.npz')), 'bytes')


if __name__ == '__main__':
    main()
