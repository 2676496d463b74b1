"""NumPy restatement of the loaders' guidance-mask chain (maggie/dataloader/transforms.py:388-565: GenMaskFromAlpha, RandomBinarizedMask,
DownUpMask, CutMask, MaskDropout), for the tests only -- the product never imports it.

OpenCV is not a dependency of this project, so `threshold`, `dilate` / `erode` with a rectangle and `resize` restate its
DOCUMENTED behaviour (an unpinned third-party restatement, like the ellipse filters of groundtruth_restatement.py):
  * threshold(u8, t, maxval, THRESH_BINARY): maxval where v > floor(t);
  * dilate / erode with np.ones((k, k)): anchor a = k // 2, dst[y, x] = max (min) over 0 <= i, j < k of src[y + i - a, x + j - a], pixels
    outside the image take no part (groundtruth_restatement's filters with an explicit element);
  * resize(INTER_LINEAR) on 8-bit data: size round_half_even(W * fx) with scale 1 / fx, or the given size with scale 1.0 / (dst / src);
    f = float32((d + 0.5) * scale - 0.5), s = floor(f), f -= s, clamped to the first / last index with f = 0; coefficients
    round_half_even(float32(1 - f) * 2048), round_half_even(f * 2048); rows S[s] * c0 + S[s + 1] * c1 in int32; columns
    (((b0 * (R0 >> 4)) >> 16) + ((b1 * (R1 >> 4)) >> 16) + 2) >> 2.
tests/test_maskgen_cpu.py checks the filters against scipy.ndimage and the resize against a float formulation.

`cv2_standin()` packages them as the `cv2` the reference's transforms import; tests/golden/make_maskgen_golden.py runs the reference's own
classes over it, which pins the draw order and the glue (tests/golden/maskgen_pinned.npz), not OpenCV. The table-level operators
(`binarize_morph`, `downup`, `cut`, `stats`, `drop`, `chain`) restate the same chain from a `MaskDraws`-shaped record: what the device
computes. The seeded inputs of the fixture are regenerated here: it stores outputs only."""
import types

import numpy as np

import groundtruth_restatement as G

ORDERS = ('dilate_erode', 'erode_dilate', 'dilate', 'erode')
THRESH_BINARY, INTER_NEAREST, INTER_LINEAR = 0, 0, 1


# ---- OpenCV, restated ----------------------------------------------------------------------------------------------------------------------------
def threshold(src, thresh, maxval, kind=THRESH_BINARY):
    assert kind == THRESH_BINARY and np.asarray(src).dtype == np.uint8
    return thresh, np.where(np.asarray(src) > int(np.floor(thresh)), np.uint8(maxval), np.uint8(0)).astype(np.uint8)


def rect_dilate(src, k):
    return G.dilate(src, np.ones((int(k), int(k)), np.uint8))


def rect_erode(src, k):
    return G.erode(src, np.ones((int(k), int(k)), np.uint8))


def resize_axis(src, dst, scale):
    """One axis, index by index: (ofs, c0, c1) lists."""
    ofs, c0, c1 = [], [], []
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(f))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0)
        ofs.append(s)
        c0.append(int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048))))
        c1.append(int(np.rint(np.float32(f * np.float32(2048)))))
    return np.asarray(ofs, np.int64), np.asarray(c0, np.int32), np.asarray(c1, np.int32)


def resize_geometry(H, W, dsize=(0, 0), fx=0.0, fy=0.0):
    """(dh, dw, scale_y, scale_x) of cv2.resize(src, dsize, fx=fx, fy=fy)."""
    if tuple(dsize) == (0, 0):
        dw, dh = int(np.rint(W * fx)), int(np.rint(H * fy))
        sx, sy = 1.0 / fx, 1.0 / fy
    else:
        dw, dh = int(dsize[0]), int(dsize[1])
        sx, sy = (1.0 / (dw / W), 1.0 / (dh / H)) if dw > 0 and dh > 0 else (0.0, 0.0)
    if dw <= 0 or dh <= 0:
        raise ValueError('resize: destination size %d x %d' % (dh, dw))
    return dh, dw, sy, sx


def resize(src, dsize=(0, 0), dst=None, fx=0.0, fy=0.0, interpolation=INTER_LINEAR):
    """cv2.resize of one uint8 plane with INTER_LINEAR. (GenMaskFromAlpha passes INTER_NEAREST in the `dst` position of a same-size call: the
    interpolation stays linear, and a same-size linear resize is a copy.)"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and interpolation == INTER_LINEAR
    H, W = src.shape
    dh, dw, sy, sx = resize_geometry(H, W, dsize, fx, fy)
    xo, a0, a1 = resize_axis(W, dw, sx)
    yo, b0, b1 = resize_axis(H, dh, sy)
    S = src.astype(np.int32)
    rows = S[:, xo] * a0[None] + S[:, np.minimum(xo + 1, W - 1)] * a1[None]                   # (H, dw) int32
    R0, R1 = rows[yo], rows[np.minimum(yo + 1, H - 1)]
    out = (((b0[:, None] * (R0 >> 4)) >> 16) + ((b1[:, None] * (R1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_float(src, dsize=(0, 0), fx=0.0, fy=0.0):
    """The same bilinear chain in float64 with exact weights (no fixed point, no rounding): the independent formulation."""
    src = np.asarray(src, np.float64)
    H, W = src.shape
    dh, dw, sy, sx = resize_geometry(H, W, dsize, fx, fy)

    def axis(n_src, n_dst, scale):
        f = (np.arange(n_dst) + 0.5) * scale - 0.5
        s = np.floor(f)
        f = f - s
        f = np.where((s < 0) | (s >= n_src - 1), 0.0, f)
        s = np.clip(s, 0, n_src - 1).astype(np.int64)
        return s, np.minimum(s + 1, n_src - 1), f
    x0, x1, fxs = axis(W, dw, sx)
    y0, y1, fys = axis(H, dh, sy)
    rows = src[:, x0] * (1 - fxs)[None] + src[:, x1] * fxs[None]
    return rows[y0] * (1 - fys)[:, None] + rows[y1] * fys[:, None]


def cv2_standin():
    """The `cv2` module the reference's mask transforms need: threshold, dilate, erode, resize and the constants they name."""
    cv2 = types.ModuleType('cv2')
    cv2.THRESH_BINARY, cv2.INTER_NEAREST, cv2.INTER_LINEAR = THRESH_BINARY, INTER_NEAREST, INTER_LINEAR
    cv2.threshold = threshold
    cv2.dilate = lambda src, kernel, iterations=1: G.dilate(src, np.asarray(kernel), iterations)
    cv2.erode = lambda src, kernel, iterations=1: G.erode(src, np.asarray(kernel), iterations)
    cv2.resize = resize
    return cv2


# ---- the chain from a table of draws (what the device computes) ----------------------------------------------------------------------------------
def binarize_morph(plane, thr, k_dilate, k_erode, order):
    """transforms.py:393-424 with the threshold already floored; `order`: a name, its index, or 4 for the threshold alone."""
    order = ORDERS[order] if isinstance(order, (int, np.integer)) and order < 4 else order
    b = (np.asarray(plane) > int(thr)).astype(np.uint8)
    if order == 'dilate_erode':
        b = rect_erode(rect_dilate(b, k_dilate), k_erode)
    elif order == 'erode_dilate':
        b = rect_dilate(rect_erode(b, k_erode), k_dilate)
    elif order == 'dilate':
        b = rect_dilate(b, k_dilate)
    elif order == 'erode':
        b = rect_erode(b, k_erode)
    else:
        assert order == 4
    return b * np.uint8(255)


def downup(plane, ratio=0.125):
    """transforms.py:488-491."""
    h, w = plane.shape
    small = resize(plane, (0, 0), fx=ratio, fy=ratio)
    back = resize(small, (w, h))
    return (back > 127).astype(np.uint8) * np.uint8(255)


def cut(planes, rects):
    """rects (P, 8): (src_plane, dst_row, dst_col, src_row, src_col, h, w, 0); every source is read before anything is written."""
    src = np.array(planes, copy=True)
    out = np.array(planes, copy=True)
    for p, (sp, dr, dc, sr, sc, h, w, _) in enumerate(np.asarray(rects).tolist()):
        if sp >= 0:
            out[p, dr:dr + h, dc:dc + w] = src[sp, sr:sr + h, sc:sc + w]
    return out


def stats(planes):
    """(P, 5): (count, xmin, xmax, ymin, ymax) of planes > 0; an empty plane gives (0, W, -1, H, -1)."""
    out = []
    for m in planes:
        ys, xs = np.where(m > 0)
        out.append((len(ys), xs.min(), xs.max(), ys.min(), ys.max()) if len(ys) else (0, m.shape[1], -1, m.shape[0], -1))
    return np.asarray(out, np.int32).reshape(len(planes), 5)


def drop(planes, selection, st):
    """transforms.py:550-563 for the entries (plane, idx, ph, pw) of `selection`."""
    out = np.array(planes, copy=True)
    for i, idx, ph, pw in np.asarray(selection).reshape(-1, 4).tolist():
        if i < 0:
            continue
        ys, xs = np.where(planes[i] > 0)
        x, y = int(xs[idx]), int(ys[idx])
        x = min(x, int(st[i][2]) - pw)
        y = min(y, int(st[i][4]) - ph)
        out[i, y:y + ph, x:x + pw] = 0
    return out


def chain(planes, draws, selection=None):
    """The whole chain for (P, H, W) uint8 planes from a MaskDraws-shaped record (host arrays `morph`, `downup`, `cut`, `ratio`) and, for the
    drop-out, the (n, 4) selection `draw_dropout` made from `stats` of the result so far."""
    m = np.stack([binarize_morph(pl, *row) for pl, row in zip(planes, np.asarray(draws.morph).tolist())])
    m = np.stack([downup(pl, draws.ratio) if a else pl for pl, a in zip(m, np.asarray(draws.downup).tolist())])
    m = cut(m, draws.cut)
    if selection is not None:
        m = drop(m, selection, stats(m))
    return m


def from_alpha(alphas, down_up=True, ratio=0.125):
    m = ((np.asarray(alphas) > 127) * 255).astype(np.uint8)
    return np.stack([downup(pl, ratio) for pl in m]) if down_up else m


# ---- seeded inputs (regenerated, never stored) ---------------------------------------------------------------------------------------------------
def blob_planes(seed, n, H, W, small=()):
    """(n, H, W) uint8 soft ellipses (groundtruth_restatement.soft_planes); the planes named in `small` hold a 10 x 12 soft dot instead --
    a bounding box under 16 pixels, which MaskDropout's size test skips."""
    a = G.soft_planes(seed, n, H, W)
    for p in small:
        a[p] = 0
        a[p, H // 2 - 5:H // 2 + 5, W // 3 - 6:W // 3 + 6] = 200
    return a


def noisy_ellipse(seed, H, W, salt=0.02):
    """A filled ellipse with `salt` of its pixels flipped: the input of the resize comparison."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((((yy - 0.45 * H) / (0.3 * H)) ** 2 + ((xx - 0.55 * W) / (0.35 * W)) ** 2) <= 1)
    return ((m ^ (rng.random((H, W)) < salt)) * 255).astype(np.uint8)


# the cases of tests/golden/maskgen_pinned.npz: input planes, the RandomState seed of the loader and the seed of Python's `random`
GOLDEN = {
    # him.py:50-54 (image training): the alphas go in as masks; RandomBinarizedMask -> DownUpMask -> CutMask
    'image_internal': dict(seed=518, n=3, H=96, W=160, rs_seed=18, py_seed=19, max_k=30, p=0.5, video=False),      # internal cut, overlapping
    'image_plain': dict(seed=509, n=3, H=96, W=160, rs_seed=9, py_seed=10, max_k=30, p=0.5, video=False),          # no cut at all
    # vim.py:58-66 (video training): GenMaskFromAlpha first, MaskDropout last; plane 2 is too small for the drop-out's size test
    'video': dict(seed=523, n=8, H=96, W=160, small=(2,), rs_seed=23, py_seed=24, max_k=30, p=0.5, video=True),    # external cut, drop-out
}


def golden_inputs(name):
    c = GOLDEN[name]
    return blob_planes(c['seed'], c['n'], c['H'], c['W'], c.get('small', ()))
