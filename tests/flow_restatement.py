"""Dense Farneback flow (Farneback 2003, structured as OpenCV's calcOpticalFlowFarneback structures it) and the MESSDdt reduction of the
reference's maggie/utils/metric.py:450-531 in plain NumPy: what csrc/flow.hip is held against (tests/test_gpu_flow.py) and what
tests/golden/make_flow_golden.py holds against an independent scipy.ndimage statement (flow) and the reference's own code (reduction).

The parameters are the reference's call (metric.py:453-455): pyr_scale 0.5, levels 5, winsize 10, iterations 2, poly_n 7, poly_sigma 1.5, the
Gaussian window, no initial flow. `dtype` selects the arithmetic: fp32 is what OpenCV and the device compute in, fp64 is the yardstick.
NOT compared with cv2.calcOpticalFlowFarneback (cv2 is not part of this build): DESIGN.md section 23 lists what is taken on trust."""
import numpy as np

PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA, MIN_SIZE = 0.5, 5, 10, 2, 7, 1.5, 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)


# ---- the pyramid -------------------------------------------------------------------------------------------------------------------------------------
def levels_of(h, w):
    scale, k = 1.0, 0
    while k < LEVELS:
        scale *= PYR_SCALE
        if w * scale < MIN_SIZE or h * scale < MIN_SIZE:
            break
        k += 1
    return k


def level_size(h, w, k):
    """(rows, columns) of pyramid level k: half-even rounding of the scaled size."""
    scale = PYR_SCALE ** k
    return int(round(h * scale)), int(round(w * scale))


def smooth_size(k):
    sigma = (1.0 / PYR_SCALE ** k - 1.0) * 0.5
    return sigma, max(int(round(5 * sigma)) | 1, 3)


def gauss_taps(n, sigma):
    """Normalised exp(-x^2 / 2 sigma^2) on n taps, in fp64; [1/4, 1/2, 1/4] for sigma 0 (n is 3 there)."""
    if sigma <= 0:
        assert n == 3
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(n, dtype=np.float64) - (n - 1) / 2
    g = np.exp(-x * x / (2.0 * sigma * sigma))
    return g / g.sum()


def corr(img, taps, axis, mode):
    """Correlation along one axis of (..., H, W), taps added in index order; mode 'reflect' (reflect-101) or 'edge' (replicate)."""
    r = len(taps) // 2
    n = img.shape[axis]
    pad = [(0, 0)] * img.ndim
    pad[axis] = (r, r)
    p = np.pad(img, pad, mode=mode)
    out = np.zeros_like(img)
    sl = [slice(None)] * img.ndim
    for i, t in enumerate(taps):
        sl[axis] = slice(i, i + n)
        out += img.dtype.type(t) * p[tuple(sl)]
    return out


def resize_taps(n_src, n_dst, dtype):
    """Left tap, right tap and right weight of a bilinear resize: pixel centres (i + 1/2) s - 1/2, taps clamped, weight 0 where the left one is."""
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5).astype(dtype)
    i0 = np.floor(f).astype(np.int64)
    w = f - i0.astype(dtype)
    lo, hi = i0 < 0, i0 >= n_src - 1
    w[lo | hi] = 0
    i0[lo] = 0
    i0[hi] = n_src - 1
    return i0, np.minimum(i0 + 1, n_src - 1), w


def resize(img, h, w):
    """Bilinear resize of (..., H, W) to (..., h, w): columns first, then rows."""
    dt = img.dtype
    x0, x1, wx = resize_taps(img.shape[-1], w, dt)
    t = img[..., x0] * (1 - wx) + img[..., x1] * wx
    y0, y1, wy = resize_taps(img.shape[-2], h, dt)
    wy = wy[:, None]
    return t[..., y0, :] * (1 - wy) + t[..., y1, :] * wy


def level_image(u8, k, dtype):
    H, W = u8.shape[-2:]
    sigma, n = smooth_size(k)
    g = gauss_taps(n, sigma).astype(dtype)
    img = corr(corr(u8.astype(dtype), g, -1, 'reflect'), g, -2, 'reflect')          # rows (horizontal) first, then columns
    return resize(img, *level_size(H, W, k))


# ---- polynomial expansion ----------------------------------------------------------------------------------------------------------------------------
def poly_setup():
    """g, x g, x^2 g on +-POLY_N and the four entries of the inverse Gram matrix of (1, x, y, x^2, y^2, xy) under g (x) g, in fp64."""
    x = np.arange(-POLY_N, POLY_N + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * POLY_SIGMA * POLY_SIGMA))
    g /= g.sum()
    X, Y = np.meshgrid(x, x)
    basis = [np.ones_like(X), X, Y, X * X, Y * Y, X * Y]
    w = np.outer(g, g)
    G = np.array([[(w * a * b).sum() for b in basis] for a in basis])
    ig = np.linalg.inv(G)
    return g, x * g, x * x * g, (ig[1, 1], ig[0, 3], ig[3, 3], ig[5, 5])


def polyexp(img):
    """(..., H, W) -> (..., 5, H, W): b_x, b_y, A_xx, A_yy, A_xy. Columns (vertical) first, then rows; replicate border."""
    dt = img.dtype
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_setup()
    g, xg, xxg = g.astype(dt), xg.astype(dt), xxg.astype(dt)
    ig11, ig03, ig33, ig55 = (dt.type(v) for v in (ig11, ig03, ig33, ig55))
    v0, v1, v2 = corr(img, g, -2, 'edge'), corr(img, xg, -2, 'edge'), corr(img, xxg, -2, 'edge')
    s = corr(v0, g, -1, 'edge')
    return np.stack([ig11 * corr(v0, xg, -1, 'edge'), ig11 * corr(v1, g, -1, 'edge'), ig03 * s + ig33 * corr(v0, xxg, -1, 'edge'),
                     ig03 * s + ig33 * corr(v2, g, -1, 'edge'), ig55 * corr(v1, xg, -1, 'edge')], axis=-3)


# ---- matrices and the flow update -----------------------------------------------------------------------------------------------------------------
def border_scale(n, dtype):
    s = np.ones(n, dtype)
    for i in range(min(5, n)):
        s[i] *= dtype.type(BORDER[i])
        s[n - 1 - i] *= dtype.type(BORDER[i])
    return s


def matrices(R0, R1, flow):
    """R0, R1 (5, H, W), flow (H, W, 2) -> (5, H, W): G11, G12, G22, h1, h2."""
    dt = R0.dtype
    H, W = R0.shape[-2:]
    dx, dy = flow[..., 0], flow[..., 1]
    fx = np.arange(W, dtype=dt)[None, :] + dx
    fy = np.arange(H, dtype=dt)[:, None] + dy
    x1, y1 = np.floor(fx), np.floor(fy)
    fx, fy = fx - x1, fy - y1
    x1, y1 = x1.astype(np.int64), y1.astype(np.int64)
    inside = (x1 >= 0) & (x1 < W - 1) & (y1 >= 0) & (y1 < H - 1)
    xc, yc = np.clip(x1, 0, max(W - 2, 0)), np.clip(y1, 0, max(H - 2, 0))
    xn, yn = np.minimum(xc + 1, W - 1), np.minimum(yc + 1, H - 1)
    a00, a01, a10, a11 = (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy
    S = a00 * R1[:, yc, xc] + a01 * R1[:, yc, xn] + a10 * R1[:, yn, xc] + a11 * R1[:, yn, xn]
    half, quarter = dt.type(0.5), dt.type(0.25)
    bx = np.where(inside, (R0[0] - S[0]) * half, 0)
    by = np.where(inside, (R0[1] - S[1]) * half, 0)
    axx = np.where(inside, (R0[2] + S[2]) * half, R0[2])
    ayy = np.where(inside, (R0[3] + S[3]) * half, R0[3])
    axy = np.where(inside, (R0[4] + S[4]) * quarter, R0[4] * half)
    sc = border_scale(H, dt)[:, None] * border_scale(W, dt)[None, :]
    bx, by, axx, ayy, axy = bx * sc, by * sc, axx * sc, ayy * sc, axy * sc
    bx = bx + (axx * dx + axy * dy)
    by = by + (axy * dx + ayy * dy)
    return np.stack([axx * axx + axy * axy, (axx + ayy) * axy, ayy * ayy + axy * axy, axx * bx + axy * by, axy * bx + ayy * by])


def update_flow(M):
    dt = M.dtype
    m = WINSIZE // 2
    g = gauss_taps(2 * m + 1, 0.3 * m).astype(dt)
    B = corr(corr(M, g, -2, 'edge'), g, -1, 'edge')                  # columns first, then rows
    g11, g12, g22, h1, h2 = B
    idet = 1 / (g11 * g22 - g12 * g12 + dt.type(1e-3))
    return np.stack([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet], axis=-1)


def farneback(prev_u8, next_u8, dtype=np.float32):
    """One plane pair (H, W) uint8 -> flow (H, W, 2) in `dtype`: [..., 0] along columns (x), [..., 1] along rows (y); next(p + flow) ~ prev(p)."""
    dtype = np.dtype(dtype)
    H, W = prev_u8.shape
    flow = None
    for k in range(levels_of(H, W), -1, -1):
        h, w = level_size(H, W, k)
        if flow is None:
            flow = np.zeros((h, w, 2), dtype)
        else:
            flow = np.moveaxis(resize(np.moveaxis(flow, -1, 0), h, w), 0, -1) * dtype.type(1 / PYR_SCALE)
        R0, R1 = polyexp(level_image(prev_u8, k, dtype)), polyexp(level_image(next_u8, k, dtype))
        M = matrices(R0, R1, flow)
        for it in range(ITERATIONS):
            flow = update_flow(M)
            if it < ITERATIONS - 1:
                M = matrices(R0, R1, flow)
    return flow


# ---- the reduction ---------------------------------------------------------------------------------------------------------------------------------
def gt_u8(gt):
    """The planes the reference hands to cv2: one fp32 multiply, truncated (metric.py:465, :453)."""
    return (np.asarray(gt, np.float32) * np.float32(255)).astype(np.uint8)


def messddt(pred, gt, trimap, flows):
    """pred, gt, trimap (or None) fp32 (F, N, H, W), flows (F-1, N, H, W, 2) of integers -> (score, count) of one update() as metric.py:458-531
    computes them: pixel (i, j) of pair t reads its warped sample of FRAME 1 at row clamp(j + fx, 0, H-1), column clamp(i + fy, 0, W-1)."""
    pred, gt = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    F, N, H, W = pred.shape
    mask = np.ones_like(gt) if trimap is None else (np.asarray(trimap) == 1).astype(np.float32)
    score, count = 0.0, 0
    if F < 2:
        return score, count
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    for n in range(N):
        err, num = 0.0, 0.0
        for t in range(F - 1):
            f = np.asarray(flows[t, n]).astype(np.int64)
            idx = np.clip(j + f[..., 0], 0, H - 1) * W + np.clip(i + f[..., 1], 0, W - 1)
            p1, g1, m1 = (a[1, n].reshape(-1)[idx] for a in (pred, gt, mask))
            e = (pred[t, n] - gt[t, n]) ** 2 * mask[t, n] - (p1 - g1) ** 2 * m1
            err += float(np.abs(e).astype(np.float64).sum())
            num += float(mask[t, n].astype(np.float64).sum()) + 1.0
        score += err / num * 10000
        count += 1
    return score, count


def messddt_restated(pred, gt, trimap, dtype=np.float64):
    """The whole metric: flow of the ground truth's uint8 planes in `dtype`, rounded half to even, then the reduction. Also returns the flows."""
    F, N, H, W = gt.shape
    u8 = gt_u8(gt)
    flows = np.zeros((max(F - 1, 0), N, H, W, 2), np.int64)
    for t in range(F - 1):
        for n in range(N):
            flows[t, n] = np.rint(farneback(u8[t, n], u8[t + 1, n], dtype)).astype(np.int64)
    return messddt(pred, gt, trimap, flows) + (flows,)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------------------
BLOBS = (2, 6, 20, 60)


ISSUE_SHIFT = (3.2, -2.1)        # the one shift the issue names whose fractional part (0.9) lies outside the band it states: 0.4 px from .5, kept as named


def check_shift(shift):
    """Every component that moves has its fractional part in [0.15, 0.35] u [0.65, 0.85]: 0.15 px from the rounding boundary at .5 and from
    the integers. A component of exactly 0 does not move; ISSUE_SHIFT is the named exception."""
    if tuple(shift) == ISSUE_SHIFT:
        return
    for v in shift:
        fr = round(v - np.floor(v), 9)
        assert v == 0 or 0.15 <= fr <= 0.35 or 0.65 <= fr <= 0.85, shift


def frames(h, w, shifts, seed):
    """uint8 (h, w) frames of one pattern moved by each of `shifts` = (dx, dy) px: band-limited noise summed over blob sizes of 2, 6, 20 and
    60 px (curvature at every pyramid scale), stretched to 0..255 with about 1 % saturated. The move is a Fourier shift of the periodic
    pattern, so sub-pixel amounts are exact: frame(x, y) = pattern(x - dx, y - dy)."""
    rng = np.random.default_rng(seed)
    fy, fx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
    spec = np.zeros((h, w), np.complex128)
    for b in BLOBS:
        s = b / 2.0
        band = np.fft.fft2(rng.standard_normal((h, w))) * np.exp(-2 * (np.pi * s) ** 2 * (fx * fx + fy * fy))
        spec += band / np.sqrt((np.abs(band) ** 2).sum())
    lo, hi = np.percentile(np.fft.ifft2(spec).real, [0.5, 99.5])
    out = []
    for dx, dy in shifts:
        a = np.fft.ifft2(spec * np.exp(-2j * np.pi * (fx * dx + fy * dy))).real
        out.append(np.clip(np.rint((a - lo) / (hi - lo) * 255), 0, 255).astype(np.uint8))
    return out


def frame_pair(h, w, shift, seed):
    """(prev, next) of `frames`: next(x, y) = prev(x - dx, y - dy) for shift = (dx, dy)."""
    if shift[0] or shift[1]:
        check_shift(shift)
    return tuple(frames(h, w, [(0.0, 0.0), shift], seed))


# the flow cases of tests/test_gpu_flow.py and the fixture: name -> (h, w, shift (dx, dy), seed)
FLOW_CASES = {
    '40x36': (40, 36, (1.2, -0.8), 1),
    '131x150': (131, 150, (3.2, -2.1), 2),
    '131x150_still': (131, 150, (0.0, 0.0), 2),
    '9x11': (9, 11, (1.2, 0.8), 5),
    '1024x1031': (1024, 1031, (9.3, 6.2), 4),
}
BATCH_SHAPE = (70, 90)
BATCH_SHIFTS = ((1.2, 0.3), (-2.3, 1.8), (0.0, 0.0), (4.7, -3.2), (-0.8, -5.3))


def batch_pairs():
    prev, nxt = zip(*[frame_pair(BATCH_SHAPE[0], BATCH_SHAPE[1], s, 10 + i) for i, s in enumerate(BATCH_SHIFTS)])
    return np.stack(prev), np.stack(nxt)


def matte_clip(F, N, h, w, seed, trimap):
    """A (F, N, h, w) fp32 clip for the metric: gt planes k / 255 of a moving pattern, pred = gt plus noise, trimap in {0, 1, 2} or None."""
    rng = np.random.default_rng(seed)
    gt = np.empty((F, N, h, w), np.float32)
    for n in range(N):
        step = (1.7 + 0.6 * n, -1.3 + 1.1 * n)                                # px per frame; (2.3, -0.2) for n = 1
        check_shift(step)
        clip = frames(h, w, [(step[0] * t, step[1] * t) for t in range(F)], seed + n)
        gt[:, n] = np.stack(clip).astype(np.float32) / np.float32(255)
    pred = np.clip(gt + rng.normal(0, 0.1, gt.shape).astype(np.float32), 0, 1).astype(np.float32)
    tri = rng.integers(0, 3, gt.shape).astype(np.float32) if trimap else None
    return pred, gt, tri


# the reduction cases of the fixture (at most 48 x 64): name -> (F, N, H, W, trimap, largest |flow| component, seed)
REDUCTION_CASES = {
    'f4_n2_48x64_trimap_wild': (4, 2, 48, 64, True, 70, 21),           # flows that push the coordinates past both clamps
    'f2_n1_40x33': (2, 1, 40, 33, False, 4, 22),
    'f3_n2_8x32_all_values': (3, 2, 8, 32, False, 5, 23),              # every gt plane holds k / 255 for all 256 k
    'f3_n1_33x40_trimap': (3, 1, 33, 40, True, 9, 24),
    'f1_n2_16x20': (1, 2, 16, 20, False, 3, 25),                       # a single frame: nothing is added
}


def reduction_case(name):
    """pred, gt, trimap (or None) fp32 (F, N, H, W) and integer flows (F-1, N, H, W, 2) of a fixture case, from its seed."""
    F, N, H, W, trimap, reach, seed = REDUCTION_CASES[name]
    rng = np.random.default_rng(seed)
    if 'all_values' in name:
        assert H * W == 256
        gt = np.stack([rng.permutation(256) for _ in range(F * N)]).reshape(F, N, H, W).astype(np.float32) / np.float32(255)
    else:
        gt = rng.integers(0, 256, (F, N, H, W)).astype(np.float32) / np.float32(255)
    pred = np.clip(gt + rng.normal(0, 0.2, gt.shape), 0, 1).astype(np.float32)
    tri = rng.integers(0, 3, gt.shape).astype(np.float32) if trimap else None
    flows = rng.integers(-reach, reach + 1, (max(F - 1, 0), N, H, W, 2)).astype(np.int64)
    return pred, gt, tri, flows
