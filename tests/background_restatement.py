"""NumPy restatement of the background chain (maggie/dataloader/transforms.py:307-370,841-864) the device kernels of csrc/background.hip are
compared with: LoadRandomBackground's draws, blur and window, HistogramMatching, ComposeBackground. Pure host code, no GPU, no OpenCV, no skimage.

  * the blur is the integer statement the project defines (taps of 8 fractional bits, 16-bit and 32-bit sums, (s + 32768) >> 16,
    BORDER_REFLECT_101); tests/test_background_cpu.py bounds it against scipy's fp64 correlation;
  * the histogram matching is stated twice: `match_unique`, the float branch of skimage's published algorithm on the float32 frames
    (np.unique -> cumsum / size -> np.interp), and `match_table`, the 256-entry table from bincounts with np.interp's rule written out;
  * the composite is stated twice: `compose_literal`, the reference's expression on float32 frames, and `compose_table` through the (256, 2)
    weights table."""
import numpy as np

KERNEL_SIZES, SIGMAS = (5, 15, 25), (1.0, 1.5, 3.0, 5.0)
PAIRS = [(ks, s) for ks in KERNEL_SIZES for s in SIGMAS]


# ---- draws ------------------------------------------------------------------------------------------------------------------------------------
def window_calls(random, bg_hw, frame_hw, blur_p=0.5, sizes=KERNEL_SIZES, sigmas=SIGMAS):
    """The sequence of calls on the RandomState behind the file's choice: (ksize, sigma) or None, x, y."""
    blur = None
    if random.rand() < blur_p:
        ks = random.choice(sizes)
        blur = (int(ks), float(random.choice(sigmas)))
    x = random.randint(0, bg_hw[1] - frame_hw[1])
    y = random.randint(0, bg_hw[0] - frame_hw[0])
    return blur, int(x), int(y)


def histmatch_calls(random, p=0.3):
    """None when the step does not fire, else (ratio, match_bg)."""
    if random.rand() > p:
        return None
    ratio = random.uniform(0, 0.5)
    return float(ratio), bool(random.rand() < 0.05)


# ---- blur -------------------------------------------------------------------------------------------------------------------------------------
def float_taps(ks, sigma):
    """cv2.getGaussianKernel's formula for sigma > 0, in fp64."""
    i = np.arange(ks, dtype=np.float64) - (ks - 1) / 2
    k = np.exp(-(i ** 2) / (2 * sigma ** 2))
    return k / k.sum()


def taps(ks, sigma):
    q = np.rint(256 * float_taps(ks, sigma)).astype(np.int64)
    q[ks // 2] += 256 - q.sum()
    return q


def r101(p, n):
    """BORDER_REFLECT_101 of index array p on a side of n, repeated for sides below the reach; 0 for n == 1."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    m = np.mod(p, 2 * (n - 1))
    return np.where(m < n, m, 2 * (n - 1) - m)


def blur(bg, q):
    """The integer blur of the whole (H, W, 3) uint8 background with taps q."""
    H, W = bg.shape[:2]
    R = len(q) // 2
    src = bg.astype(np.int64)
    s1 = np.zeros_like(src)
    for k, qk in enumerate(q):
        s1 += int(qk) * src[:, r101(np.arange(W) + k - R, W)]
    assert s1.max() <= 255 * 256
    s2 = np.zeros_like(src)
    for k, qk in enumerate(q):
        s2 += int(qk) * s1[r101(np.arange(H) + k - R, H)]
    return ((s2 + 32768) >> 16).astype(np.uint8)


def window(bg, q, x, y, h, w):
    out = bg if q is None else blur(bg, q)
    return np.ascontiguousarray(out[y:y + h, x:x + w])


def clamped_window(bg, table, h, w):
    """What the device makes of a win table that holds anything."""
    bh, bw = bg.shape[:2]
    ks = min(max(int(table[0]), 1), 25) | 1
    x, y = min(max(int(table[1]), 0), bw - w), min(max(int(table[2]), 0), bh - h)
    return window(bg, np.clip(np.asarray(table[4:4 + ks], np.int64), 0, 256), x, y, h, w)


# ---- histogram matching -----------------------------------------------------------------------------------------------------------------------
def match_unique(source, template):
    """One channel, float32 arrays of any shape: the float branch of the published algorithm. Returns float64 values in source's shape."""
    values, inverse, counts = np.unique(source.reshape(-1), return_inverse=True, return_counts=True)
    t_values, t_counts = np.unique(template.reshape(-1), return_counts=True)
    q = np.cumsum(counts) / source.size
    t_q = np.cumsum(t_counts) / template.size
    return np.interp(q, t_q, t_values)[inverse.reshape(-1)].reshape(source.shape)


def histmatch_literal(fg_u8, bg_u8, ratio, match_bg):
    """HistogramMatching on the float32 copies of (T, H, W, 3) frames and a tiled (T, H, W, 3) background: the matched uint8 fg and bg."""
    fg, bg = fg_u8.astype(np.float32), bg_u8.astype(np.float32)
    src, tmpl = (bg, fg) if match_bg else (fg, bg)
    matched = np.empty(src.shape, dtype=src.dtype)
    for c in range(3):
        matched[..., c] = match_unique(src[..., c], tmpl[..., c])
    blended = matched * ratio + src * (1. - ratio)
    assert blended.dtype == np.float32
    if match_bg:
        bg = blended
    else:
        fg = blended
    return fg.astype(np.uint8), bg.astype(np.uint8)


def interp_written_out(x, xp, fp):
    """np.interp's rule, element by element in fp64, every operation rounded on its own."""
    out = np.empty(len(x), np.float64)
    n = len(xp)
    for i, xv in enumerate(x):
        if n == 1 or xv < xp[0]:
            out[i] = fp[0]
        elif xv > xp[-1]:
            out[i] = fp[-1]
        else:
            j = int(np.searchsorted(xp, xv, side='right')) - 1
            if j == n - 1 or xp[j] == xv:
                out[i] = fp[j]
            else:
                slope = np.float64(fp[j + 1] - fp[j]) / np.float64(xp[j + 1] - xp[j])
                prod = np.float64(slope * np.float64(xv - xp[j]))
                out[i] = prod + fp[j]
    return out


def match_table(counts_src, counts_tmpl, ratio):
    """One channel: the 256-entry uint8 curve from the two 256-bin counts; bins the source does not hold are the identity."""
    counts_src, counts_tmpl = np.asarray(counts_src, np.int64), np.asarray(counts_tmpl, np.int64)
    occ_s, occ_t = np.nonzero(counts_src)[0], np.nonzero(counts_tmpl)[0]
    q = np.cumsum(counts_src[occ_s]) / int(counts_src.sum())
    t_q = np.cumsum(counts_tmpl[occ_t]) / int(counts_tmpl.sum())
    m32 = interp_written_out(q, t_q, occ_t.astype(np.float64)).astype(np.float32)
    blended = m32 * np.float32(ratio) + occ_s.astype(np.float32) * np.float32(1. - ratio)
    assert blended.dtype == np.float32
    lut = np.arange(256, dtype=np.uint8)
    lut[occ_s] = blended.astype(np.uint8)
    return lut


def counts_of(frames_u8):
    """(3, 256) counts of (..., 3) uint8 frames."""
    flat = frames_u8.reshape(-1, 3)
    return np.stack([np.bincount(flat[:, c], minlength=256) for c in range(3)])


def luts(fg_u8, bg_u8, hist):
    """(2, 3, 256) uint8: the foreground's curves and the background's; `hist` = None or (ratio, match_bg)."""
    out = np.broadcast_to(np.arange(256, dtype=np.uint8), (2, 3, 256)).copy()
    if hist is not None:
        ratio, match_bg = hist
        cf, cb = counts_of(fg_u8), counts_of(bg_u8)
        for c in range(3):
            out[1 if match_bg else 0, c] = match_table(cb[c], cf[c], ratio) if match_bg else match_table(cf[c], cb[c], ratio)
    return out


def apply_luts(x_u8, lut3):
    return np.stack([lut3[c][x_u8[..., c]] for c in range(3)], axis=-1)


# ---- composite --------------------------------------------------------------------------------------------------------------------------------
def compose_literal(fg_u8, alphas_u8, bg_u8):
    """The reference's expression; bg (H, W, 3) or fg's shape."""
    fg, bg = fg_u8.astype(np.float32), np.broadcast_to(bg_u8, fg_u8.shape).astype(np.float32)
    a = alphas_u8[..., None].astype(float) / 255.0
    return np.clip(fg * a + bg * (1 - a), 0, 255).astype(np.uint8)


def weights():
    a = np.arange(256).astype(float) / 255.0
    return np.stack([a, 1 - a], axis=1)


def compose_table(fg_u8, alphas_u8, bg_u8, wt=None):
    wt = weights() if wt is None else wt
    s = fg_u8.astype(np.float64) * wt[alphas_u8, 0][..., None] + np.broadcast_to(bg_u8, fg_u8.shape).astype(np.float64) * wt[alphas_u8, 1][..., None]
    return np.clip(s, 0, 255).astype(np.uint8)


# ---- the chain --------------------------------------------------------------------------------------------------------------------------------
def chain(fg_u8, alphas_u8, bg_full_u8, blur_draw, x, y, hist):
    """frames, matched fg, matched window of one item: fg (T, H, W, 3), alphas (T, H, W), the decoded background, the draws."""
    T, h, w = alphas_u8.shape
    win = window(bg_full_u8, None if blur_draw is None else taps(*blur_draw), x, y, h, w)
    fg, bg = fg_u8, win
    if hist is not None:
        fg, tiled = histmatch_literal(fg_u8, np.tile(win, (T, 1, 1, 1)), *hist)
        bg = tiled[0]
        assert all(np.array_equal(t, bg) for t in tiled)
    return compose_literal(fg, alphas_u8, bg), fg, bg


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------
def image(h, w, seed, kind='noise'):
    """A deterministic (h, w, 3) uint8 image: noise, a smooth ramp with noise, or a narrow band of values."""
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'band':
        return rng.integers(90, 131, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = (yy * 3 + xx * 2)[..., None] + np.array([0, 40, 90])
    return ((ramp + rng.integers(0, 30, (h, w, 3))) % 256).astype(np.uint8)


def clip(T, h, w, seed, kind='ramp'):
    return np.stack([image(h, w, seed + 17 * t, kind) for t in range(T)])


def alphas(T, h, w, seed):
    """Alphas with runs of 0 and 255 and a soft part."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (T, h, w), dtype=np.uint8)
    a[rng.random((T, h, w)) < 0.3] = 0
    a[rng.random((T, h, w)) < 0.3] = 255
    return a


# the cases of the curve tests: name -> (source values, template values) per channel, as flat uint8 arrays
def curve_cases():
    rng = np.random.default_rng(5)
    n = 600
    cases = {
        'source_one_value': (np.full(n, 77, np.uint8), rng.integers(0, 256, n, dtype=np.uint8)),
        'template_one_value': (rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 200, np.uint8)),
        'source_brighter': (rng.integers(180, 256, n, dtype=np.uint8), rng.integers(0, 60, n, dtype=np.uint8)),
        'source_darker': (rng.integers(0, 60, n, dtype=np.uint8), rng.integers(180, 256, n, dtype=np.uint8)),
        'disjoint': (rng.choice(np.arange(0, 256, 2), n).astype(np.uint8), rng.choice(np.arange(1, 256, 2), n).astype(np.uint8)),
        'few_against_many': (rng.choice([3, 90, 250], n).astype(np.uint8), rng.integers(0, 256, n, dtype=np.uint8)),
        'many_against_few': (rng.integers(0, 256, n, dtype=np.uint8), rng.choice([3, 90, 250], n).astype(np.uint8)),
        'sizes_differ': (rng.integers(0, 256, n, dtype=np.uint8), rng.integers(20, 230, 3 * n + 1, dtype=np.uint8)),
    }
    same = rng.integers(0, 256, n, dtype=np.uint8)
    cases['equal'] = (same, same.copy())
    return cases
