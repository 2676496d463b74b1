"""MotionBlur of the video loader restated in integer NumPy (maggie/dataloader/transforms.py:965-1034), written without the package under test:

  * `blur_plane`      the definition tap by tap (`sums_plane`, then `rhe`): out[y, x] = rhe( sum_k src[r101(y + dy_k, H), r101(x + dx_k, W)] / n ), with `r101` OpenCV's
                      BORDER_REFLECT_101 as its explicit loop and `rhe` round-half-to-even on the exact rational;
  * `reference_call`  the reference's `MotionBlur.__call__` line by line with the pixels left out and a stub where it calls `self.motion_aug`:
                      what it draws from the loader's RandomState, in which order, and when the kernel is made;
  * `KERNELS`, `SHAPES`, `inputs`   the cases tests/test_motion_cpu.py holds against scipy and tests/test_gpu_motion.py runs on the device.

tests/test_motion_cpu.py compares `blur_plane` with `scipy.ndimage.correlate(float64, mode='mirror')` (exact integer sums in fp64) followed by
`np.rint(S / n)` on every case, and with the fixture tests/golden/motion_pinned.npz that scipy wrote."""
import numpy as np

MAX_KSIZE, MAX_TAPS = 49, 49


def r101(p, length):
    """cv::borderInterpolate(p, len, BORDER_REFLECT_101): the loop, which runs more than once when the source is smaller than the reach."""
    if 0 <= p < length:
        return p
    if length == 1:
        return 0
    while p < 0 or p >= length:
        p = -p if p < 0 else 2 * (length - 1) - p
    return p


def offsets(kernel):
    """[(dy, dx)] of the non-zero entries of a square odd-sided kernel image from its anchor ksize // 2, in row-major order."""
    k = np.asarray(kernel)
    assert k.ndim == 2 and k.shape[0] == k.shape[1] and k.shape[0] % 2 == 1
    a = k.shape[0] // 2
    return [(int(y) - a, int(x) - a) for y, x in zip(*np.nonzero(k))]


def rhe(S, n):
    """round-half-to-even of S / n for integer arrays S >= 0 and an integer n >= 1, in integers."""
    S = np.asarray(S, np.int64)
    q, r = S // n, S % n
    return np.where(2 * r > n, q + 1, np.where(2 * r == n, q + (q & 1), q))


def sums_plane(src, offs):
    """The integer sums S of one (H, W) uint8 plane over the taps `offs`, tap by tap."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and len(offs) >= 1
    H, W = src.shape
    S = np.zeros((H, W), np.int64)
    for dy, dx in offs:
        ys = np.array([r101(y + dy, H) for y in range(H)])
        xs = np.array([r101(x + dx, W) for x in range(W)])
        S += src[np.ix_(ys, xs)]
    return S


def blur_plane(src, offs):
    """One (H, W) uint8 plane with the taps `offs`: the integer sum, then `rhe`."""
    return rhe(sums_plane(src, offs), len(offs)).astype(np.uint8)


def blur_planes(x, offs):
    """(..., H, W) uint8 planes, each on its own."""
    x = np.asarray(x)
    flat = x.reshape((-1,) + x.shape[-2:])
    return np.stack([blur_plane(p, offs) for p in flat]).reshape(x.shape) if flat.shape[0] else x.copy()


def blur_frames(x, offs):
    """(..., H, W, 3) uint8 frames: every colour channel is a plane (filter2D filters channels independently)."""
    x = np.asarray(x)
    return np.moveaxis(blur_planes(np.moveaxis(x, -1, -3), offs), -3, -1)


def clamped_offsets(table):
    """What the device makes of ANY int32 table: n clipped to 1..49, every offset to +-24."""
    t = np.asarray(table, np.int64)
    n = int(np.clip(t[0], 1, MAX_TAPS))
    return [(int(np.clip(t[2 + 2 * k], -24, 24)), int(np.clip(t[3 + 2 * k], -24, 24))) for k in range(n)]


def reference_call(random, p, motion_aug, bg=None):
    """`MotionBlur.__call__` (transforms.py:971-1019), its draws and its calls of `self.motion_aug` line by line; `motion_aug` is a stub."""
    if random.rand() > p:                                                   # :972
        return
    if random.uniform(0, 1) < 0.5 and bg is not None:                      # :980
        motion_aug()                                                        # :984
    else:
        if random.uniform(0, 1) < 0.9:                                     # :995
            motion_aug()                                                    # :1006
        if random.uniform(0, 1) < 0.3 and bg is not None:                  # :1019
            motion_aug()                                                    # :1023


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
def _line(ksize, x0, y0, x1, y1):
    k = np.zeros((ksize, ksize), np.uint8)
    steps = max(abs(x1 - x0), abs(y1 - y0))
    for i in range(steps + 1):
        t = i / steps if steps else 0.0
        k[int(np.floor(y0 + t * (y1 - y0) + 0.5)), int(np.floor(x0 + t * (x1 - x0) + 0.5))] = 1
    return k


def _single(ksize, y, x):
    k = np.zeros((ksize, ksize), np.uint8)
    k[y, x] = 1
    return k


# name -> the uint8 0 / 1 kernel image
KERNELS = {
    'k3_n2': _line(3, 0, 0, 1, 1),                  # n = 2: every odd sum is an exact tie
    'k49_diagonal': _line(49, 0, 0, 48, 48),        # n = 49, the whole reach in both directions
    'k49_horizontal': _line(49, 0, 24, 48, 24),
    'k49_vertical': _line(49, 24, 0, 24, 48),
    'k49_corner': _line(49, 0, 0, 2, 2),            # 3 pixels at offsets -24 .. -22: a halo on one side only
    'k11': _line(11, 1, 9, 8, 2),                   # n = 8, even
    'k13': _line(13, 0, 3, 12, 9),                  # n = 13, a shallow line
    'n1': _single(5, 0, 4),                         # one tap off the centre: a reflected shift
}
assert [int(k.sum()) for k in KERNELS.values()] == [2, 49, 49, 49, 3, 8, 13, 1]

TILE_ROWS, TILE_COLS = 32, 64                       # MG_MOTION_TILE_ROWS / _TILE_COLS; tests/test_gpu_motion.py holds them against mg_motion_limits
# smaller than the reach (several reflections); one tile; one pixel over a tile in each direction; more than two tiles wide with w and 3 w no
# multiples of 4
SHAPES = [(1, 1), (1, 9), (2, 3), (5, 7), (TILE_ROWS, TILE_COLS), (TILE_ROWS + 1, TILE_COLS + 1), (9, 2 * TILE_COLS + 3)]
KINDS = ('random', 'white', 'checker')


def inputs(h, w, kind, seed, channels=0):
    """A (h, w) plane or (h, w, channels) image: random bytes, all 255 (the accumulator's width at n = 49), or a 0 / 255 checkerboard."""
    shape = (h, w) + ((channels,) if channels else ())
    if kind == 'random':
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if kind == 'white':
        return np.full(shape, 255, np.uint8)
    assert kind == 'checker'
    board = (((np.arange(h)[:, None] + np.arange(w)[None, :]) & 1) * 255).astype(np.uint8)
    return board if not channels else np.repeat(board[..., None], channels, -1)


def case_frames(h, w):
    """(3, h, w, 3): one frame of each kind."""
    return np.stack([inputs(h, w, kind, 1000 * h + w + i, 3) for i, kind in enumerate(KINDS)])


def case_planes(h, w):
    """(7, h, w): five random planes, a white one, a checkerboard."""
    return np.stack([inputs(h, w, 'random', 7000 * h + w + i) for i in range(5)] + [inputs(h, w, 'white', 0), inputs(h, w, 'checker', 0)])

