"""MotionBlur of the video loader on the device (HIP kernel of csrc/motion.hip) -- the step the reference runs between GammaContrast and
AdditiveGaussionNoise of a video training item (maggie/dataloader/transforms.py:965-1034, vim.py:49-55):

  RandomCropByAlpha -> RandomHorizontalFlip -> GammaContrast -> MotionBlur -> AdditiveGaussionNoise -> JpegCompression -> RandomAffine

  * `taps_of`       a kernel image (the uint8 0 / 1 line, or the normalised float kernel) -> the int32 table the device reads;
  * `MotionDraws`   one item's draw: the table, or nothing when the blur did not fire;
  * `draw`          the reference's calls on the loader's `np.random.RandomState`, in its order (pure host code); the kernel itself comes from
                    the caller's `kernel_fn` (albumentations' generator);
  * `line_kernel`, `draw_kernel`   a stand-in for that generator for callers without OpenCV;
  * `apply`         the blur of the frames and the alpha planes of one item with one table; `blur_frames`, `blur_planes` the single-tensor forms.

The kernel albumentations draws is a ksize x ksize image (ksize odd, 3..49) with one 8-connected line of ones, divided by its sum: n <= 49
taps of weight 1 / n. Every plane (each colour channel of each frame, each alpha plane; `filter2D` filters channels independently) is

  out[y, x] = rhe( sum_k src[r101(y + dy_k, H), r101(x + dx_k, W)] / n )

with (dy_k, dx_k) the offsets of the non-zero entries from the anchor ksize // 2 (correlation, no flip), r101 OpenCV's BORDER_REFLECT_101
(0 for a length of 1, repeated for sources smaller than the reach) and rhe round-half-to-even of the exact rational: the integer sum S, q = S // n,
r = S % n, q + 1 if 2 r > n, q + (q & 1) if 2 r == n, else q. This is the correctly rounded value of what both float paths of `cv2.filter2D`
approximate. Away from exact ties it is what any correct float evaluation rounds to; an exact tie needs an even n, and there OpenCV's answer
depends on fl32(1 / n) and on which of its two code paths runs (direct below 13 x 13, DFT from there), while this rounds to even; a difference
is one grey level. No comparison with OpenCV was run: it is not a dependency and not installed where this was written.

A `MotionDraws` moved to the device (`.to(device)`) makes `apply` upload nothing and never synchronise, so it can be captured in a graph and a
new table written into `draws.taps` between replays: the launch does not depend on the table's contents, and the kernel clamps n to 1..49 and
every offset to +-24. Wrong dtype, rank, size or table raise before anything touches the device. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import photometric
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, images, int_table, integer, resolve_device, to_device, upload
from .photometric import NORM, RAW                                          # MG_PHOTO_RAW / MG_PHOTO_NORM: the one pair of epilogue constants

MAX_KSIZE, MAX_TAPS = 49, 49               # MG_MOTION_MAX_KSIZE / _MAX_TAPS (include/maggie_hip.h)
TABLE = 2 + 2 * MAX_TAPS                   # MG_MOTION_TABLE
TILE_ROWS, TILE_COLS, MAX_SIDE = 32, 64, 32767                              # MG_MOTION_TILE_ROWS / _TILE_COLS / _MAX_SIDE


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------
def taps_of(kernel):
    """The int32 [TABLE] table of a kernel image: [0] = n, [1] = ksize, then the n (dy, dx) offsets of the non-zero entries from the anchor
    ksize // 2 in row-major order, zeros after them. `kernel`: a square array, odd-sided, 3..49 a side, whose non-zero entries are all equal --
    the uint8 0 / 1 line image or the float kernel divided by its sum. 1..49 taps; ValueError otherwise."""
    k = np.asarray(kernel)
    if k.ndim != 2 or k.shape[0] != k.shape[1]:
        raise ValueError('the kernel must be a square 2-D array (got shape %s)' % (k.shape,))
    ksize = int(k.shape[0])
    if ksize % 2 == 0 or not 3 <= ksize <= MAX_KSIZE:
        raise ValueError('the kernel side must be odd and in 3..%d (got %d)' % (MAX_KSIZE, ksize))
    if k.dtype == np.bool_:
        k = k.astype(np.uint8)
    if not (np.issubdtype(k.dtype, np.integer) or np.issubdtype(k.dtype, np.floating)):
        raise ValueError('the kernel must be an integer or float array (got %s)' % k.dtype)
    ys, xs = np.nonzero(k)
    if ys.size < 1:
        raise ValueError('the kernel has no tap')
    if ys.size > MAX_TAPS:
        raise ValueError('the kernel has %d taps; a line in a %d box has at most %d' % (ys.size, MAX_KSIZE, MAX_TAPS))
    v = k[ys, xs]
    if not (v == v[0]).all() or not v[0] > 0:
        raise ValueError('the non-zero entries of the kernel must all be equal and positive: n taps of weight 1 / n')
    t = np.zeros((TABLE,), np.int32)
    t[0], t[1] = ys.size, ksize
    t[2:2 + 2 * ys.size:2] = ys - ksize // 2
    t[3:3 + 2 * ys.size:2] = xs - ksize // 2
    return t


def _check_table(t):
    """A host table as `taps_of` makes it."""
    t = np.asarray(t)
    if t.dtype != np.int32 or t.shape != (TABLE,):
        raise ValueError('taps must be an int32 table of %d entries (got %s %s)' % (TABLE, t.dtype, t.shape))
    n, ksize = int(t[0]), int(t[1])
    if not 1 <= n <= MAX_TAPS or ksize % 2 == 0 or not 3 <= ksize <= MAX_KSIZE:
        raise ValueError('taps: n must be in 1..%d and ksize odd in 3..%d (got n = %d, ksize = %d)' % (MAX_TAPS, MAX_KSIZE, n, ksize))
    if np.abs(t[2:2 + 2 * n]).max() > ksize // 2:
        raise ValueError('taps: an offset lies outside the %d x %d kernel' % (ksize, ksize))
    return t


class MotionDraws:
    """The MotionBlur draw of one item: `taps`, the int32 [TABLE] table of `taps_of`, or None when the blur did not fire. Made from a `kernel`
    image or from a table: a NumPy table is checked; a device tensor is taken as it is (int32, TABLE entries). `.to(device)` gives the same
    record with a device tensor; `apply` with that uploads nothing and does not synchronise: capture it in a graph and write a new table into
    `taps` between replays (the kernel clamps n to 1..49 and the offsets to +-24)."""

    def __init__(self, kernel=None, taps=None):
        if kernel is not None and taps is not None:
            raise ValueError('give the kernel or the table, not both')
        if kernel is not None:
            taps = taps_of(kernel)
        elif torch.is_tensor(taps):
            if taps.dtype != torch.int32 or taps.numel() != TABLE:
                raise ValueError('taps must be an int32 table of %d entries (got %s %s)' % (TABLE, taps.dtype, tuple(taps.shape)))
        elif taps is not None:
            taps = _check_table(taps)
        self.taps = taps

    @property
    def fired(self):
        """Whether the blur runs."""
        return self.taps is not None

    @property
    def on_device(self):
        return self.taps is None or torch.is_tensor(self.taps)

    def to(self, device=None):
        device = resolve_device(device)
        return MotionDraws(taps=upload(self.taps, device))


def draw(random, p=0.3, kernel_fn=None):
    """The calls `MotionBlur.__call__` (transforms.py:971-1019) makes on the loader's `np.random.RandomState` for an item without `bg`, in its
    order: `rand()`, not fired when `> p`; `uniform(0, 1)` of the bg branch (consumed; the branch needs a bg); `uniform(0, 1) < 0.9` decides
    whether the clip is blurred, and only then `kernel_fn()` is called for the kernel image (albumentations' own generator, which is not this
    `random`: `lambda: draw_kernel(py_random)` without OpenCV); the last `uniform(0, 1)` of the bg blur (consumed). Returns a MotionDraws."""
    if random.rand() > p:
        return MotionDraws()
    random.uniform(0, 1)
    kernel = None
    if random.uniform(0, 1) < 0.9:
        if kernel_fn is None:
            raise ValueError('the blur fired: kernel_fn must return the kernel image')
        kernel = kernel_fn()
    random.uniform(0, 1)
    return MotionDraws(kernel)


def line_kernel(ksize, p0, p1):
    """A (ksize, ksize) uint8 image with an 8-connected line of ones from p0 = (x0, y0) to p1 = (x1, y1): max(|dx|, |dy|) + 1 pixels, one per
    step of the longer axis, the shorter coordinate rounded to the nearest integer (halves up). A stand-in for `cv2.line(kernel, p0, p1, 1,
    thickness=1)`: equality with cv2.line pixel for pixel is NOT claimed and was not checked."""
    ksize = integer(ksize, 'ksize')
    if ksize % 2 == 0 or not 3 <= ksize <= MAX_KSIZE:
        raise ValueError('ksize must be odd and in 3..%d (got %d)' % (MAX_KSIZE, ksize))
    (x0, y0), (x1, y1) = ((integer(v, 'a coordinate') for v in pt) for pt in (p0, p1))
    if min(x0, y0, x1, y1) < 0 or max(x0, y0, x1, y1) >= ksize:
        raise ValueError('the end points must lie inside the %d x %d kernel (got %r, %r)' % (ksize, ksize, p0, p1))
    dx, dy = x1 - x0, y1 - y0
    steps = max(abs(dx), abs(dy))
    kernel = np.zeros((ksize, ksize), np.uint8)
    for i in range(steps + 1):
        x = x0 + ((2 * i * dx + steps) // (2 * steps) if steps else 0)
        y = y0 + ((2 * i * dy + steps) // (2 * steps) if steps else 0)
        kernel[y, x] = 1
    return kernel


def draw_kernel(py_random, blur_limit=(3, 49)):
    """albumentations' published draw of MotionBlur's kernel (`get_params`) on a Python `random.Random`: an odd ksize chosen from blur_limit,
    two end points with `randint(0, ksize - 1)`, the y pair redrawn with `sample(range(ksize), 2)` when the x are equal, and the line between
    them from `line_kernel` where albumentations calls cv2.line. Returns the uint8 0 / 1 image. Equality with albumentations' generator (its
    version, its calls, cv2.line) is NOT claimed and was not checked: neither is installed where this was written."""
    lo, hi = (integer(v, 'blur_limit') for v in blur_limit)
    ksize = py_random.choice(list(range(lo, hi + 1, 2)))
    xs, xe = py_random.randint(0, ksize - 1), py_random.randint(0, ksize - 1)
    if xs == xe:
        ys, ye = py_random.sample(range(ksize), 2)
    else:
        ys, ye = py_random.randint(0, ksize - 1), py_random.randint(0, ksize - 1)
    return line_kernel(ksize, (xs, ys), (xe, ye))


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------
def _draws(draws, need_fired):
    if not isinstance(draws, MotionDraws):
        raise TypeError('draws must be a MotionDraws (got %s)' % type(draws).__name__)
    if need_fired and not draws.fired:
        raise ValueError('the draws did not fire: there is nothing to blur with')
    return draws


def _sized(x_u8, channels, what):
    x, lead, n, h, w = images(x_u8, channels, what)
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError('%s must be at most %d pixels a side (got %d x %d)' % (what, MAX_SIDE, h, w))
    return x, lead, n, h, w


def _run_frames(f, n, h, w, table, epilogue, mean, std):
    out = torch.empty((n, 3, h, w) if epilogue == NORM else (n, h, w, 3), dtype=torch.float32 if epilogue == NORM else torch.uint8, device=f.device)
    if n > 0:
        hip.call('mg_motion_frames', hip.ptr(f), hip.ptr(out), hip.ptr(table), c_long(n), c_int(h), c_int(w), c_int(epilogue), float3(mean),
                 float3(std), hip.stream())
    return out


def _run_planes(x, n, h, w, table):
    out = torch.empty((n, h, w), dtype=torch.uint8, device=x.device)
    if n > 0:
        hip.call('mg_motion_planes', hip.ptr(x), hip.ptr(out), hip.ptr(table), c_long(n), c_int(h), c_int(w), hip.stream())
    return out


def blur_frames(frames_u8, draws, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """The blur of fired `draws` on (..., h, w, 3) uint8 frames. Returns uint8 (..., h, w, 3) on the device, or with `normalize` fp32
    (..., 3, h, w): ToTensor + Normalize of the uint8 result, the bits of `normalize_frames` on it, with no uint8 intermediate. One launch."""
    _draws(draws, True)
    f, lead, n, h, w = _sized(frames_u8, 3, 'frames')
    f = to_device(f, device)
    table = int_table(draws.taps, f.device, TABLE, 'MotionDraws.taps')
    out = _run_frames(f, n, h, w, table, NORM if normalize else RAW, mean, std)
    return out.reshape(lead + ((3, h, w) if normalize else (h, w, 3)))


def blur_planes(planes_u8, draws, device=None):
    """The blur of fired `draws` on (..., h, w) uint8 planes. Returns uint8 in the same shape on the device. One launch."""
    _draws(draws, True)
    x, lead, n, h, w = _sized(planes_u8, 1, 'planes')
    x = to_device(x, device)
    return _run_planes(x, n, h, w, int_table(draws.taps, x.device, TABLE, 'MotionDraws.taps')).reshape(lead + (h, w))


def apply(frames_u8, alphas_u8, draws, *, normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """MotionBlur of `draws` (a MotionDraws) on the stacked uint8 arrays of one item: frames (..., h, w, 3) and alphas (..., h, w) or None, all
    with the one kernel, as the reference filters them as channels of one image. Returns (frames, alphas) on the device: uint8 in the input
    layout, the frames with `normalize` as fp32 (..., 3, h, w). One launch for the frames and one for the alphas. Draws that did not fire
    give the inputs themselves (on the device), or the bits of `normalize_frames` of the frames."""
    _draws(draws, False)
    f, lead, n, h, w = _sized(frames_u8, 3, 'frames')
    a = None
    if alphas_u8 is not None:
        a, alead, an, ah, aw = _sized(alphas_u8, 1, 'alphas')
        if (ah, aw) != (h, w):
            raise ValueError('alphas: expected %d x %d like the frames (got %d x %d)' % (h, w, ah, aw))
    if not draws.fired:
        if normalize:
            f = photometric.apply(f, photometric.PhotoDraws(), normalize=True, mean=mean, std=std, device=device)
        else:
            f = to_device(f, device)
        return f, (None if a is None else to_device(a, f.device))
    f = to_device(f, device)
    dev = f.device
    table = int_table(draws.taps, dev, TABLE, 'MotionDraws.taps')
    out_f = _run_frames(f, n, h, w, table, NORM if normalize else RAW, mean, std).reshape(lead + ((3, h, w) if normalize else (h, w, 3)))
    out_a = None
    if a is not None:
        out_a = _run_planes(to_device(a, dev), an, h, w, table).reshape(alead + (h, w))
    return out_f, out_a
