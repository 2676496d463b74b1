"""Background compositing on the device (HIP kernels of csrc/background.hip) -- the chain of the reference's transforms for data sets that ship
only foregrounds and alphas (maggie/dataloader/transforms.py:307-370,841-864):

  LoadRandomBackground -> HistogramMatching -> ComposeBackground

  * `draw_path`, `draw_window`, `draw_histmatch`   the reference's calls on the loader's `np.random.RandomState`, in its order (pure host code);
  * `BackgroundDraws`, `HistDraws`                 one item's draws; `.to(device)` makes a later call upload nothing;
  * `gaussian_taps`                                the integer taps of the blur;
  * `blur_crop`                                    the window of the blurred background, one launch (`mg_bg_blur_crop`);
  * `histograms`                                   per-channel counts of a clip, one launch (`mg_bg_hist`);
  * `match_luts`                                   the two tone curves of the histogram matching (`mg_bg_match_lut`, one workgroup);
  * `compose`                                      the alpha composite through the curves, one launch (`mg_bg_compose`);
  * `random_background`                            the driver: at most five launches of this library (window, two histograms, curves,
                                                   composite) and one fill of the 6 KB of counts; nothing is read back.

The blur is integer arithmetic modelled on OpenCV's 8-bit fixed-point path: taps q_i = rint(256 k_i) of cv2.getGaussianKernel's formula, the
centre absorbing 256 - sum(q); horizontal 16-bit sums, vertical 32-bit sums, (s + 32768) >> 16; BORDER_REFLECT_101 on the whole background.
It was NOT compared with cv2.GaussianBlur (OpenCV is not a dependency and not installed where this was written): a tap or an output may
differ from it by one unit. The histogram matching restates the float branch of skimage.exposure.match_histograms (the version with
`channel_axis`): np.unique -> cumsum / size -> np.interp. On uint8 frames that is a 256-entry table per channel, which the device builds from
the histograms. It was NOT compared with skimage, which is not installed either. The `cv2.resize` behind the reference's crop is always an
identity (the window has the frame's size) and is not built.

Wrong dtype (TypeError), shape, kernel size or window (ValueError) raise before anything touches the device. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import check_u8, images, integer, resolve_device, to_device, upload

MAX_KSIZE, WIN_TABLE = 25, 32              # MG_BG_MAX_KSIZE / MG_BG_WIN_TABLE (include/maggie_hip.h)
TILE_ROWS, TILE_COLS, MAX_SIDE = 16, 64, 32767                              # MG_BG_TILE_ROWS / _TILE_COLS / _MAX_SIDE
BLUR_KERNEL_SIZES, BLUR_SIGMAS = (5, 15, 25), (1.0, 1.5, 3.0, 5.0)          # LoadRandomBackground's defaults

_WEIGHTS, _IDENTITY = {}, {}               # per device: the (256, 2) fp64 table of the composite, the (2, 3, 256) identity curves


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------
def gaussian_taps(ksize, sigma):
    """The int32 [ksize] taps of the blur: k_i = exp(-(i - (ksize - 1) / 2)^2 / (2 sigma^2)) normalised in fp64, q_i = rint(256 k_i) (halves
    to even), the centre tap absorbing 256 - sum(q). ksize odd in 1..25, sigma > 0; ValueError otherwise."""
    ksize = integer(ksize, 'ksize')
    if ksize % 2 == 0 or not 1 <= ksize <= MAX_KSIZE:
        raise ValueError('ksize must be odd and in 1..%d (got %d)' % (MAX_KSIZE, ksize))
    sigma = float(sigma)
    if not (sigma > 0 and np.isfinite(sigma)):
        raise ValueError('sigma must be positive (got %r)' % sigma)
    i = np.arange(ksize, dtype=np.float64) - (ksize - 1) / 2
    k = np.exp(-(i * i) / (2 * sigma * sigma))
    k = k / k.sum()
    q = np.rint(256 * k).astype(np.int64)
    q[ksize // 2] += 256 - int(q.sum())
    if q.min() < 0 or q[ksize // 2] < 1:
        raise ValueError('the taps of ksize %d, sigma %r do not quantise to 8 bits with a positive centre' % (ksize, sigma))
    return q.astype(np.int32)


def _win_table(taps, x, y):
    t = np.zeros((WIN_TABLE,), np.int32)
    if taps is None:
        t[0], t[4] = 1, 256                                                 # the plain copy: one tap of weight 1
    else:
        t[0] = len(taps)
        t[4:4 + len(taps)] = taps
    t[1], t[2] = x, y
    return t


class BackgroundDraws:
    """The LoadRandomBackground draw of one item: `taps` (the int32 taps of `gaussian_taps`, or None when the blur did not fire), the window's
    corner `x`, `y` in the background and its size `h`, `w` (the frames'). `win` is the int32 [WIN_TABLE] table the device reads: ksize, x, y, 0,
    the taps. `.to(device)` gives the same record with `win` on the device; `blur_crop` with that uploads nothing and does not synchronise, and
    a new table may be written into `win` between replays of a captured graph (the kernel clamps ksize, x, y and the taps to their ranges)."""

    def __init__(self, taps, x, y, h, w, win=None):
        if taps is not None:
            taps = np.asarray(taps)
            if taps.ndim != 1 or not np.issubdtype(taps.dtype, np.integer) or taps.size % 2 == 0 or taps.size > MAX_KSIZE:
                raise ValueError('taps must be an odd number (1..%d) of ints (got %s %s)' % (MAX_KSIZE, taps.dtype, taps.shape))
            if taps.min() < 0 or int(taps.sum()) != 256:
                raise ValueError('taps must be >= 0 and sum to 256 (got a sum of %d)' % int(taps.sum()))
            taps = taps.astype(np.int32)
        self.taps = taps
        self.x, self.y, self.h, self.w = (integer(v, n) for v, n in ((x, 'x'), (y, 'y'), (h, 'h'), (w, 'w')))
        if self.x < 0 or self.y < 0 or self.h < 1 or self.w < 1:
            raise ValueError('the window must have x, y >= 0 and h, w >= 1 (got x %d, y %d, h %d, w %d)' % (self.x, self.y, self.h, self.w))
        self.win = _win_table(taps, self.x, self.y) if win is None else win

    @property
    def blurred(self):
        return self.taps is not None

    @property
    def on_device(self):
        return torch.is_tensor(self.win)

    def to(self, device=None):
        device = resolve_device(device)
        return BackgroundDraws(self.taps, self.x, self.y, self.h, self.w, upload(self.win, device))


class HistDraws:
    """The HistogramMatching draw of one item that fired: `ratio` of the blend and `match_bg` (the background is matched to the foreground
    instead of the foreground to the background). `table` is the fp32 [4] the device reads: f32(ratio), f32(1. - ratio), match_bg, 0 -- the two
    scalars as NumPy makes them from a Python float next to a float32 array. `.to(device)` as for BackgroundDraws."""

    def __init__(self, ratio, match_bg=False, table=None):
        self.ratio = float(ratio)
        if not 0.0 <= self.ratio <= 1.0:
            raise ValueError('ratio must lie in [0, 1] (got %r)' % (ratio,))
        self.match_bg = bool(match_bg)
        self.table = np.array([self.ratio, 1. - self.ratio, float(self.match_bg), 0.0], np.float32) if table is None else table

    @property
    def on_device(self):
        return torch.is_tensor(self.table)

    def to(self, device=None):
        device = resolve_device(device)
        return HistDraws(self.ratio, self.match_bg, upload(self.table, device))


def draw_path(random, bg_paths):
    """`random.choice(bg_paths)`: the first call of LoadRandomBackground on the loader's RandomState."""
    return random.choice(bg_paths)


def draw_window(random, bg_hw, frame_hw, blur_p=0.5, blur_kernel_size=BLUR_KERNEL_SIZES, blur_sigma=BLUR_SIGMAS):
    """The calls LoadRandomBackground makes once the file's size is known, in its order: `rand()`; when it is below `blur_p`,
    `choice(kernel sizes)` and `choice(sigmas)`; `randint(0, bw - w)` and `randint(0, bh - h)`. The background must be strictly larger than the
    frames on both sides: for equal sizes `randint(0, 0)` raises ValueError, as it does in the reference. Returns a BackgroundDraws."""
    bh, bw = (integer(v, 'bg_hw') for v in bg_hw)
    h, w = (integer(v, 'frame_hw') for v in frame_hw)
    taps = None
    if random.rand() < blur_p:
        ksize = random.choice(blur_kernel_size)
        sigma = random.choice(blur_sigma)
        taps = gaussian_taps(int(ksize), float(sigma))
    x = random.randint(0, bw - w)
    y = random.randint(0, bh - h)
    return BackgroundDraws(taps, int(x), int(y), h, w)


def draw_histmatch(random, p=0.3):
    """The calls of HistogramMatching: `rand()`, None when it is above `p`; else `uniform(0, 0.5)` and `rand() < 0.05`. Returns a HistDraws."""
    if random.rand() > p:
        return None
    ratio = random.uniform(0, 0.5)
    match_bg = random.rand() < 0.05
    return HistDraws(ratio, match_bg)


# ---- argument checks (all before any launch) --------------------------------------------------------------------------------------------------
def _bg_draws(draws):
    if not isinstance(draws, BackgroundDraws):
        raise TypeError('draws must be a BackgroundDraws (got %s)' % type(draws).__name__)
    win = draws.win
    if torch.is_tensor(win):
        if win.dtype != torch.int32 or win.numel() != WIN_TABLE:
            raise ValueError('BackgroundDraws.win must be int32 with %d entries (got %s %s)' % (WIN_TABLE, win.dtype, tuple(win.shape)))
    elif not isinstance(win, np.ndarray) or win.dtype != np.int32 or win.shape != (WIN_TABLE,):
        raise ValueError('BackgroundDraws.win must be an int32 table of %d entries' % WIN_TABLE)
    return draws


def _hist_draws(draws):
    if draws is None:
        return None
    if not isinstance(draws, HistDraws):
        raise TypeError('hist_draws must be a HistDraws or None (got %s)' % type(draws).__name__)
    t = draws.table
    if torch.is_tensor(t):
        if t.dtype != torch.float32 or t.numel() != 4:
            raise ValueError('HistDraws.table must be float32 with 4 entries (got %s %s)' % (t.dtype, tuple(t.shape)))
    elif not isinstance(t, np.ndarray) or t.dtype != np.float32 or t.shape != (4,):
        raise ValueError('HistDraws.table must be a float32 table of 4 entries')
    return draws


def _background(bg_u8, draws):
    """The checked background of a window: the tensor, bh, bw."""
    bg = check_u8(bg_u8, 'background')
    if bg.dim() != 3 or bg.shape[-1] != 3 or bg.shape[0] < 1 or bg.shape[1] < 1:
        raise ValueError('background: expected (H, W, 3) (got shape %s)' % (tuple(bg.shape),))
    bh, bw = int(bg.shape[0]), int(bg.shape[1])
    if bh > MAX_SIDE or bw > MAX_SIDE:
        raise ValueError('background must be at most %d pixels a side (got %d x %d)' % (MAX_SIDE, bh, bw))
    if draws.x + draws.w > bw or draws.y + draws.h > bh:
        raise ValueError('the window %d x %d at (%d, %d) leaves the %d x %d background' % (draws.h, draws.w, draws.y, draws.x, bh, bw))
    return bg, bh, bw


def _clip(frames_u8, what='frames'):
    f, lead, n, h, w = images(frames_u8, 3, what)
    if n * h * w >= 2 ** 31:
        raise ValueError('%s: the clip must have fewer than 2^31 pixels (got %d)' % (what, n * h * w))
    return f, lead, n, h, w


def _luts(luts):
    if luts is None:
        return None
    a = luts if torch.is_tensor(luts) else np.asarray(luts)
    if a.dtype != (torch.uint8 if torch.is_tensor(a) else np.uint8):
        raise TypeError('luts must be uint8 (got %s)' % a.dtype)
    if tuple(a.shape) != (2, 3, 256):
        raise ValueError('luts must have shape (2, 3, 256) (got %s)' % (tuple(a.shape),))
    return a


def _fg_alphas(fg_u8, alphas_u8):
    f, lead, n, h, w = _clip(fg_u8, 'fg')
    a, alead, an, ah, aw = images(alphas_u8, 1, 'alphas')
    if (alead, ah, aw) != (lead, h, w):
        raise ValueError('alphas: expected shape %s like fg (got %s)' % (lead + (h, w), tuple(a.shape)))
    if n > 65535:
        raise ValueError('fg: at most 65535 frames (got %d)' % n)
    return f, a, lead, n, h, w


def _compose_args(fg_u8, alphas_u8, bg_u8):
    f, a, lead, n, h, w = _fg_alphas(fg_u8, alphas_u8)
    b = check_u8(bg_u8, 'background')
    if tuple(b.shape) == (h, w, 3):
        bn = 1
    elif tuple(b.shape) == lead + (h, w, 3):
        bn = n
    else:
        raise ValueError('bg: expected shape %s or %s (got %s)' % ((h, w, 3), lead + (h, w, 3), tuple(b.shape)))
    return f, a, b, lead, n, bn, h, w


def _weights(device):
    """The (256, 2) fp64 table a / 255.0, 1 - a / 255.0 of the composite, made on the host once per device."""
    t = _WEIGHTS.get(device)
    if t is None:
        a = np.arange(256).astype(float) / 255.0
        t = _WEIGHTS[device] = torch.from_numpy(np.ascontiguousarray(np.stack([a, 1 - a], axis=1))).to(device)
    return t


def identity_luts(device=None):
    """The cached (2, 3, 256) identity curves of a device (shared: do not write into them)."""
    device = resolve_device(device)
    t = _IDENTITY.get(device)
    if t is None:
        t = _IDENTITY[device] = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8), (2, 3, 256)))).to(device)
    return t


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------
def _run_window(bg, bh, bw, draws):
    out = torch.empty((draws.h, draws.w, 3), dtype=torch.uint8, device=bg.device)
    win = upload(draws.win, bg.device).contiguous()
    hip.need_cuda(win)
    hip.call('mg_bg_blur_crop', hip.ptr(bg), c_int(bh), c_int(bw), hip.ptr(win), hip.ptr(out), c_int(draws.h), c_int(draws.w), hip.stream())
    return out


def _run_hist(x, pixels, counts):
    hip.call('mg_bg_hist', hip.ptr(x), c_long(pixels), hip.ptr(counts), hip.stream())


def _run_luts(counts, hist_draws):
    luts = torch.empty((2, 3, 256), dtype=torch.uint8, device=counts.device)
    table = upload(hist_draws.table, counts.device).contiguous()
    hip.need_cuda(table)
    hip.call('mg_bg_match_lut', hip.ptr(counts[0]), hip.ptr(counts[1]), hip.ptr(table), hip.ptr(luts), hip.stream())
    return luts


def _run_compose(f, a, b, lead, n, bn, h, w, luts, return_fg_bg):
    dev = f.device
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    fo = torch.empty_like(out) if return_fg_bg else None
    bo = torch.empty(b.shape, dtype=torch.uint8, device=dev) if return_fg_bg else None
    if n > 0:
        hip.call('mg_bg_compose', hip.ptr(f), hip.ptr(a), hip.ptr(b), c_long(bn), c_long(n), c_int(h), c_int(w), hip.ptr(luts),
                 hip.ptr(_weights(dev)), hip.ptr(out), hip.ptr(fo), hip.ptr(bo), hip.stream())
    out = out.reshape(lead + (h, w, 3))
    return (out, fo.reshape(lead + (h, w, 3)), bo) if return_fg_bg else out


def blur_crop(bg_u8, draws, device=None):
    """The window `draws` (a BackgroundDraws) cuts from the blurred (H, W, 3) uint8 background: uint8 (h, w, 3) on the device. Only the
    window's pixels are computed; without taps the launch is a plain copy of the window. One launch."""
    draws = _bg_draws(draws)
    bg, bh, bw = _background(bg_u8, draws)
    return _run_window(to_device(bg, device), bh, bw, draws)


def histograms(frames_u8, device=None):
    """The per-channel counts of (..., H, W, 3) uint8 frames over the whole clip: (3, 256) on the device, int32 (the bits of the library's
    uint32: a clip has fewer than 2^31 pixels, ValueError otherwise). One launch behind the fill of the counts."""
    f, lead, n, h, w = _clip(frames_u8)
    f = to_device(f, device)
    counts = torch.zeros((3, 256), dtype=torch.int32, device=f.device)
    if n > 0:
        _run_hist(f, n * h * w, counts)
    return counts


def match_luts(fg_u8, bg_u8, hist_draws, device=None):
    """The tone curves of HistogramMatching for the clip `fg_u8` (..., H, W, 3) and the background `bg_u8` (its window (H, W, 3), or the tiled
    (..., H, W, 3): the quantiles are the same): uint8 (2, 3, 256) on the device, [0] for the foreground, [1] for the background. The side
    that is not matched, and byte values that do not occur, are the identity. `hist_draws` None gives the shared identity curves without a
    launch. Two histogram launches and one workgroup for the curves; nothing is read back."""
    hist_draws = _hist_draws(hist_draws)
    f, _, n, h, w = _clip(fg_u8, 'fg')
    b, _, bn, bh, bw = _clip(bg_u8, 'bg')
    if hist_draws is None:
        return identity_luts(resolve_device(device, f if f.is_cuda else b))
    if n == 0 or bn == 0:
        raise ValueError('match_luts needs at least one frame on either side')
    f = to_device(f, device)
    b = to_device(b, f.device)
    counts = torch.zeros((2, 3, 256), dtype=torch.int32, device=f.device)
    _run_hist(f, n * h * w, counts[0])
    _run_hist(b, bn * bh * bw, counts[1])
    return _run_luts(counts, hist_draws)


def compose(fg_u8, alphas_u8, bg_u8, luts=None, return_fg_bg=False, device=None):
    """ComposeBackground: uint8(clip(fg * (a / 255.0) + bg * (1 - a / 255.0), 0, 255)) in fp64, with `fg` and `bg` first sent through the
    curves `luts` (uint8 (2, 3, 256) of `match_luts`, or None). fg (..., H, W, 3), alphas (..., H, W), bg (H, W, 3) shared by all frames or
    (..., H, W, 3). Returns the frames on the device in fg's shape; with `return_fg_bg` also the curve-applied fg and bg (bg in its own
    shape), which the reference keeps in the item. One launch."""
    f, a, b, lead, n, bn, h, w = _compose_args(fg_u8, alphas_u8, bg_u8)
    luts = _luts(luts)
    f = to_device(f, device)
    dev = f.device
    a, b = to_device(a, dev), to_device(b, dev)
    if luts is not None:
        luts = upload(luts, dev).contiguous()
    return _run_compose(f, a, b, lead, n, bn, h, w, luts, return_fg_bg)


def random_background(fg_u8, alphas_u8, bg_u8, bg_draws, hist_draws, return_fg_bg=False, device=None):
    """LoadRandomBackground -> HistogramMatching -> ComposeBackground of one item: `fg_u8` (..., H, W, 3) and `alphas_u8` (..., H, W) over the
    window `bg_draws` cuts from the decoded (BH, BW, 3) background `bg_u8`, matched with `hist_draws` (None: not fired). Returns the composed
    frames on the device, with `return_fg_bg` also the matched fg and the matched (H, W, 3) window. At most five launches of the library and
    one fill; with draws on the device nothing is uploaded, so the call can be captured in a graph."""
    bg_draws, hist_draws = _bg_draws(bg_draws), _hist_draws(hist_draws)
    bg, bh, bw = _background(bg_u8, bg_draws)
    f, a, lead, n, h, w = _fg_alphas(fg_u8, alphas_u8)
    if (h, w) != (bg_draws.h, bg_draws.w):
        raise ValueError('the window is %d x %d but the frames are %d x %d' % (bg_draws.h, bg_draws.w, h, w))
    f = to_device(f, device)
    dev = f.device
    a = to_device(a, dev)
    window = _run_window(to_device(bg, dev), bh, bw, bg_draws)
    luts = None
    if hist_draws is not None and n > 0:
        counts = torch.zeros((2, 3, 256), dtype=torch.int32, device=dev)
        _run_hist(f, n * h * w, counts[0])
        _run_hist(window, h * w, counts[1])
        luts = _run_luts(counts, hist_draws)
    return _run_compose(f, a, window, lead, n, 1, h, w, luts, return_fg_bg)
