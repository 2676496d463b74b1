"""The training crop of the loaders on the device (HIP kernels of csrc/crop.hip) -- the two steps the reference runs between
PaddingMultiplyBy and the mask chain of a training item (maggie/dataloader/transforms.py:191-305, wired in him.py:44-45 and vim.py:49-50):

  ... -> Stack -> RandomCropByAlpha(crop, random, padding_prob) -> RandomHorizontalFlip(random, flip_p) -> ...

  * `draw`            the reference's calls on the loader's `np.random.RandomState`, in its order, quirks included (pure host code);
  * `draw_on_device`  `draw` with the two data-dependent questions -- the box of `alphas.mean(0) > 127`, and which candidate window holds a
                      value `> 127` -- answered by mg_crop_bbox / mg_crop_hits;
  * `apply`           the pixels: the window and the flip as one gather (crop branch), or the zero border and cv2.resize as one table-driven
                      launch per array (padding branch), raw uint8 or, for the frames, straight to the normalised fp32 tensor.

Everything on the device is integer work or the IEEE divisions of Normalize: the results are bit-exact, no tolerance anywhere. The interpolation
tables of the padding branch are `geometry.resize_tables` on the padded size (`maskgen.resize_axis`, `geometry.nearest_axis`), not a copy. A
`CropDraws` moved to the device (`.to(device)`) makes `apply` upload nothing and never synchronise, so it can be captured in a graph and a new
window written into `draws.window` between replays.

What stays with the caller: the draws of GammaContrast, AdditiveGaussionNoise and JpegCompression (imgaug's own generators; no equality with
them is claimed), which follow the flip in the reference's stream and precede the mask chain's, and the kernel of MotionBlur for video. The
steps themselves have device forms: `lut` here is a per-channel tone curve the caller drew, utils/motion.py has MotionBlur, utils/photometric.py
the noise and the JPEG round trip, utils/affine.py RandomAffine with its draws. Also the caller's: the `> 127` area filter and the random instance removal of
him.py:119-149.

Wrong dtype, rank or size raise before a launch; a crop larger than the image raises the reference's ValueError. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import geometry
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, images, int_table, integer, lut_table, resolve_device, to_device, upload
from .geometry import LINEAR, NEAREST

RAW, NORM = 0, 1                           # MG_CROP_RAW / MG_CROP_NORM (include/maggie_hip.h)
MAX_WINDOWS = 3                            # MG_CROP_MAX_WINDOWS: the reference tries three windows
MAX_PLANES = 1 << 22                       # MG_CROP_MAX_PLANES
CHUNK = 16                                 # MG_CROP_CHUNK
# The crop branch's frames with normalize=True: True = the gather's own Normalize epilogue (one launch, no uint8 intermediate), False = the raw
# gather followed by `normalize_frames`. Both give the same bits (tests/test_gpu_crop.py); DESIGN.md section 17 records which is measured faster.
FUSED_NORMALIZE = True


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------------
def _size(crop_size):
    try:
        ch, cw = crop_size
    except (TypeError, ValueError):
        raise TypeError('crop_size must be (height, width) (got %r)' % (crop_size,))
    return integer(ch, 'crop_size'), integer(cw, 'crop_size')


def pad_amounts(H, W):
    """(pad_h, pad_w) of the padding branch (transforms.py:247-252): the short side is padded, on both sides, to the long one (less one when
    the difference is odd)."""
    return (0, (H - W) // 2) if H > W else ((W - H) // 2, 0)


def pad_tables(H, W, crop_size, flip):
    """The padding branch as tables: (pad_h, pad_w, out_h, out_w, linear, nearest). The reference hands `crop_size` = (ch, cw) to cv2.resize as
    `dsize`, which is (width, height): the result is ch wide and cw high. `linear` ([out_w][3] | [out_h][3]) and `nearest` ([out_w] | [out_h])
    are `geometry.resize_tables` of the padded size, the column part reversed when `flip` is set."""
    ch, cw = _size(crop_size)
    pad_h, pad_w = pad_amounts(H, W)
    out_h, out_w = cw, ch
    t = geometry.resize_tables(H + 2 * pad_h, W + 2 * pad_w, out_h, out_w)
    linear, nearest = t['linear'], t['nearest']
    if flip:
        linear = np.concatenate([linear[:3 * out_w].reshape(out_w, 3)[::-1].reshape(-1), linear[3 * out_w:]])
        nearest = np.concatenate([nearest[:out_w][::-1], nearest[out_w:]])
    return pad_h, pad_w, out_h, out_w, np.ascontiguousarray(linear, np.int32), np.ascontiguousarray(nearest, np.int32)


class CropDraws:
    """The draws of one item's RandomCropByAlpha + RandomHorizontalFlip for (H, W) arrays:
      branch  'crop' or 'pad';  flip  whether the columns are reversed;  out_h, out_w  the size of the result
      crop:   window (3,) int32 (x0, y0, flip) -- what mg_crop_gather reads; pairs: how many randint pairs the reference consumed (1..3);
              box: (min_x, max_x, min_y, max_y) as the reference computed them
      pad:    pad (pad_h, pad_w); linear / nearest: the int32 tables of mg_crop_padresize, the flip folded into the columns
    NumPy arrays as drawn; `.to(device)` gives the same record with device tensors. `apply` with that uploads nothing and does not
    synchronise: capture it in a graph and write a new (x0, y0, flip) into `window` between replays (the kernel clamps it to the source)."""

    def __init__(self, branch, H, W, crop_size, flip, out_h, out_w, window=None, pairs=0, box=None, pad=(0, 0), linear=None, nearest=None):
        self.branch, self.H, self.W, self.crop_size, self.flip = branch, int(H), int(W), tuple(crop_size), bool(flip)
        self.out_h, self.out_w, self.window, self.pairs, self.box, self.pad = int(out_h), int(out_w), window, int(pairs), box, tuple(pad)
        self.linear, self.nearest = linear, nearest

    @property
    def on_device(self):
        return torch.is_tensor(self.window if self.branch == 'crop' else self.linear)

    def to(self, device=None):
        device = resolve_device(device)
        return CropDraws(self.branch, self.H, self.W, self.crop_size, self.flip, self.out_h, self.out_w, upload(self.window, device), self.pairs,
                         self.box, self.pad, upload(self.linear, device), upload(self.nearest, device))


def draw(random, H, W, crop_size, padding_prob, flip_p, bbox, hits):
    """RandomCropByAlpha.__call__ + RandomHorizontalFlip.__call__ as draws: the reference's calls on `random` (the loader's
    np.random.RandomState) in the reference's order, leaving it in the reference's state. Pure host code.
      `bbox()`         -> (count, xmin, xmax, ymin, ymax) of `alphas.mean(0) > 127`; asked only on the crop branch (the branch draw does not
                          depend on the box, so it is made first);
      `hits(windows)`  -> the index of the first of the (x0, y0) windows in which any plane holds a value > 127, or None.
    The reference draws a window, looks at it and draws again up to three times, so how many randint pairs it consumes depends on the data. Here
    all three candidates are drawn from a saved state, `hits` answers for them at once, and the consumed pairs are replayed from that state: one
    question instead of up to three, the same generator state afterwards. An empty box is the reference's `except`: (0, W, 0, H) -- W, not
    W - 1."""
    H, W = integer(H, 'H'), integer(W, 'W')
    ch, cw = _size(crop_size)
    if H < ch or W < cw:
        raise ValueError('Crop size {} is larger than image size {}'.format(crop_size, (H, W)))       # transforms.py:231
    if ch < 1 or cw < 1:
        raise ValueError('crop_size must be at least 1 x 1 (got %r)' % (crop_size,))
    if random.rand() > padding_prob:
        count, xmin, xmax, ymin, ymax = (int(v) for v in bbox())
        min_x, max_x, min_y, max_y = (xmin, xmax, ymin, ymax) if count > 0 else (0, W, 0, H)
        hi_x, hi_y = max(max_x - cw, min_x + 1), max(max_y - ch, min_y + 1)
        state = random.get_state()
        windows = []
        for _ in range(MAX_WINDOWS):
            x, y = random.randint(min_x, hi_x), random.randint(min_y, hi_y)
            windows.append((min(int(x), W - cw), min(int(y), H - ch)))
        first = hits(windows)
        pairs = MAX_WINDOWS if first is None else int(first) + 1
        if not 1 <= pairs <= MAX_WINDOWS:
            raise ValueError('hits() must name one of the %d windows or None (got %r)' % (MAX_WINDOWS, first))
        random.set_state(state)
        for _ in range(pairs):
            random.randint(min_x, hi_x), random.randint(min_y, hi_y)
        x0, y0 = windows[pairs - 1]
        flip = bool(random.rand() < flip_p)
        return CropDraws('crop', H, W, (ch, cw), flip, ch, cw, window=np.asarray([x0, y0, int(flip)], np.int32), pairs=pairs,
                         box=(min_x, max_x, min_y, max_y))
    flip = bool(random.rand() < flip_p)
    pad_h, pad_w, out_h, out_w, linear, nearest = pad_tables(H, W, (ch, cw), flip)
    return CropDraws('pad', H, W, (ch, cw), flip, out_h, out_w, pad=(pad_h, pad_w), linear=linear, nearest=nearest)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------
def _planes(x_u8, what):
    return images(x_u8, 1, what)


def bbox(alphas_u8, device=None):
    """(5,) int32 on the device: (count, xmin, xmax, ymin, ymax) of the pixels where the sum over ALL planes of (..., H, W) uint8 alphas exceeds
    127 * planes -- `alphas.mean(0) > 127`; (0, W, -1, H, -1) when there is none."""
    x, _, P, H, W = _planes(alphas_u8, 'alphas')
    if P < 1 or P > MAX_PLANES:
        raise ValueError('expected 1..%d planes (got %d)' % (MAX_PLANES, P))
    x = to_device(x, device)
    out = torch.empty((5,), dtype=torch.int32, device=x.device)
    hip.call('mg_crop_bbox', hip.ptr(x), hip.ptr(out), c_long(P), c_int(H), c_int(W), hip.stream())
    return out


def window_hits(alphas_u8, windows, crop_size, device=None):
    """(n,) int32 on the device: 1 where any plane of the alphas holds a value > 127 inside the (ch, cw) window at (x0, y0) = windows[k]."""
    x, _, P, H, W = _planes(alphas_u8, 'alphas')
    ch, cw = _size(crop_size)
    if P < 1 or P > MAX_PLANES:
        raise ValueError('expected 1..%d planes (got %d)' % (MAX_PLANES, P))
    if not (1 <= ch <= H and 1 <= cw <= W):
        raise ValueError('Crop size {} is larger than image size {}'.format(crop_size, (H, W)))
    if torch.is_tensor(windows):
        n = int(windows.shape[0])
        if windows.dtype != torch.int32 or tuple(windows.shape) != (n, 2):
            raise ValueError('windows must be int32 of shape (n, 2) (got %s %s)' % (windows.dtype, tuple(windows.shape)))
    else:
        windows = np.asarray(windows, np.int32).reshape(-1, 2)
        n = windows.shape[0]
    if n > MAX_WINDOWS:
        raise ValueError('at most %d windows (got %d)' % (MAX_WINDOWS, n))
    x = to_device(x, device)
    wt = windows.contiguous() if torch.is_tensor(windows) else torch.from_numpy(windows).to(x.device, non_blocking=True)
    hip.need_cuda(wt)
    out = torch.zeros((n,), dtype=torch.int32, device=x.device)
    if n > 0:
        hip.call('mg_crop_hits', hip.ptr(x), hip.ptr(wt), hip.ptr(out), c_int(n), c_long(P), c_int(H), c_int(W), c_int(ch), c_int(cw),
                 hip.stream())
    return out


def draw_on_device(random, alphas_u8, crop_size, padding_prob=0.5, flip_p=0.5, device=None):
    """`draw` for (P, H, W) uint8 alphas (host or device), the box and the hit test answered by mg_crop_bbox and mg_crop_hits. Returns a
    host-side `CropDraws`. Read-backs per item, the only host synchronisations of the stage: on the padding branch none (the box is never
    computed); on the crop branch one of 20 bytes (the box) and then one of at most 12 bytes (the three candidates' hit words)."""
    x, _, P, H, W = _planes(alphas_u8, 'alphas')
    if P < 1 or P > MAX_PLANES:
        raise ValueError('expected 1..%d planes (got %d)' % (MAX_PLANES, P))
    held = []

    def on_device():
        if not held:
            held.append(to_device(x, device))
        return held[0]

    def box():
        return bbox(on_device()).cpu().numpy()

    def first_hit(windows):
        h = window_hits(on_device(), windows, crop_size).cpu().numpy()
        return int(np.flatnonzero(h)[0]) if h.any() else None
    return draw(random, H, W, crop_size, padding_prob, flip_p, box, first_hit)


def apply(frames_u8, alphas_u8, masks_u8, draws, *, normalize=False, lut=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """The crop (or pad-and-resize) and the flip of `draws` on the stacked uint8 arrays of one item: frames (T, H, W, 3), alphas (P, H, W),
    masks (P, H, W) or None (any leading dimensions). Returns (frames, alphas, masks) on the device: uint8 in the input layout at
    (draws.out_h, draws.out_w); with `normalize` the frames are (T, 3, out_h, out_w) fp32, ToTensor + Normalize of the uint8 result with no
    uint8 intermediate. `lut`: (3, 256) uint8, applied per channel to the frames after the crop / resize and before Normalize. Frames and
    alphas of the padding branch are INTER_LINEAR, masks INTER_NEAREST; a tap in the border reads 0."""
    if not isinstance(draws, CropDraws):
        raise TypeError('draws must be a CropDraws (got %s)' % type(draws).__name__)
    f, flead, fn, H, W = images(frames_u8, 3, 'frames')
    if (H, W) != (draws.H, draws.W):
        raise ValueError('the draws were made for %d x %d arrays (got frames of %d x %d)' % (draws.H, draws.W, H, W))
    planes = []
    for x, what in ((alphas_u8, 'alphas'), (masks_u8, 'masks')):
        if x is None:
            planes.append(None)
            continue
        x, lead, n, h, w = _planes(x, what)
        if (h, w) != (H, W):
            raise ValueError('%s: expected %d x %d like the frames (got %d x %d)' % (what, H, W, h, w))
        planes.append((x, lead, n))
    lut_table(lut)                                                             # the shape and dtype errors, before the device
    f = to_device(f, device)
    dev = f.device
    lut = lut_table(lut, dev)
    oh, ow = draws.out_h, draws.out_w
    m3, s3 = float3(mean), float3(std)
    if draws.branch == 'crop':
        window = int_table(draws.window, dev, 3, 'CropDraws.window')

        def run(x, n, C, epilogue, table):
            shape = (n, 3, oh, ow) if epilogue == NORM else (n, oh, ow) + ((3,) if C == 3 else ())
            out = torch.empty(shape, dtype=torch.float32 if epilogue == NORM else torch.uint8, device=dev)
            if n > 0:
                hip.call('mg_crop_gather', hip.ptr(x), hip.ptr(out), hip.ptr(window), hip.ptr(table), c_long(n), c_int(C), c_int(H), c_int(W),
                         c_int(oh), c_int(ow), c_int(epilogue), m3, s3, hip.stream())
            return out
    else:
        linear = int_table(draws.linear, dev, 3 * (ow + oh), 'CropDraws.linear')
        nearest = int_table(draws.nearest, dev, ow + oh, 'CropDraws.nearest')
        pad_h, pad_w = draws.pad

        def run(x, n, C, epilogue, table, interp=LINEAR):
            shape = (n, 3, oh, ow) if epilogue == NORM else (n, oh, ow) + ((3,) if C == 3 else ())
            out = torch.empty(shape, dtype=torch.float32 if epilogue == NORM else torch.uint8, device=dev)
            xt, yt = (linear, linear[3 * ow:]) if interp == LINEAR else (nearest, nearest[ow:])
            if n > 0:
                hip.call('mg_crop_padresize', hip.ptr(x), hip.ptr(out), hip.ptr(xt), hip.ptr(yt), hip.ptr(table), c_long(n), c_int(C), c_int(H),
                         c_int(W), c_int(pad_h), c_int(pad_w), c_int(oh), c_int(ow), c_int(interp), c_int(epilogue), m3, s3, hip.stream())
            return out
    if normalize and (FUSED_NORMALIZE or draws.branch != 'crop'):
        out_f = run(f, fn, 3, NORM, lut).reshape(flead + (3, oh, ow))
    else:
        out_f = run(f, fn, 3, RAW, lut).reshape(flead + (oh, ow, 3))
        if normalize:
            from .preprocess import normalize_frames       # lazy: preprocess imports this module for the training item's wiring
            out_f = normalize_frames(out_f, mean, std, dev)
    outs = [out_f]
    for entry, interp in zip(planes, (LINEAR, NEAREST)):
        if entry is None:
            outs.append(None)
            continue
        x, lead, n = entry
        x = to_device(x, dev)
        o = run(x, n, 1, RAW, None) if draws.branch == 'crop' else run(x, n, 1, RAW, None, interp)
        outs.append(o.reshape(lead + (oh, ow)))
    return outs[0], outs[1], outs[2]
