"""Compositing on the device (HIP kernels of csrc/compose.hip): what the reference's two synthesis tools do with Pillow on 80 host workers
(tools/synthesize_image_him.py makes I-HIM50K, tools/synthesize_video_him.py makes V-HIM2K5), so that a training job can draw fresh
composites from the source foregrounds and backgrounds and hand them to `geometry.resize_short_pad -> crop -> ... -> train_item`.

  * `resample_tables`, `pil_resize`   `Image.crop(crop).resize(size, filter)`, bicubic (a = -0.5) or bilinear, exact;
  * `paste`                           `Image.paste`, with or without a mask, in place, clipped as Pillow clips it;
  * `try_place`, `commit`, `planes_u8`  the accept / reject loop's arithmetic: areas before and after an occlusion, the accepted placement,
                                      the planes as the tools save them;
  * `alpha_box`                       x, y, w, h of alpha > 0 (`cv2.boundingRect`);
  * `draw_sources`, `synthesize_image`  the image tool from the decoded arrays on, its draws in its order on a `numpy.random.RandomState`;
  * `plan_video`, `video_frame`       the video tool's geometry (pure host) and one composited frame.

Conventions are Pillow's: a size is (width, height), a box (left, top, right, bottom), a position (x, y). Pixels are uint8 tensors or arrays,
planes (..., H, W) and frames (..., H, W, 3) (`_inputs.py`).

The resampler: per axis and output index i, with scale = in / out, fs = max(scale, 1), support = S fs (S = 2 bicubic, 1
bilinear), center = (i + 0.5) scale, the taps are the source indices max(int(center - support + 0.5), 0) .. min(int(center + support + 0.5), in)
with weights f((x - center + 0.5) * (1 / fs)), divided by their left-to-right sum and rounded to 22 fractional bits (halves away from zero).
A pass is clip8((2^21 + sum in * tap) >> 22); the horizontal pass runs first, a pass whose size does not change is skipped, and the value
between the passes is a byte. One launch does both passes when the source rows a tile of TILE_ROWS output rows reads fit MAX_ROWS rows of LDS;
otherwise two launches go through global memory. Same bytes; `regime=` forces a form.

Argument errors are raised before anything touches the device; without a GPU the error is `hip.MaggieHipError`. `pil_resize`, `paste`, `commit`
and `planes_u8` read nothing back: they can be captured in a graph, and `pil_resize` given device tables (`ResizeTables.to(device)`) follows
tables rewritten between replays (the kernel clamps every entry to the source). There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import photometric
from ._inputs import check_u8, images, integer, resolve_device, to_device, upload

TILE_ROWS, TILE_BYTES, MAX_ROWS = 16, 192, 128                             # MG_COMPOSE_TILE_ROWS / _TILE_BYTES / _MAX_ROWS (include/maggie_hip.h)
LDS_BYTES = MAX_ROWS * TILE_BYTES                                           # MG_COMPOSE_LDS_BYTES
TAB_HEADER, MAX_PLANES, SUM_BLOCKS, MAX_SIDE = 4, 10, 64, 32767             # MG_COMPOSE_TAB_HEADER / _MAX_PLANES / _SUM_BLOCKS / _MAX_SIDE
FUSED, TWO_PASS = 0, 1                                                      # MG_COMPOSE_FUSED / _TWO_PASS
REGIMES = {'fused': FUSED, 'two_pass': TWO_PASS}
PRECISION = 22
SUPPORT = {'bicubic': 2.0, 'bilinear': 1.0}
_DTYPES = {torch.float32: 0, torch.float64: 1}                              # MG_COMPOSE_F32 / _F64


# ---- the resampler's tables (host) ----------------------------------------------------------------------------------------------------------
def _bicubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * -0.5, 0.0))


def _bilinear(x):
    x = np.abs(x)
    return np.where(x < 1.0, 1.0 - x, 0.0)


def _filter(name):
    if name not in SUPPORT:
        raise ValueError("filter must be 'bicubic' or 'bilinear' (got %r)" % (name,))
    return _bicubic if name == 'bicubic' else _bilinear


def resample_tables(in_size, out_size, filter='bicubic'):
    """The int32 (out_size, TAB_HEADER + K) table of one axis: a row is (first source index, tap count, 0, 0, the taps in 2^-22 units, zeros
    up to K); K = the resampler's kernel size ceil(support) * 2 + 1 rounded up to a multiple of 4. All rows at once in float64 arrays, each
    element through the scalar code's operations in the scalar code's order (the sum runs over the tap index, left to right)."""
    f = _filter(filter)
    in_size, out_size = integer(in_size, 'in_size'), integer(out_size, 'out_size')
    if not (1 <= in_size <= MAX_SIDE and 1 <= out_size <= MAX_SIDE):
        raise ValueError('sizes must be in 1..%d (got %d -> %d)' % (MAX_SIDE, in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ss = 1.0 / fs
    K = (int(np.ceil(support)) * 2 + 1 + 3) // 4 * 4
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # astype truncates towards zero, like int()
    n = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    k = np.arange(K, dtype=np.int64)[None, :]
    live = k < n[:, None]
    w = np.where(live, f(((k + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    total = np.zeros(out_size, np.float64)
    for j in range(K):                                                      # left to right; the zeros past a row's count change nothing
        total = total + w[:, j]
    w = np.where((total != 0.0)[:, None], w / np.where(total != 0.0, total, 1.0)[:, None], w)
    taps = np.where(w < 0, -0.5 + w * (1 << PRECISION), 0.5 + w * (1 << PRECISION)).astype(np.int64)
    t = np.zeros((out_size, TAB_HEADER + K), np.int32)
    t[:, 0], t[:, 1] = xmin, n
    t[:, TAB_HEADER:] = np.where(live, taps, 0)
    return t


def rows_read(ytab, out_h):
    """The most source rows a tile of TILE_ROWS output rows reads: what decides between the two forms."""
    if ytab is None:
        return min(TILE_ROWS, out_h)
    first = ytab[0::TILE_ROWS, 0]
    last_i = np.minimum(np.arange(0, out_h, TILE_ROWS) + TILE_ROWS - 1, out_h - 1)
    return int((ytab[last_i, 0] + ytab[last_i, 1] - first).max())


class ResizeTables:
    """The tables of one resize geometry: `x`, `y` (None for a pass that is skipped), `in_size`, `out_size` (both (w, h)), `rows` (`rows_read`)
    and `regime`, the form the host picks. `.to(device)` uploads them once; `pil_resize(..., tables=)` then uploads nothing."""

    def __init__(self, in_size, out_size, filter='bicubic'):
        (iw, ih), (ow, oh) = in_size, out_size
        self.in_size, self.out_size, self.filter = (iw, ih), (ow, oh), filter
        _filter(filter)
        self.x = resample_tables(iw, ow, filter) if iw != ow else None
        self.y = resample_tables(ih, oh, filter) if ih != oh else None
        self.rows = rows_read(self.y, oh)
        self.regime = FUSED if self.rows <= MAX_ROWS else TWO_PASS

    def to(self, device=None):
        device = resolve_device(device)
        t = object.__new__(ResizeTables)
        t.__dict__.update(self.__dict__)
        t.x, t.y = upload(self.x, device), upload(self.y, device)
        return t


def _size(size, what='size'):
    if not isinstance(size, (tuple, list)) or len(size) != 2:
        raise ValueError('%s must be (width, height) (got %r)' % (what, size))
    w, h = integer(size[0], what), integer(size[1], what)
    if not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError('%s: height and width must be in 1..%d (got %r)' % (what, MAX_SIDE, (w, h)))
    return w, h


def _xy(xy):
    if not isinstance(xy, (tuple, list)) or len(xy) != 2:
        raise ValueError('xy must be (x, y) (got %r)' % (xy,))
    x, y = integer(xy[0], 'x'), integer(xy[1], 'y')
    if max(abs(x), abs(y)) > MAX_SIDE:
        raise ValueError('xy must lie within +-%d (got %r)' % (MAX_SIDE, (x, y)))
    return x, y


def _pixels(x_u8, what, channels=None):
    """uint8 (..., H, W) or (..., H, W, 3) -> tensor, leading shape, N, H, W, bytes per pixel. Without `channels` (1 or 3) an array of three or
    more dimensions whose last is 3 means frames."""
    x = check_u8(x_u8, what)
    if channels not in (None, 1, 3):
        raise ValueError('channels must be None, 1 or 3 (got %r)' % (channels,))
    ps = channels or (3 if x.dim() >= 3 and x.shape[-1] == 3 else 1)
    x, lead, n, h, w = images(x, ps, what)
    if h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError('%s must be at most %d pixels a side (got %d x %d)' % (what, MAX_SIDE, h, w))
    return x, lead, n, h, w, ps


def _regime(tables, regime):
    if regime is None:
        return tables.regime
    if regime not in REGIMES:
        raise ValueError("regime must be None, 'fused' or 'two_pass' (got %r)" % (regime,))
    if REGIMES[regime] == FUSED and tables.rows > MAX_ROWS:
        raise ValueError('the fused form holds %d source rows per tile; this geometry reads %d' % (MAX_ROWS, tables.rows))
    return REGIMES[regime]


def _dev_table(t, device):
    if t is None:
        return None
    if torch.is_tensor(t):
        hip.need_cuda(t)
        return t
    return torch.from_numpy(t).to(device, non_blocking=True)


def pil_resize(src_u8, size, filter='bicubic', crop=None, regime=None, device=None, tables=None, out=None, channels=None):
    """`Image.crop(crop).resize(size, filter)` of (..., H, W) planes or (..., H, W, 3) frames (`channels` 1 or 3; None: a last dimension of 3 in three or more means frames). `size`:
    (width, height); `crop`: (left, top, right, bottom) inside the source, read in place by the kernel. `regime`: None (the host picks from
    the tables), 'fused' or 'two_pass' -- the same bytes from both. `tables`: a `ResizeTables` of this geometry (with `.to(device)`: nothing is
    uploaded). `out`: a contiguous uint8 device tensor of the result's shape to write into (any byte alignment). Returns uint8 on the device."""
    x, lead, n, H, W, ps = _pixels(src_u8, 'src', channels)
    ow, oh = _size(size)
    if crop is None:
        crop = (0, 0, W, H)
    if not isinstance(crop, (tuple, list)) or len(crop) != 4:
        raise ValueError('crop must be (left, top, right, bottom) (got %r)' % (crop,))
    l, t, r, b = (integer(v, 'crop') for v in crop)
    if not (0 <= l < r <= W and 0 <= t < b <= H):
        raise ValueError('crop %r must be a non-empty box inside the %d x %d source' % ((l, t, r, b), W, H))
    if tables is None:
        tables = ResizeTables((r - l, b - t), (ow, oh), filter)
    elif not isinstance(tables, ResizeTables) or tables.in_size != (r - l, b - t) or tables.out_size != (ow, oh):
        raise ValueError('tables must be the ResizeTables of %r -> %r' % ((r - l, b - t), (ow, oh)))
    rg = _regime(tables, regime)
    shape = lead + ((oh, ow, 3) if ps == 3 else (oh, ow))
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError('out must be a contiguous uint8 tensor of shape %s' % (shape,))
        hip.need_cuda(out)
    x = to_device(x, device)
    xt, yt = _dev_table(tables.x, x.device), _dev_table(tables.y, x.device)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=x.device)
    tmp = None
    if rg == TWO_PASS and yt is not None:
        tmp = torch.empty((n * (b - t) * ((ow * ps + 15) // 16 * 16),), dtype=torch.uint8, device=x.device)
    if n > 0:
        hip.call('mg_compose_resize', hip.ptr(x), hip.ptr(out), hip.ptr(tmp), hip.ptr(xt), hip.ptr(yt), c_long(n), c_int(ps), c_int(H), c_int(W),
                 c_int(l), c_int(t), c_int(r - l), c_int(b - t), c_int(oh), c_int(ow), c_int(0 if xt is None else xt.shape[1] - TAB_HEADER),
                 c_int(0 if yt is None else yt.shape[1] - TAB_HEADER), c_int(rg), hip.stream())
    return out


# ---- paste ----------------------------------------------------------------------------------------------------------------------------------
def _single(x_u8, what, ps=None):
    x, lead, n, h, w, p = _pixels(x_u8, what, ps)
    if lead not in ((), (1,)) or (ps is not None and p != ps):
        raise ValueError('%s: expected one %s (got shape %s)' % (what, 'plane (H, W)' if ps == 1 else 'image', tuple(x.shape)))
    return x, h, w, p


def paste(dst_u8, src_u8, xy, mask_u8=None):
    """`dst.paste(src, xy, mask)` in place on the DEVICE tensor `dst_u8`: (H, W) or (H, W, 3), `src_u8` of the same kind, `mask_u8` an (h, w)
    plane of the source's size or None (a copy). The box is clipped to the destination. Returns `dst_u8`."""
    if not torch.is_tensor(dst_u8):
        raise TypeError('dst must be a device tensor: the paste is in place (got %s)' % type(dst_u8).__name__)
    d, dh, dw, ps = _single(dst_u8, 'dst')
    s, sh, sw, _ = _single(src_u8, 'src', ps)
    x, y = _xy(xy)
    m = None
    if mask_u8 is not None:
        m, mh, mw, _ = _single(mask_u8, 'mask', 1)
        if (mh, mw) != (sh, sw):
            raise ValueError('mask: expected %d x %d like the source (got %d x %d)' % (sh, sw, mh, mw))
    if not d.is_contiguous():
        raise ValueError('dst must be contiguous: the paste is in place')
    hip.need_cuda(d)
    s = to_device(s, d.device)
    m = None if m is None else to_device(m, d.device)
    hip.call('mg_compose_paste', hip.ptr(d), hip.ptr(s), hip.ptr(m), c_int(ps), c_int(dh), c_int(dw), c_int(sh), c_int(sw), c_int(x), c_int(y),
             hip.stream())
    return dst_u8


# ---- placement --------------------------------------------------------------------------------------------------------------------------------
_UNIT = {}


def unit_table(dtype, device):
    """v / 255 for v in 0..255 as the tools get it (a float64 quotient, rounded when stored as fp32) on `device`; made once per device."""
    key = (dtype, str(device))
    if key not in _UNIT:
        t = np.arange(256, dtype=np.float64) / 255.0
        _UNIT[key] = torch.from_numpy(t.astype(np.float32) if dtype == torch.float32 else t).to(device)
    return _UNIT[key]


def _planes(planes, dtype=None):
    if not torch.is_tensor(planes) or planes.dim() != 3 or planes.dtype not in _DTYPES:
        raise TypeError('planes must be a (P, H, W) fp32 or fp64 device tensor')
    if dtype is not None and planes.dtype != dtype:
        raise TypeError('planes are %s, dtype says %s' % (planes.dtype, dtype))
    P, H, W = (int(v) for v in planes.shape)
    if not (1 <= P <= MAX_PLANES and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError('planes: expected 1..%d planes of 1..%d a side (got %s)' % (MAX_PLANES, MAX_SIDE, tuple(planes.shape)))
    if not planes.is_contiguous():
        raise ValueError('planes must be contiguous')
    return P, H, W


def try_place(planes, a, xy, n_prev, dtype=None):
    """What placing the alpha plane `a` (uint8 (h, w)) at `xy` would do to planes 0..n_prev-1, without writing anything: a float64 array
    (new_areas[n_prev], old_areas[n_prev], area of a / 255). new_area_j = sum plane_j * (1 - a / 255) with 1 - x and the product in the
    planes' dtype (`dtype`, when given, must name it) and the sum in fp64: one partial per workgroup over a strided chunk, then the partials
    in index order -- a fixed order, not NumPy's. One read-back of 8 * (2 * MAX_PLANES + 1) bytes."""
    P, H, W = _planes(planes, dtype)
    n_prev = integer(n_prev, 'n_prev')
    if not 0 <= n_prev <= P:
        raise ValueError('n_prev must be in 0..%d (got %d)' % (P, n_prev))
    a, ha, wa, _ = _single(a, 'a', 1)
    x, y = _xy(xy)
    hip.need_cuda(planes)
    a = to_device(a, planes.device)
    partial = torch.empty((2 * MAX_PLANES + 2, SUM_BLOCKS), dtype=torch.float64, device=planes.device)
    out = torch.empty((2 * MAX_PLANES + 1,), dtype=torch.float64, device=planes.device)
    hip.call('mg_compose_try_place', hip.ptr(planes), hip.ptr(a), hip.ptr(unit_table(planes.dtype, planes.device)), hip.ptr(partial), hip.ptr(out),
             c_int(_DTYPES[planes.dtype]), c_int(H), c_int(W), c_int(ha), c_int(wa), c_int(x), c_int(y), c_int(n_prev), hip.stream())
    r = out.cpu().numpy()
    return r[:n_prev], r[MAX_PLANES:MAX_PLANES + n_prev], float(r[2 * MAX_PLANES])


def commit(image_u8, fg_canvas_u8, planes, fg_u8, a, xy, idx, dtype=None):
    """The accepted placement, one launch, in place on device tensors: `image_u8` (H, W, 3) gets the masked paste of `fg_u8` through `a`;
    `fg_canvas_u8` (H, W, 3) becomes `fg_u8` on black; plane `idx` becomes a / 255 (0 outside the box); planes 0..idx-1 are multiplied by
    1 - a / 255 in their dtype. `image_u8`, `fg_canvas_u8` (and with both `fg_u8`) may be None."""
    P, H, W = _planes(planes, dtype)
    idx = integer(idx, 'idx')
    if not 0 <= idx < P:
        raise ValueError('idx must be in 0..%d (got %d)' % (P - 1, idx))
    a, ha, wa, _ = _single(a, 'a', 1)
    x, y = _xy(xy)
    for t, what in ((image_u8, 'image'), (fg_canvas_u8, 'fg_canvas')):
        if t is not None:
            if not torch.is_tensor(t) or t.dtype != torch.uint8 or tuple(t.shape) != (H, W, 3) or not t.is_contiguous():
                raise ValueError('%s must be a contiguous uint8 device tensor of shape %s' % (what, (H, W, 3)))
    fg = None
    if fg_u8 is not None:
        fg, fh, fw, _ = _single(fg_u8, 'fg', 3)
        if (fh, fw) != (ha, wa):
            raise ValueError('fg: expected %d x %d like a (got %d x %d)' % (ha, wa, fh, fw))
    elif image_u8 is not None or fg_canvas_u8 is not None:
        raise ValueError('fg is needed to paste into image or fg_canvas')
    hip.need_cuda(planes, image_u8, fg_canvas_u8)
    a = to_device(a, planes.device)
    fg = None if fg is None else to_device(fg, planes.device)
    hip.call('mg_compose_commit', hip.ptr(image_u8), hip.ptr(fg_canvas_u8), hip.ptr(planes), hip.ptr(fg), hip.ptr(a),
             hip.ptr(unit_table(planes.dtype, planes.device)), c_int(_DTYPES[planes.dtype]), c_int(H), c_int(W), c_int(ha), c_int(wa), c_int(x),
             c_int(y), c_int(idx), hip.stream())


def planes_u8(planes):
    """((plane * 255) truncated to uint8, int32 (P,) flags: 1 where the plane holds a non-zero value), both on the device; no read-back."""
    P, H, W = _planes(planes)
    hip.need_cuda(planes)
    out = torch.empty((P, H, W), dtype=torch.uint8, device=planes.device)
    flags = torch.empty((P,), dtype=torch.int32, device=planes.device)
    hip.call('mg_compose_planes_u8', hip.ptr(planes), hip.ptr(out), hip.ptr(flags), c_int(_DTYPES[planes.dtype]), c_long(P), c_int(H), c_int(W),
             hip.stream())
    return out, flags


def alpha_box(alpha_u8, device=None):
    """(x, y, w, h) of alpha > 0, as `cv2.boundingRect` reports it, of one (H, W) uint8 plane; one read-back of 16 bytes. An all-zero plane
    raises ValueError (the tools crop to an empty box there and fail)."""
    a, h, w, _ = _single(alpha_u8, 'alpha', 1)
    a = to_device(a, device)
    box = torch.empty((4,), dtype=torch.int32, device=a.device)
    hip.call('mg_compose_alpha_box', hip.ptr(a), hip.ptr(box), c_int(h), c_int(w), hip.stream())
    x0, y0, x1, y1 = (int(v) for v in box.cpu().numpy())
    if x1 < 0:
        raise ValueError('the alpha plane is all zero: there is no box')
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


# ---- the image tool -----------------------------------------------------------------------------------------------------------------------------
def draw_sources(random, n_fg_files, n_bg_files):
    """The image tool's two file draws (synthesize_image_him.py:25, 42) as indices into the caller's lists: (2..4 distinct foreground indices,
    one background index). The tool draws nothing between them, so both are made here; the caller decodes the files and passes the same
    `random` on to `synthesize_image(..., random=random)`."""
    fg = random.choice(integer(n_fg_files, 'n_fg_files'), size=(random.randint(2, 5),), replace=False)
    return fg, int(random.choice(integer(n_bg_files, 'n_bg_files')))


def synthesize_image(sample_id, fgs_u8, alphas_u8, bg_u8, jpeg=False, random=None, device=None):
    """`generate_image` (synthesize_image_him.py:33-111) from the decoded arrays on: `fgs_u8` a list of (h, w, 3), `alphas_u8` of (h, w), `bg_u8`
    (H, W, 3). The draws are the tool's, in its order, on `random`, or on `RandomState(sample_id)` when `random` is None (`draw_sources` made
    the file draws on it before). Per instance: box of alpha > 0, crop, bicubic resize to uniform(0.5, 0.9) * H / h, up to three (x, y) draws (a
    resized foreground as wide as the background or wider has an empty range: no draw, no state consumed, the instance is dropped), rejected
    when an earlier instance with area > 0 keeps less than 0.7 of it. Areas are the fp64 sums of `try_place` (the tool's are NumPy's fp32
    sums, about 1e-6 relative away).

    Returns None when nothing was placed, else a dict of device tensors `image` (H, W, 3), `bg`, `alphas` (P', H, W) uint8 of the non-empty
    planes, `fgs` (P', H, W, 3), and `history`: per instance the list of (x, y, accepted). With `jpeg`, `image`, `bg` and `fgs` went through
    `photometric.jpeg_roundtrip(quality=75)`: what a loader decodes from the .jpg files the tool saves (Pillow's default quality)."""
    if len(fgs_u8) != len(alphas_u8) or not 1 <= len(fgs_u8) <= MAX_PLANES:
        raise ValueError('expected 1..%d foregrounds with one alpha each (got %d and %d)' % (MAX_PLANES, len(fgs_u8), len(alphas_u8)))
    bg, H, W, _ = _single(bg_u8, 'bg', 3)
    srcs = []
    for fg, al in zip(fgs_u8, alphas_u8):
        f, fh, fw, _ = _single(fg, 'fg', 3)
        a, ah, aw, _ = _single(al, 'alpha', 1)
        if (fh, fw) != (ah, aw):
            raise ValueError('alpha: expected %d x %d like its foreground (got %d x %d)' % (fh, fw, ah, aw))
        srcs.append((f, a))
    random = np.random.RandomState(sample_id) if random is None else random
    bg = to_device(bg, device)
    dev = bg.device
    srcs = [(to_device(f, dev), to_device(a, dev)) for f, a in srcs]
    boxes = [alpha_box(a) for _, a in srcs]
    inst = []
    for (f, a), (x, y, w, h) in zip(srcs, boxes):
        scale = random.uniform(0.5, 0.9) * H / h
        size, crop = (int(w * scale), int(h * scale)), (x, y, x + w, y + h)
        tables = ResizeTables((w, h), _size(size), 'bicubic').to(dev)
        inst.append((pil_resize(f, size, crop=crop, tables=tables), pil_resize(a, size, crop=crop, tables=tables)))
    n = len(inst)
    image = bg.clone()
    planes = torch.zeros((n, H, W), dtype=torch.float32, device=dev)
    canvases = torch.zeros((n, H, W, 3), dtype=torch.uint8, device=dev)
    history = []
    for i, (f, a) in enumerate(inst):
        h, w = int(a.shape[0]), int(a.shape[1])
        tries, ok = [], False
        for _ in range(3):
            try:
                x = random.randint(0, W - w)
                y = random.randint(0, H - h)
            except ValueError:
                break
            new, old, _ = try_place(planes, a, (x, y), i)
            ok = not np.any((old > 0) & (new / (old + 1e-7) < 0.7))
            tries.append((int(x), int(y), bool(ok)))
            if ok:
                break
        history.append(tries)
        if ok:
            commit(image, canvases[i], planes, f, a, (x, y), i)
    u8, flags = planes_u8(planes)
    keep = np.flatnonzero(flags.cpu().numpy())
    if keep.size == 0:
        return None
    keep = torch.from_numpy(keep).to(dev)
    out = {'image': image, 'bg': bg, 'alphas': u8[keep], 'fgs': canvases[keep], 'history': history}
    if jpeg:
        for k in ('image', 'bg', 'fgs'):
            out[k] = photometric.jpeg_roundtrip(out[k], 75)
    return out


# ---- the video tool -----------------------------------------------------------------------------------------------------------------------------
LEVELS = ('easy', 'medium', 'hard')
OCCLUDED_ABORT = {'easy': None, 'medium': 0.3, 'hard': 0.85}                # synthesize_video_him.py:179: a frame pair above it drops the clip
OCCLUDED_KEEP = {'easy': None, 'medium': 0.05, 'hard': 0.5}                 # :196-201: the caller drops a clip whose max_occluded is below it


STRETCH = {'easy': None, 'medium': (1.0, 1.5), 'hard': (1.0, 2.0)}          # :101-104: the random factor on an instance's share of the width


def _video_scales(rs, level, bg_h, bg_w, widths, heights):
    """Per instance the resize factor (:95-107): the instances share the background's width in proportion to their aspect, a level's
    stretch is one uniform draw, and a result taller than the background is replaced by its height times uniform(0.8, 1.0)."""
    aspects = [bw * 1.0 / bh for bw, bh in zip(widths, heights)]
    whole = sum(aspects)
    scales = []
    for aspect, bw, bh in zip(aspects, widths, heights):
        s = bg_w * (aspect / whole) / bw
        if STRETCH[level] is not None:
            s = s * rs.uniform(*STRETCH[level])
        if s * bh > bg_h:
            s = bg_h / bh * rs.uniform(0.8, 1.0)
        scales.append(s)
    return scales


def _video_corners(rs, level, bg_h, bg_w, sizes):
    """Per instance (left, top) (:110-127): left to right from 0, each instance starting where the one before ended; off 'easy' moved by a
    drawn distance below half the width (the distance first, then its sign); kept inside on the right, then on the left; standing on the
    bottom edge."""
    cursor, corners = 0, []
    for nw, nh in sizes:
        left = cursor
        if level != 'easy':
            distance = rs.randint(0, bg_w // 2)
            left = cursor + distance * rs.choice([-1, 1])
        left = max(min(left, bg_w - nw), 0)
        corners.append((int(left), bg_h - nh))
        cursor = left + nw
    return corners


def plan_video(random_state, level, bg_hw, boxes, n_bg_frames=1):
    """The geometry of `gen_video` (synthesize_video_him.py:91-131), pure host code with the tool's draws in its order on `random_state`:
    `boxes` are the instances' (x, y, w, h) over their clips, `bg_hw` the background's (height, width), `n_bg_frames` the number of
    background frames. Returns a dict: `ratios`, `boxes`, `placed` = [(x1, y1, new_w, new_h)] with the int() sizes, x1 jittered (not at
    'easy') and clamped to the width (to 0 last, so a wide instance hangs over the right edge), y1 = h - new_h, and `start_bg_frame`,
    one more draw when there are several background frames."""
    if level not in LEVELS:
        raise ValueError('level must be one of %r (got %r)' % (LEVELS, level))
    bg_h, bg_w = integer(bg_hw[0], 'bg_hw'), integer(bg_hw[1], 'bg_hw')
    boxes = [tuple(integer(v, 'a box') for v in b) for b in boxes]
    if not boxes or any(len(b) != 4 or b[2] < 1 or b[3] < 1 for b in boxes):
        raise ValueError('boxes must be non-empty (x, y, w, h) with w, h >= 1 (got %r)' % (boxes,))
    widths, heights = [b[2] for b in boxes], [b[3] for b in boxes]
    scales = _video_scales(random_state, level, bg_h, bg_w, widths, heights)
    sizes = [(int(bw * s), int(bh * s)) for bw, bh, s in zip(widths, heights, scales)]
    corners = _video_corners(random_state, level, bg_h, bg_w, sizes)
    start = int(random_state.randint(0, n_bg_frames - 1)) if n_bg_frames > 1 else 0
    return {'ratios': scales, 'boxes': boxes, 'placed': [c + sz for c, sz in zip(corners, sizes)], 'start_bg_frame': start}


def video_frame(bg_u8, fgrs_u8, alphas_u8, plan, level, device=None):
    """One frame of `gen_video` (synthesize_video_him.py:136-184): per instance crop to its box, bilinear resize, masked paste into the
    frame, the alpha canvas / 255 as an fp64 plane, and the earlier planes times 1 - it. `occluded` = 1 - new_area / (area + 1e-7) of every
    earlier plane with area > 0, from `try_place`'s fp64 sums. Returns (frame (H, W, 3) uint8, planes (n, H, W) fp64, max_occluded, abort):
    `abort` when an `occluded` passed the level's threshold (0.3 medium, 0.85 hard) -- the tool drops the clip there, so frame and planes are
    None and max_occluded is the largest value before it. The caller keeps max_occluded over the clip and applies OCCLUDED_KEEP."""
    if level not in LEVELS:
        raise ValueError('level must be one of %r (got %r)' % (LEVELS, level))
    bg, H, W, _ = _single(bg_u8, 'bg', 3)
    n = len(plan['placed'])
    if len(fgrs_u8) != n or len(alphas_u8) != n or not 1 <= n <= MAX_PLANES:
        raise ValueError('expected the %d foregrounds and alphas of the plan (got %d and %d)' % (n, len(fgrs_u8), len(alphas_u8)))
    frame = to_device(bg, device).clone()
    dev = frame.device
    planes = torch.zeros((n, H, W), dtype=torch.float64, device=dev)
    limit, most = OCCLUDED_ABORT[level], 0.0
    for i, (fgr, al, (bx, by, bw, bh), (x1, y1, nw, nh)) in enumerate(zip(fgrs_u8, alphas_u8, plan['boxes'], plan['placed'])):
        crop = (bx, by, bx + bw, by + bh)
        tables = ResizeTables((bw, bh), _size((nw, nh)), 'bilinear').to(dev)
        a = pil_resize(al, (nw, nh), 'bilinear', crop, device=dev, tables=tables)
        f = pil_resize(fgr, (nw, nh), 'bilinear', crop, device=dev, tables=tables)
        new, old, _ = try_place(planes, a, (x1, y1), i)
        # the tool walks j upwards and stops at the first pair past the threshold: planes below it are already multiplied, the rest not
        stop = None
        for j in range(i):
            if old[j] > 0:
                o = 1.0 - new[j] / (old[j] + 1e-7)
                if limit is not None and o > limit:
                    stop = j
                    break
                most = max(most, o)
        if stop is not None:
            return None, None, float(most), True
        commit(frame, None, planes, f, a, (x1, y1), i)
    return frame, planes, float(most), False
