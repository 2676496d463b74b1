"""Input geometry of the loaders on the device (HIP kernels of csrc/geometry.hip) -- the stage every reference pipeline starts with
(maggie/dataloader/transforms.py:104-166, wired in him.py:36-41, vim.py:43-46 and demo/maggie_predictor.py:26-32):

  Load -> ResizeShort(short_size) -> PaddingMultiplyBy(64) -> Stack -> ... -> ToTensor -> Normalize

  * `resize`            cv2.resize of uint8 planes or 3-channel frames, INTER_LINEAR or (legacy) INTER_NEAREST;
  * `plan`              ResizeShort + PaddingMultiplyBy for one source size: sizes, pads, tables, `transform_info` (pure host code);
  * `resize_short_pad`  the raw form: resized and padded uint8 frames / alphas / masks plus `transform_info`;
  * `resize_pad_normalize`, `resize_pad_planes`  the fused forms: the resize, the padding and the tensor stage (Normalize; `/ 255` into
    slots; the masks' nearest 1/8 down-scale of him.py:175-176) in ONE launch, no uint8 intermediate.

The interpolation tables are NumPy work on the host (float32 / float64 steps exactly as OpenCV takes them; the linear axis is
`maskgen.resize_axis`), cached per geometry and uploaded once per device. Everything on the device is integer work or IEEE division: the
results are bit-exact, no tolerance anywhere. Once the tables of a geometry are on the device a call uploads nothing and does not
synchronise, so it can be captured in a graph.

OpenCV takes its area path for an exact 2x reduction in both axes; that is `(a + b + c + d + 2) >> 2`, which the fixed-point linear
scheme gives identically (coefficients 1024 / 1024, no shift truncates): no separate path (tests/test_geometry_cpu.py pins the identity).

Wrong dtype, rank or channel count, `short_size < 1` or an empty destination raise before a launch. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, check_u8, float3, images, integer, to_device
from .maskgen import resize_axis

LINEAR, NEAREST = 0, 1                     # MG_RESIZE_LINEAR / MG_RESIZE_NEAREST (include/maggie_hip.h)
RAW, NORM, SLOTS = 0, 1, 2                 # MG_RESIZE_RAW / _NORM / _SLOTS
SHARED_ROWS, DIRECT = 0, 1                 # MG_RESIZE_SHARED_ROWS / MG_RESIZE_DIRECT
TILE_ROWS, TILE_COLS, MAX_ROWS = 32, 64, 68     # MG_RESIZE_TILE_ROWS / _TILE_COLS / _MAX_ROWS
INTERPOLATIONS = {'linear': LINEAR, 'nearest': NEAREST}
REGIMES = {'shared': SHARED_ROWS, 'direct': DIRECT}
_TABLES = {}                               # (H, W, dh, dw) -> host tables
_DEVICE_TABLES = {}                        # (H, W, dh, dw, device index) -> (linear, nearest) uploaded
_PLANS = {}                                # (h, w, short_size, divisor) -> Plan
_DEVICE_MASK8 = {}                         # (plan key, device index) -> the composed mask table, uploaded


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------
def nearest_axis(src, dst):
    """One axis of cv2.resize(INTER_NEAREST) (the legacy rule, not INTER_NEAREST_EXACT): min(floor(d * (1.0 / (dst / src))), src - 1), in double."""
    ifx = 1.0 / (np.float64(dst) / np.float64(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64), src - 1).astype(np.int32)


def tile_rows_read(ofs, src, tile=TILE_ROWS):
    """The most source rows any `tile`-row output tile reads through the row table `ofs` (taps ofs and ofs + 1, clamped)."""
    worst = 0
    for t0 in range(0, len(ofs), tile):
        t1 = min(t0 + tile, len(ofs))
        worst = max(worst, min(int(ofs[t1 - 1]) + 1, src - 1) - int(ofs[t0]) + 1)
    return worst


def resize_tables(H, W, dh, dw):
    """The tables of cv2.resize from (H, W) to (dh, dw), cached: `x`, `y` the linear axes (ofs, c0, c1) with scale 1.0 / (dst / src);
    `nx`, `ny` the nearest indices; `linear` ([dw][3] | [dh][3]) and `nearest` ([dw] | [dh]) the int32 buffers the kernel reads;
    `rows_read` the worst tile's source-row footprint and `regime` the kernel form the host picks from it."""
    H, W, dh, dw = integer(H, 'H'), integer(W, 'W'), integer(dh, 'dh'), integer(dw, 'dw')
    key = (H, W, dh, dw)
    if key in _TABLES:
        return _TABLES[key]
    if H < 1 or W < 1:
        raise ValueError('the source must have at least one pixel (got %d x %d)' % (H, W))
    if dh < 1 or dw < 1:
        raise ValueError('empty destination: %d x %d' % (dh, dw))
    if H * W * 3 >= 2 ** 31 or dh * dw * 3 >= 2 ** 31:
        raise ValueError('an image must have fewer than 2^31 bytes')
    t = {'x': resize_axis(W, dw, 1.0 / (dw / W)), 'y': resize_axis(H, dh, 1.0 / (dh / H)), 'nx': nearest_axis(W, dw), 'ny': nearest_axis(H, dh)}
    t['linear'] = np.concatenate([np.stack([a.astype(np.int32) for a in t[n]], 1).reshape(-1) for n in ('x', 'y')])
    t['nearest'] = np.concatenate([t['nx'], t['ny']]).astype(np.int32)
    t['rows_read'] = tile_rows_read(t['y'][0], H)
    t['regime'] = SHARED_ROWS if t['rows_read'] <= MAX_ROWS else DIRECT
    _TABLES[key] = t
    return t


def _regime(t, regime):
    """None: the host's choice from the row table; 'shared' / 'direct': forced (the tests run both on one input)."""
    if regime is None:
        return t['regime']
    if regime not in REGIMES:
        raise ValueError("regime must be None, 'shared' or 'direct' (got %r)" % (regime,))
    if REGIMES[regime] == SHARED_ROWS and t['rows_read'] > MAX_ROWS:
        raise ValueError('the shared-rows regime holds %d source rows per tile; this geometry reads %d' % (MAX_ROWS, t['rows_read']))
    return REGIMES[regime]


class Plan:
    """ResizeShort(short_size) + PaddingMultiplyBy(divisor) for (h, w) sources: `ratio`, the resized size (`rh`, `rw`; the source's when
    ratio == 1: no resize is performed), `pad_h`, `pad_w`, the output size `out_h`, `out_w`, the `tables` (`resize_tables`) and
    `transform_info` -- the list the reference's transforms append, which `postprocessing.reverse_transform_tensor` reads."""

    def __init__(self, h, w, short_size, divisor):
        self.h, self.w, self.short_size, self.divisor = h, w, short_size, divisor
        self.ratio = short_size * 1.0 / min(w, h)                                     # transforms.py:118
        self.resized = self.ratio != 1
        self.rw, self.rh = (int(w * self.ratio), int(h * self.ratio)) if self.resized else (w, h)
        if self.rw < 1 or self.rh < 1:
            raise ValueError('empty destination: %d x %d scaled by %r is %d x %d' % (h, w, self.ratio, self.rh, self.rw))
        self.pad_h = (divisor - self.rh % divisor) % divisor                          # transforms.py:150-151
        self.pad_w = (divisor - self.rw % divisor) % divisor
        self.out_h, self.out_w = self.rh + self.pad_h, self.rw + self.pad_w
        self.tables = resize_tables(h, w, self.rh, self.rw)
        self.key = (h, w, short_size, divisor)
        self._mask8 = None

    @property
    def transform_info(self):
        return [{'name': 'resize', 'ori_size': (self.h, self.w), 'ratio': self.ratio}, {'name': 'padding', 'pad_size': (self.pad_h, self.pad_w)}]

    def mask8(self):
        """The masks' path as ONE index map: nearest resize, padding, then F.interpolate(mode='nearest') to (out_h // 8, out_w // 8)
        (him.py:175-176; source index min(floor(float32(d) * float32(src / dst)), src - 1)). Returns (mh, mw, vh, vw, table): the output size,
        the part of it that reads the resized mask (the rest reads the padding) and the int32 buffer [vw] | [vh] of source indices."""
        if self._mask8 is None:
            mh, mw = self.out_h // 8, self.out_w // 8
            if mh < 1 or mw < 1:
                raise ValueError('empty destination: a %d x %d mask has no 1/8 size' % (self.out_h, self.out_w))

            def axis(out, small, valid, idx):
                step = np.float32(out) / np.float32(small)
                at = np.arange(small, dtype=np.int64) if small == out else \
                    np.minimum(np.floor(np.arange(small, dtype=np.float32) * step).astype(np.int64), out - 1)
                at = at[at < valid]                                                   # non-decreasing: the padding is a suffix
                return idx[at].astype(np.int32)
            ys = axis(self.out_h, mh, self.rh, self.tables['ny'])
            xs = axis(self.out_w, mw, self.rw, self.tables['nx'])
            self._mask8 = (mh, mw, len(ys), len(xs), np.concatenate([xs, ys]).astype(np.int32))
        return self._mask8


def plan(h, w, short_size, divisor=64):
    """The `Plan` of (h, w) sources, cached. Pure host code: usable without a GPU."""
    h, w, short_size, divisor = integer(h, 'h'), integer(w, 'w'), integer(short_size, 'short_size'), integer(divisor, 'divisor')
    if h < 1 or w < 1:
        raise ValueError('the source must have at least one pixel (got %d x %d)' % (h, w))
    if short_size < 1:
        raise ValueError('short_size must be at least 1 (got %d)' % short_size)
    if divisor < 1:
        raise ValueError('divisor must be at least 1 (got %d)' % divisor)
    key = (h, w, short_size, divisor)
    if key not in _PLANS:
        _PLANS[key] = Plan(h, w, short_size, divisor)
    return _PLANS[key]


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------
def _device_tables(H, W, dh, dw, device):
    key = (H, W, dh, dw, device.index)
    if key not in _DEVICE_TABLES:
        t = resize_tables(H, W, dh, dw)
        _DEVICE_TABLES[key] = (torch.from_numpy(t['linear']).to(device), torch.from_numpy(t['nearest']).to(device))
    return _DEVICE_TABLES[key]


def _launch(x, out, xtab, ytab, slots, images, n_in, n_slots, C, H, W, dh, dw, Ho, Wo, interp, epilogue, regime, mean=None, std=None, thresh=0):
    m = None if mean is None else float3(mean)
    s = None if std is None else float3(std)
    hip.call('mg_resize_u8', hip.ptr(x), hip.ptr(out), hip.ptr(xtab), hip.ptr(ytab), hip.ptr(slots), c_long(images), c_int(n_in), c_int(n_slots),
             c_int(C), c_int(H), c_int(W), c_int(dh), c_int(dw), c_int(Ho), c_int(Wo), c_int(interp), c_int(epilogue), c_int(regime), m, s,
             c_int(int(thresh)), hip.stream())


def _axes(tabs, interp, dw):
    """The (column, row) table views of one interpolation inside its uploaded buffer."""
    t = tabs[interp]
    return (t, t[3 * dw:]) if interp == LINEAR else (t, t[dw:])


def _interp(interpolation):
    if interpolation not in INTERPOLATIONS:
        raise ValueError("interpolation must be 'linear' or 'nearest' (got %r)" % (interpolation,))
    return INTERPOLATIONS[interpolation]


def _raw(x, N, C, H, W, dh, dw, Ho, Wo, interp, regime):
    """(N, H, W[, 3]) device uint8 -> (N, Ho, Wo[, 3]) uint8: resized to (dh, dw), zero padding to the right and below."""
    xt, yt = _axes(_device_tables(H, W, dh, dw, x.device), interp, dw)
    out = torch.empty((N, Ho, Wo) + ((3,) if C == 3 else ()), dtype=torch.uint8, device=x.device)
    if N > 0:
        _launch(x, out, xt, yt, None, N, 1, 1, C, H, W, dh, dw, Ho, Wo, interp, RAW, regime)
    return out


def resize(src_u8, dsize, interpolation='linear', channels=None, regime=None, device=None):
    """cv2.resize(src, dsize, interpolation=...) of uint8 (..., H, W) planes or (..., H, W, 3) frames; `dsize` is (w, h) as in OpenCV.
    Returns a uint8 device tensor. `channels`: 1 or 3; None reads a last dimension of 3 (and a rank of at least 3) as frames.
    `regime`: None (the host picks from the tables), 'shared' or 'direct' -- the same bits from both."""
    x = check_u8(src_u8)
    if channels is None:
        channels = 3 if x.dim() >= 3 and x.shape[-1] == 3 else 1
    if channels not in (1, 3):
        raise ValueError('channels must be 1 or 3 (got %r)' % (channels,))
    interp = _interp(interpolation)
    try:
        dw, dh = dsize
    except (TypeError, ValueError):
        raise TypeError('dsize must be (w, h) (got %r)' % (dsize,))
    dw, dh = integer(dw, 'dsize'), integer(dh, 'dsize')
    x, lead, N, H, W = images(x, channels, 'resize')
    t = resize_tables(H, W, dh, dw)
    rg = _regime(t, regime)
    x = to_device(x, device)
    return _raw(x, N, channels, H, W, dh, dw, dh, dw, interp, rg).reshape(lead + (dh, dw) + ((3,) if channels == 3 else ()))


def _plan_of(H, W, short_size, divisor):
    return short_size if isinstance(short_size, Plan) else plan(H, W, short_size, divisor)


def _check_plan(p, H, W, what):
    if (p.h, p.w) != (H, W):
        raise ValueError('%s: expected %d x %d like the frames (got %d x %d)' % (what, p.h, p.w, H, W))


def resize_short_pad(frames_u8, alphas_u8=None, masks_u8=None, short_size=768, divisor=64, regime=None, device=None):
    """ResizeShort(short_size) -> PaddingMultiplyBy(divisor) of one item: (..., H, W, 3) frames with INTER_LINEAR, (..., H, W) alphas with
    INTER_LINEAR, (..., H, W) masks with INTER_NEAREST, each padded with zeros to the right and below. Returns
    (frames, alphas, masks, transform_info): uint8 device tensors (None where nothing was given) -- the raw form, for `maskgen` or for
    inspection. With ratio == 1 nothing is resized, as in the reference."""
    f, flead, fn, H, W = images(frames_u8, 3, 'frames')
    p = _plan_of(H, W, short_size, divisor)
    rg = _regime(p.tables, regime)
    planes = []
    for x, what in ((alphas_u8, 'alphas'), (masks_u8, 'masks')):
        if x is None:
            planes.append(None)
            continue
        x, lead, n, h, w = images(x, 1, what)
        _check_plan(p, h, w, what)
        planes.append((x, lead, n))
    f = to_device(f, device)
    out = [_raw(f, fn, 3, H, W, p.rh, p.rw, p.out_h, p.out_w, LINEAR, rg).reshape(flead + (p.out_h, p.out_w, 3))]
    for entry, interp in zip(planes, (LINEAR, NEAREST)):
        if entry is None:
            out.append(None)
            continue
        x, lead, n = entry
        x = to_device(x, f.device)
        out.append(_raw(x, n, 1, H, W, p.rh, p.rw, p.out_h, p.out_w, interp, rg).reshape(lead + (p.out_h, p.out_w)))
    return out[0], out[1], out[2], p.transform_info


def resize_pad_planes_u8(planes_u8, short_size=768, divisor=64, interpolation='linear', regime=None, device=None):
    """(..., H, W) uint8 planes -> (..., out_h, out_w) uint8, resized and padded like the frames of their item."""
    x, lead, n, H, W = images(planes_u8, 1, 'planes')
    p = _plan_of(H, W, short_size, divisor)
    _check_plan(p, H, W, 'planes')
    interp, rg = _interp(interpolation), _regime(p.tables, regime)
    x = to_device(x, device)
    return _raw(x, n, 1, H, W, p.rh, p.rw, p.out_h, p.out_w, interp, rg).reshape(lead + (p.out_h, p.out_w))


def resize_pad_normalize(frames_u8, short_size=768, divisor=64, mean=IMAGENET_MEAN, std=IMAGENET_STD, regime=None, device=None):
    """(..., H, W, 3) uint8 frames -> ((..., 3, out_h, out_w) fp32, Plan): ResizeShort, PaddingMultiplyBy, ToTensor and Normalize.norm in
    one launch with no uint8 intermediate. The padding precedes Normalize in the reference, so a padded cell holds (0 / 255 - mean) / std."""
    f, lead, n, H, W = images(frames_u8, 3, 'frames')
    p = _plan_of(H, W, short_size, divisor)
    _check_plan(p, H, W, 'frames')
    rg = _regime(p.tables, regime)
    f = to_device(f, device)
    xt, yt = _axes(_device_tables(H, W, p.rh, p.rw, f.device), LINEAR, p.rw)
    out = torch.empty(lead + (3, p.out_h, p.out_w), dtype=torch.float32, device=f.device)
    if n > 0:
        _launch(f, out, xt, yt, None, n, 1, 1, 3, H, W, p.rh, p.rw, p.out_h, p.out_w, LINEAR, NORM, rg, mean, std)
    return out, p


def resize_pad_planes(planes_u8, short_size=768, divisor=64, interpolation='linear', n_slots=None, slot_ids=None, thresh=0, down8=False,
                      regime=None, device=None):
    """(F, n_i, H, W) uint8 planes -> (F, n_slots, Ho, Wo) fp32 = v / 255 (0 below `thresh`) of the resized and padded plane, plane j of
    every frame written to slot slot_ids[j] (default: identity), other slots zero -- `preprocess.scale_planes` of the planes
    `resize_short_pad` would return, in one launch. `down8` (masks, nearest only): (Ho, Wo) = (out_h // 8, out_w // 8), the nearest
    down-scale of him.py:175-176 folded into the index map; otherwise (Ho, Wo) = (out_h, out_w)."""
    x = check_u8(planes_u8)
    if x.dim() != 4:
        raise ValueError('expected (F, n_i, H, W) planes (got shape %s)' % (tuple(x.shape),))
    F_, n_i, H, W = (int(v) for v in x.shape)
    if n_i < 1 or H < 1 or W < 1:
        raise ValueError('expected at least one plane of at least one pixel (got shape %s)' % (tuple(x.shape),))
    p = _plan_of(H, W, short_size, divisor)
    _check_plan(p, H, W, 'planes')
    interp, rg = _interp(interpolation), _regime(p.tables, regime)
    if down8 and interp != NEAREST:
        raise ValueError('down8 composes index maps: it needs nearest interpolation')
    n_slots = n_i if n_slots is None else integer(n_slots, 'n_slots')
    src = None
    if slot_ids is not None:
        ids = [int(i) for i in slot_ids]
        if len(ids) != n_i or len(set(ids)) != n_i or min(ids) < 0 or max(ids) >= n_slots:
            raise ValueError('slot_ids must name %d distinct slots below %d' % (n_i, n_slots))
        src = np.full((n_slots,), -1, np.int32)
        src[ids] = np.arange(n_i, dtype=np.int32)
        src = np.tile(src, F_)
    elif n_slots != n_i:
        raise ValueError('n_slots != n_i needs slot_ids')
    m8 = p.mask8() if down8 else None
    x = to_device(x, device)
    if down8:
        Ho, Wo, vh, vw, tab = m8
        key = (p.key, x.device.index)
        if key not in _DEVICE_MASK8:
            _DEVICE_MASK8[key] = torch.from_numpy(tab).to(x.device)
        xt, yt = _DEVICE_MASK8[key], _DEVICE_MASK8[key][vw:]
    else:
        Ho, Wo, vh, vw = p.out_h, p.out_w, p.rh, p.rw
        xt, yt = _axes(_device_tables(H, W, p.rh, p.rw, x.device), interp, p.rw)
    table = None if src is None else torch.from_numpy(src).to(x.device, non_blocking=True)
    out = torch.empty((F_, n_slots, Ho, Wo), dtype=torch.float32, device=x.device)
    if F_ > 0:
        _launch(x, out, xt, yt, table, F_, n_i, n_slots, 1, H, W, vh, vw, Ho, Wo, interp, SLOTS, rg, thresh=thresh)
    return out
