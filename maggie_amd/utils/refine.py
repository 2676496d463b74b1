"""Full-size mattes on the device (HIP kernels of csrc/refine.hip): the predictor runs the network at `ResizeShort(576)` and
`postprocessing.reverse_transform_tensor` brings the matte back to the photograph's size with a plain bilinear resize, which magnifies every
hair of a 2160 x 3840 frame 3.75 times. The full-size frame holds the edges the matte lost. `refine` is the fast guided filter (He & Sun,
"Fast Guided Filter", 2015): a local linear model alpha ~ a . I + b is fitted at the network's size, against the frame as the network saw it,
and the averaged coefficients, brought to full size bilinearly, are applied to the full-size frame.

The filter is STATED ON BYTES (tests/refine_restatement.py is the statement in NumPy and the byte-for-byte oracle): the
frame and the guide are uint8, the alpha is the byte the evaluation's PNG stores (a uint8 plane as it is, an fp32 plane by the 'unit' rule of
`mg_cutout_alpha_bytes`), the window sums are exact integers, the fit runs in fp64 with every operation rounded on its own, and the coefficients
are rounded to 16 fractional bits before they are averaged. No equality with a float implementation is claimed.

The input contract is that of utils/_inputs.py: the frames (and a guide) are uint8, a tensor or an array, on the host or on the device; the alpha
is a device tensor; TypeError / ValueError before anything touches the device; `hip.MaggieHipError` without a GPU. Nothing is read back and the
launches form one chain on the current stream; once the axis tables of a size are resident (the first call of that size uploads them) the call
can be captured in a graph. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from ._inputs import integer, need_gpu, to_device
from .matteout import _frames, _name, _plan

RADIUS, EPS = 5, 1e-4
MAX_RADIUS, MIN_EPS, MAX_SIDE = 64, 1e-6, 32767        # MG_REFINE_MAX_RADIUS / _MIN_EPS, MG_CUTOUT_MAX_SIDE (include/maggie_hip.h)
SCRATCH_BYTES = 512 << 20                                # the low-resolution scratch of one chunk of frames: 72 + 96 P bytes a pixel
_TABLES = {}


def options(refine):
    """The `refine=` argument of `cutout.cutout` and `matteout.predict_image`: False / None -> None, True -> {}, a dict with `radius` and / or
    `eps` -> the checked dict."""
    if refine is None or refine is False:
        return None
    if refine is True:
        return {}
    if not isinstance(refine, dict):
        raise TypeError('refine must be False, True or a dict with radius and / or eps (got %r)' % (refine,))
    if set(refine) - {'radius', 'eps'}:
        raise ValueError('refine takes radius and eps (got %r)' % (sorted(refine),))
    _params(refine.get('radius', RADIUS), refine.get('eps', EPS))
    return dict(refine)


def _params(radius, eps):
    radius = integer(radius, 'radius')
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError('radius must be an int of 1..%d (got %r)' % (MAX_RADIUS, radius))
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)):
        raise TypeError('eps must be a number in [%g, 1] (got %r)' % (MIN_EPS, eps))
    if not MIN_EPS <= float(eps) <= 1.0:
        raise ValueError('eps must lie in [%g, 1] (got %r)' % (MIN_EPS, eps))
    return radius, float(eps)


def _axis(src, dst):
    """Step 5 of the statement along one axis, in fp64 on the host -> (i0 int32, f float64)."""
    s = (np.arange(dst, dtype=np.float64) + 0.5) * (np.float64(src) / np.float64(dst)) - 0.5
    s = np.clip(s, 0.0, float(src - 1))
    i0 = np.floor(s)
    return i0.astype(np.int32), s - i0


def _tables(h, w, H, W, device):
    key = (h, w, H, W, device.index)
    if key not in _TABLES:
        xi, xf = _axis(w, W)
        yi, yf = _axis(h, H)
        _TABLES[key] = tuple(torch.from_numpy(a).to(device) for a in (xi, xf, yi, yf))
    return _TABLES[key]


def _checked(frames_u8, alpha, transform_info, guide, radius, eps):
    """Everything that can be wrong with the arguments, before the device is touched -> (frames, guide or None, T, P, H, W, h, w, radius, eps)."""
    f, _, T, H, W = _frames(frames_u8)
    if not torch.is_tensor(alpha):
        raise TypeError('alpha must be a device tensor (got %s)' % type(alpha).__name__)
    if alpha.dtype not in (torch.float32, torch.uint8):
        raise TypeError('alpha must be float32 or uint8 (got %s)' % alpha.dtype)
    if alpha.dim() < 3:
        raise ValueError('alpha must be (..., P, h, w) (got shape %s)' % (tuple(alpha.shape),))
    P, h, w = (int(v) for v in alpha.shape[-3:])
    if h < 1 or w < 1 or alpha.numel() != T * P * h * w:
        raise ValueError('alpha of shape %s does not hold P planes for each of %d frames' % (tuple(alpha.shape), T))
    radius, eps = _params(radius, eps)
    if transform_info is not None:
        plan = _plan(transform_info, h, w)
        if plan is None:
            raise ValueError('transform_info must be paddings behind at most one resize (got %r)' % (transform_info,))
        if min(plan) < 1:
            raise ValueError('the paddings of transform_info leave nothing of a %d x %d plane' % (h, w))
        if plan[2:] != (H, W):
            raise ValueError('the alpha comes out at %d x %d, the frames are %d x %d' % (plan[2], plan[3], H, W))
        h, w = plan[:2]
        for tr in transform_info:
            if _name(tr) == 'resize' and 'ratio' in tr:
                ratio = float(tr['ratio'])
                want = (int(H * ratio), int(W * ratio)) if ratio != 1 else (H, W)
                if want != (h, w):
                    raise ValueError('without its padding the alpha is %d x %d; the frame resized by %r is %d x %d' % ((h, w, ratio) + want))
    if max(h, w, H, W) > MAX_SIDE:
        raise ValueError('sides of 1..%d are taken (got %d x %d for %d x %d)' % (MAX_SIDE, h, w, H, W))
    g = None
    if guide is not None:
        g, single, n, gh, gw = _frames(guide, 'guide')
        if n != T or (gh, gw) != (h, w):
            raise ValueError('the guide must be (%d, %d, %d, 3) like the alpha without its padding (got shape %s)' % (T, h, w, tuple(g.shape)))
    return f, g, T, P, H, W, h, w, radius, eps


def refine(frames_u8, alpha, *, transform_info=None, guide=None, radius=RADIUS, eps=EPS, snap=False, as_float=False, device=None):
    """The alpha of every instance of every frame at the frames' size, by the statement of DESIGN.md section 36.

    frames_u8: (H, W, 3) or (T, H, W, 3) uint8 (tensor or array, host or device). alpha: a DEVICE tensor (..., P, h', w') with T * P planes,
    uint8 (taken as it is) or float32 (the 'unit' byte). With `transform_info` (the loader's list) the padding is cropped from the bottom and the
    right, which leaves (h, w), `geometry.plan`'s resized size for the frame; without it the plane covers the whole frame, at any size (larger,
    equal or smaller). guide: uint8 (T, h, w, 3), what the network saw without its padding; by default `geometry.resize` of the frames to
    (h, w), bilinear, and the frames themselves when the sizes are equal. radius: the window side, 1..64; eps: 1e-6..1, in units of the squared
    [0, 1] range. Returns uint8 (T, P, H, W); with `as_float` fp32 byte / 255.0f instead, which is what `matteout.composite` takes. With `snap`
    a byte <= 1 becomes 0 and a byte >= 254 becomes 255. T * P = 0 returns an empty tensor without a launch. The scratch (72 + 96 P bytes a
    low-resolution pixel and frame) is allocated per call, for at most `SCRATCH_BYTES` at a time: a long clip goes in chunks of frames."""
    f, g, T, P, H, W, h, w, radius, eps = _checked(frames_u8, alpha, transform_info, guide, radius, eps)
    need_gpu(alpha)
    hip.need_cuda(alpha)
    f = to_device(f, alpha.device if device is None else device).reshape(T, H, W, 3)
    if f.device != alpha.device:
        raise ValueError('frames on %s, alpha on %s' % (f.device, alpha.device))
    dev = f.device
    n = T * P
    with torch.cuda.device(dev):
        out = torch.empty((T, P, H, W), dtype=torch.float32 if as_float else torch.uint8, device=dev)
        if n == 0:
            return out
        if g is not None:
            g = to_device(g, dev).reshape(T, h, w, 3)
            if g.device != dev:
                raise ValueError('guide on %s, alpha on %s' % (g.device, dev))
        elif (h, w) == (H, W):
            g = f
        else:
            from . import geometry
            g = geometry.resize(f, (w, h), 'linear', channels=3)
        a = alpha.reshape((n,) + tuple(alpha.shape[-2:]))[:, :h, :w].contiguous()
        st = hip.stream
        if a.dtype == torch.float32:
            a8 = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
            hip.call('mg_cutout_alpha_bytes', hip.ptr(a), c_long(n * h * w), hip.ptr(a8), st())
            a = a8
        xi, xf, yi, yf = _tables(h, w, H, W, dev)
        per = max(1, min(T, SCRATCH_BYTES // ((72 + 96 * P) * h * w)))
        gsc = torch.empty((2, per, 9, h, w), dtype=torch.int32, device=dev)                  # row sums, window sums of the guide
        isc = torch.empty((2, per * P, 4, h, w), dtype=torch.int32, device=dev)              # row sums of the instance planes, A and B
        wide = torch.empty((2, per * P, 4, h, w), dtype=torch.float64, device=dev)           # int64 row sums of A and B, the fp64 means
        for t0 in range(0, T, per):
            t1 = min(T, t0 + per)
            hip.call('mg_refine_coefficients', hip.ptr(g[t0:t1]), hip.ptr(a[t0 * P:t1 * P]), c_long(t1 - t0), c_int(P), c_int(h), c_int(w),
                     c_int(radius), hip.ctypes.c_double(eps), hip.ptr(gsc[0]), hip.ptr(gsc[1]), hip.ptr(isc[0]), hip.ptr(isc[1]), hip.ptr(wide[0]),
                     hip.ptr(wide[1]), st())
            o = hip.ptr(out[t0:t1])
            hip.call('mg_refine_apply', hip.ptr(f[t0:t1]), hip.ptr(wide[1]), c_long(t1 - t0), c_int(P), c_int(h), c_int(w), c_int(H), c_int(W),
                     hip.ptr(xi), hip.ptr(xf), hip.ptr(yi), hip.ptr(yf), c_int(int(bool(snap))), None if as_float else o, o if as_float else None, st())
    return out

