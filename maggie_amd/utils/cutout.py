"""Cut-outs on the device (HIP kernels of csrc/cutout.hip): what a user of a matting model takes away. `matteout.composite` blends the frame with
a green screen, which is a preview: in every pixel with 0 < a < 1 the frame is already a mix of the subject and the old background, and
re-compositing it drags that background along as a halo. Here the other half of the matting equation is estimated, the foreground colour F,
and written with the matte as a straight (not premultiplied) RGBA image.

  * `estimate_foreground`  the blur-fusion estimator (Forte & Pitie, "Approximate Fast Foreground Colour Estimation", ICIP 2021), applied
                           twice with the radii 90 and 6, per instance.
  * `cutout`               RGBA: the estimate, the alpha byte, RGB 0 where the alpha byte is 0; with `transform_info` the alpha goes through
                           `postprocessing.reverse_transform_tensor` first, as `composite`'s default form does, or with `refine=` through
                           the guided filter of utils/refine.py.
  * `save_cutouts`         `out_dir/NN_<stem>.png` through one `pngenc.encode_images`.

The estimator is STATED ON BYTES (tests/cutout_restatement.py is the statement in NumPy and the byte-for-byte oracle): the
frame is uint8, the alpha is the byte the evaluation's PNG stores (a uint8 plane as it is, an fp32 plane by the rule of `pngenc`'s 'unit' mode:
(uint8)(x * 255.0f), NaN and negatives 0, >= 1 gives 255), every window sum is an exact integer, the formula runs in fp64 with every operation
rounded on its own, and the estimates of the first pass are rounded to bytes before the second. No equality with a float implementation
(OpenCV's `cv2.blur` form) is claimed; the rounding between the passes costs at most 1/510 of the range, far below the estimator's own error.

The input contract is that of utils/_inputs.py: the frames are uint8, a tensor or an array, on the host or on the device; the alpha is a device
tensor; TypeError / ValueError before anything touches the device; `hip.MaggieHipError` without a GPU. Nothing is read back and the launches form
one chain on the current stream, so both functions can be captured in a graph. There is no CPU fallback."""
import os

import torch

from .. import hip
from ..hip import c_int, c_long
from . import postprocessing
from . import refine as _refine
from ._inputs import check_u8, integer, need_gpu, to_device
from .matteout import _frames

RADII = (90, 6)
MAX_RADIUS, MAX_SIDE = 255, 32767            # MG_CUTOUT_MAX_RADIUS / _MAX_SIDE (include/maggie_hip.h)
SCRATCH_BYTES = 256 << 20                    # the row sums of one chunk of planes: 28 bytes a pixel and plane


def _radii(radii):
    if not isinstance(radii, (tuple, list)) or len(radii) != 2:
        raise ValueError('radii must be two ints of 1..%d (got %r)' % (MAX_RADIUS, radii))
    r = tuple(integer(v, 'a radius') for v in radii)
    if not all(1 <= v <= MAX_RADIUS for v in r):
        raise ValueError('radii must be two ints of 1..%d (got %r)' % (MAX_RADIUS, radii))
    return r


def _checked(frames_u8, alpha, radii, transform_info=None):
    """Everything that can be wrong with the arguments, before the device is touched -> (frames tensor, T, H, W, P, radii)."""
    f, _, T, H, W = _frames(frames_u8)
    if not torch.is_tensor(alpha):
        raise TypeError('alpha must be a device tensor (got %s)' % type(alpha).__name__)
    if alpha.dtype not in (torch.float32, torch.uint8):
        raise TypeError('alpha must be float32 or uint8 (got %s)' % alpha.dtype)
    if transform_info is not None and alpha.dtype != torch.float32:
        raise TypeError('an alpha that goes through the reverse transform is float32 (got %s)' % alpha.dtype)
    if alpha.dim() < 3:
        raise ValueError('alpha must be (..., P, H, W) (got shape %s)' % (tuple(alpha.shape),))
    P, h, w = (int(v) for v in alpha.shape[-3:])
    if h < 1 or w < 1 or alpha.numel() != T * P * h * w:
        raise ValueError('alpha of shape %s does not hold P planes for each of %d frames' % (tuple(alpha.shape), T))
    if transform_info is None and (h, w) != (H, W):
        raise ValueError('the alpha is %d x %d, the frames are %d x %d' % (h, w, H, W))
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError('sides of 1..%d are taken (got %d x %d)' % (MAX_SIDE, H, W))
    return f, T, H, W, P, _radii(radii)


def _run(f, alpha, T, P, H, W, radii, channels, device):
    need_gpu(alpha)
    hip.need_cuda(alpha)
    f = to_device(f, alpha.device if device is None else device)
    if f.device != alpha.device:
        raise ValueError('frames on %s, alpha on %s' % (f.device, alpha.device))
    n = T * P
    with torch.cuda.device(f.device):
        out = torch.empty((T, P, H, W, channels), dtype=torch.uint8, device=f.device)
        if n == 0:
            return out
        a = alpha.reshape(n, H, W).contiguous()
        st = hip.stream
        if a.dtype == torch.float32:
            a8 = torch.empty((n, H, W), dtype=torch.uint8, device=f.device)
            hip.call('mg_cutout_alpha_bytes', hip.ptr(a), c_long(n * H * W), hip.ptr(a8), st())
            a = a8
        most = max(1, min(n, SCRATCH_BYTES // (28 * H * W)))
        chunk = -(-n // -(-n // most))                       # chunks of equal size: five planes where four fit go as 3 + 2, not 4 + 1
        rows = torch.empty((chunk, 7, H, W), dtype=torch.int32, device=f.device)
        f1 = torch.empty((2, chunk, H, W, 3), dtype=torch.uint8, device=f.device)
        hip.call('mg_cutout_estimate', hip.ptr(f), hip.ptr(a), c_long(T), c_int(P), c_int(H), c_int(W), c_int(radii[0]), c_int(radii[1]),
                 hip.ptr(rows), hip.ptr(f1[0]), hip.ptr(f1[1]), c_long(chunk), hip.ptr(out), c_int(channels), st())
    return out


def estimate_foreground(frames_u8, alpha, *, radii=RADII, device=None):
    """The foreground colour of every instance of every frame, by the statement of DESIGN.md section 35.

    frames_u8: (H, W, 3) or (T, H, W, 3) uint8 (tensor or array, host or device). alpha: a DEVICE tensor (..., P, H, W) with T * P planes at
    the frames' size, uint8 (taken as it is) or float32 (the 'unit' byte). radii: the window sides of the two passes, each 1..255; an image
    smaller than a window is legal (the border is reflected as often as needed). Returns uint8 (T, P, H, W, 3). TypeError for a wrong dtype,
    ValueError for a wrong shape or radius, both before any launch; T * P = 0 returns an empty tensor without a launch. The scratch (uint32
    row sums, 28 bytes a pixel and plane, and the first pass's estimates) is allocated per call for at most `SCRATCH_BYTES` of row sums: a
    long clip is processed in chunks of planes. No read-back: capturable in a graph."""
    f, T, H, W, P, r = _checked(frames_u8, alpha, radii)
    return _run(f, alpha, T, P, H, W, r, 3, device)


def cutout(frames_u8, alpha, *, transform_info=None, snap=False, radii=RADII, refine=False, device=None):
    """Straight RGBA cut-outs, uint8 (T, P, H, W, 4): A is the alpha byte, RGB the estimate of `estimate_foreground`, and RGB is 0 where A is 0
    (hidden colour is useless and costs file size). With `transform_info` (the loader's list) the float32 alpha is at the network's size and
    first goes through `postprocessing.reverse_transform_tensor(alpha, transform_info, snap=snap)`. With `refine` (True, or a dict with `radius`
    and / or `eps`) the alpha bytes are those of `refine.refine(frames_u8, alpha, transform_info=transform_info, snap=snap, ...)` instead: the
    guided filter against the full-size frame in place of the bilinear reverse transform. Errors and capture as `estimate_foreground`."""
    opts = _refine.options(refine)
    if opts is not None:
        r = _radii(radii)
        a8 = _refine.refine(frames_u8, alpha, transform_info=transform_info, snap=snap, device=device, **opts)
        T, P, H, W = (int(v) for v in a8.shape)
        return _run(_frames(frames_u8)[0], a8, T, P, H, W, r, 4, device)
    f, T, H, W, P, r = _checked(frames_u8, alpha, radii, transform_info)
    if transform_info is not None and T * P:
        need_gpu(alpha)
        hip.need_cuda(alpha)
        alpha = postprocessing.reverse_transform_tensor(alpha, transform_info, snap=bool(snap))
        h, w = (int(v) for v in alpha.shape[-2:])
        if (h, w) != (H, W):
            raise ValueError('the alpha comes out at %d x %d, the frames are %d x %d' % (h, w, H, W))
    return _run(f, alpha, T, P, H, W, r, 4, device)


def save_cutouts(cutouts, out_dir, stem):
    """cutouts (P, H, W, 4) uint8 -> `out_dir/NN_<stem>.png` for NN = 00, 01, ..., RGBA files from one `pngenc.encode_images` (the naming of
    `matteout.save_composites`). Returns the paths."""
    from . import pngenc
    from .jpegenc import _write
    c = check_u8(cutouts, 'cutouts')
    if c.dim() != 4 or c.shape[-1] != 4:
        raise ValueError('cutouts must be (P, H, W, 4) (got shape %s)' % (tuple(c.shape),))
    if c.shape[0] == 0:
        return []
    files = pngenc.encode_images(c)
    paths = [os.path.join(out_dir, '%02d_%s.png' % (i, stem)) for i in range(len(files))]
    for p, data in zip(paths, files):
        _write(p, data)
    return paths
