"""RandomAffine of the loaders on the device (HIP kernels of csrc/affine.hip) -- the step the reference runs between the crop / flip and the mask
chain for 10 % of the training items (maggie/dataloader/transforms.py:926-963, dataloader/utils.py:61-221; him.py:49, vim.py:55):

  ... -> RandomCropByAlpha -> RandomHorizontalFlip -> [gamma, noise, JPEG] -> RandomAffine(random, p=affine_p) -> [mask chain] -> ...

  * `draw`         the reference's calls on the loader's `np.random.RandomState` in its order, the matrix composed with the reference's own
                   NumPy calls (rotation . shear . zoom, the offset centre with h and w swapped, the flipped matrix handed to cv2), OpenCV's
                   inversion operation for operation and the four fixed-point tables of cv2.warpAffine (pure host code);
  * `from_matrix`  the same tables for any 2 x 3 matrix;
  * `warp`         cv2.warpAffine of the stacked uint8 arrays: INTER_LINEAR for the 3-channel frames, INTER_NEAREST for the 2-D alphas (the
                   reference's behaviour), BORDER_CONSTANT 0, the destination as large as the source;
  * `apply`        `warp`, then the float64 channel shift of the frames clipped to each warped frame's own min / max, ToTensor and Normalize.

OpenCV is not a dependency: the warp restates the documented classic fixed-point path for uint8 (AB_BITS = 10, round_delta 512 / 16, five
fractional bits and integer weights of sum 32768 for INTER_LINEAR). Newer OpenCV releases carry a second INTER_LINEAR implementation; which
one a given wheel takes is not checked here. Everything on the device is integer work, the float64 add and clamp, or the IEEE divisions of
Normalize: bit-exact, no tolerance anywhere. An `AffineDraws` moved to the device (`.to(device)`) makes `apply` upload nothing and never
synchronise, so it can be captured in a graph and new tables and a new intensity written into `linear`, `nearest` and `shift` between replays.

The bracketed steps in front of it have device forms of their own (the tone curve as `lut` of utils/crop.py, noise and JPEG in
utils/photometric.py; `DevicePreprocessor.train_item_photo` runs them between the crop and this warp). The masks are not warped (the reference leaves them alone; `DevicePreprocessor.train_item_affine` has the two loaders' wirings), and `ignore_regions`,
which the reference writes and nobody reads, is not produced. Wrong dtype, rank or size raise before a launch. There is no CPU fallback."""
import numpy as np
import torch

from .. import hip
from ..hip import c_int, c_long
from . import geometry
from ._inputs import IMAGENET_MEAN, IMAGENET_STD, float3, images, int_table, integer, resolve_device, to_device, upload

LINEAR, NEAREST = geometry.LINEAR, geometry.NEAREST
STAGED, DIRECT = 0, 1                      # MG_AFFINE_STAGED / MG_AFFINE_DIRECT (include/maggie_hip.h)
REGIMES = {'staged': STAGED, 'direct': DIRECT}
TILE_ROWS, TILE_COLS, BOX_BYTES, MAX_SIDE = 32, 64, 16384, 32767     # MG_AFFINE_TILE_ROWS / _TILE_COLS / _BOX_BYTES / _MAX_SIDE
AB_BITS, AB_SCALE = 10, 1024
ROUND_DELTA = {NEAREST: AB_SCALE // 2, LINEAR: AB_SCALE // 32 // 2}
LIMIT = 1 << 30                            # table entries are kept inside +-2^30 (a million pixels away): the sum of two is an int32
# The frames' regime when the caller names none: the LDS-staged tiles for clips of at least STAGED_MIN_FRAMES frames whose every tile's source box
# fits, four global taps per pixel otherwise. Both give the same bits (tests/test_gpu_affine.py); DESIGN.md section 18 has the measurement: staged
# is ahead on the 8-frame video item and not on a single frame.
STAGED_MIN_FRAMES = 2


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------
def cv_round(a):
    """cvRound of doubles (half to even), kept inside +-2^30."""
    return np.clip(np.rint(np.asarray(a, np.float64)), -LIMIT, LIMIT - 1).astype(np.int32)


def invert(matrix):
    """The six doubles of the inverse map as cv2.warpAffine computes them (operation for operation: the bits decide the tables); D == 0 gives
    the zero map, as in OpenCV."""
    M0, M1, M2, M3, M4, M5 = (np.float64(v) for v in np.asarray(matrix, np.float64).reshape(-1))
    D = M0 * M4 - M1 * M3
    D = np.float64(1.0) / D if D != 0 else np.float64(0.0)
    A11, A22 = M4 * D, M0 * D
    M0 = A11
    M1 = M1 * -D
    M3 = M3 * -D
    M4 = A22
    b1 = -M0 * M2 - M1 * M5
    b2 = -M3 * M2 - M4 * M5
    return np.asarray([M0, M1, b1, M3, M4, b2], np.float64)


def tables(matrix, H, W, interp):
    """int32 [adelta W | bdelta W | X0 H | Y0 H] of cv2.warpAffine(src, matrix, (W, H)) for `interp` (LINEAR or NEAREST)."""
    m = invert(matrix)
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        adelta, bdelta = cv_round(m[0] * x * AB_SCALE), cv_round(m[3] * x * AB_SCALE)
        X0, Y0 = cv_round((m[1] * y + m[2]) * AB_SCALE) + ROUND_DELTA[interp], cv_round((m[4] * y + m[5]) * AB_SCALE) + ROUND_DELTA[interp]
    return np.ascontiguousarray(np.concatenate([adelta, bdelta, X0, Y0]), np.int32)


def split(table, H, W):
    """(adelta, bdelta, X0, Y0) views of a table buffer."""
    return table[:W], table[W:2 * W], table[2 * W:2 * W + H], table[2 * W + H:2 * W + 2 * H]


def box_bytes(table, H, W):
    """The most LDS bytes any output tile of the staged regime needs for its source box -- the kernel's rule on the host: the box spans the taps
    of the tile's four corners, cut to the image; rows are padded to 16 bytes."""
    adelta, bdelta, X0, Y0 = (t.astype(np.int64) for t in split(np.asarray(table), H, W))
    worst = 0
    for ty0 in range(0, H, TILE_ROWS):
        ty1 = min(ty0 + TILE_ROWS, H) - 1
        for tx0 in range(0, W, TILE_COLS):
            tx1 = min(tx0 + TILE_COLS, W) - 1
            sx = [(X0[a] + adelta[b]) >> AB_BITS for a in (ty0, ty1) for b in (tx0, tx1)]
            sy = [(Y0[a] + bdelta[b]) >> AB_BITS for a in (ty0, ty1) for b in (tx0, tx1)]
            bw = min(max(sx), W - 2) + 1 - max(min(sx), 0) + 1
            bh = min(max(sy), H - 2) + 1 - max(min(sy), 0) + 1
            if bw > 0 and bh > 0:
                worst = max(worst, int(bh) * ((int(bw) * 3 + 15) & ~15))
    return worst


class AffineDraws:
    """The draws of one item's RandomAffine for (H, W) arrays:
      fired      whether the step runs (`rand() <= p`); when it does not, everything below is None / 0 and the item takes the path without it;
      matrix     the (2, 3) float64 matrix the reference hands to cv2.warpAffine, or None when the transform is the identity (the tables are
                 the identity's then: the warp reproduces its source);
      intensity  the channel shift, a Python float;  form  which shear matrix was drawn (0 / 1, None without shear);
      linear, nearest   int32 [adelta W | bdelta W | X0 H | Y0 H]: the four tables of each interpolation (`tables_of(interp)` splits them);
      shift      float64 [1]: the intensity where the kernel reads it;
      staged_ok  whether every tile's source box fits the LDS budget of the staged regime (from the host tables).
    NumPy arrays as drawn; `.to(device)` gives the same record with device tensors. `apply` with that uploads nothing and does not synchronise:
    capture it in a graph and write new tables and a new intensity between replays (the kernels range-test every index they derive)."""

    def __init__(self, fired, H, W, matrix=None, intensity=0.0, form=None, linear=None, nearest=None, shift=None, staged_ok=False):
        self.fired, self.H, self.W, self.matrix, self.intensity, self.form = bool(fired), int(H), int(W), matrix, float(intensity), form
        self.linear, self.nearest, self.shift, self.staged_ok = linear, nearest, shift, bool(staged_ok)

    @property
    def on_device(self):
        return torch.is_tensor(self.linear)

    def tables_of(self, interp):
        return split(self.linear if interp == LINEAR else self.nearest, self.H, self.W)

    def to(self, device=None):
        device = resolve_device(device)
        return AffineDraws(self.fired, self.H, self.W, self.matrix, self.intensity, self.form, upload(self.linear, device),
                           upload(self.nearest, device), upload(self.shift, device), self.staged_ok)


def _size(H, W):
    H, W = integer(H, 'H'), integer(W, 'W')
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError('the arrays must be 1..%d pixels a side (got %d x %d)' % (MAX_SIDE, H, W))
    return H, W


def from_matrix(matrix, H, W, intensity=0., form=None):
    """Fired draws for an arbitrary (2, 3) matrix (what cv2.warpAffine is handed: it maps source to destination and is inverted here), or
    None for the identity."""
    H, W = _size(H, W)
    if matrix is not None:
        matrix = np.array(matrix, dtype=np.float64)
        if matrix.shape != (2, 3) or not np.isfinite(matrix).all():
            raise ValueError('matrix must be a finite (2, 3) array (got %r)' % (matrix,))
    m = np.asarray([[1., 0., 0.], [0., 1., 0.]]) if matrix is None else matrix
    linear, nearest = tables(m, H, W, LINEAR), tables(m, H, W, NEAREST)
    return AffineDraws(True, H, W, matrix, float(intensity), form, linear, nearest, np.asarray([intensity], np.float64),
                       box_bytes(linear, H, W) <= BOX_BYTES)


def _offset_center(matrix, x, y):
    o_x = float(x) / 2 + 0.5
    o_y = float(y) / 2 + 0.5
    offset_matrix = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset_matrix = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    return np.dot(np.dot(offset_matrix, matrix), reset_matrix)


def draw(random, H, W, p=0.1, rt=10, sh=5, zm=(0.95, 1.05), cs=0.03 * 255.):
    """RandomAffine.__call__ + random_transform as draws: the reference's calls on `random` (the loader's np.random.RandomState) in the
    reference's order, leaving it in the reference's state -- rand() (skipped when > p), uniform theta, uniform shear, uniform zx, zy, random()
    for the shear form (only when shear != 0), uniform intensity (after the warp). The matrices are made with the reference's NumPy calls in
    its order, so the float64 bits agree; `transform_matrix_offset_center` gets h as x and w as y, as the reference calls it. Pure host code."""
    H, W = _size(H, W)
    if random.rand() > p:
        return AffineDraws(False, H, W)
    theta = np.pi / 180 * random.uniform(-rt, rt) if rt else 0
    shear = np.pi / 180 * random.uniform(-sh, sh) if sh else 0
    if zm[0] == 1 and zm[1] == 1:
        zx, zy = 1, 1
    else:
        zx = random.uniform(zm[0], zm[1])
        zy = random.uniform(zm[0], zm[1])
    matrix, form = None, None
    if theta != 0:
        matrix = np.array([[np.cos(theta), -np.sin(theta), 0], [np.sin(theta), np.cos(theta), 0], [0, 0, 1]])
    if shear != 0:
        if random.random() < 0.5:
            form, shear_matrix = 0, np.array([[1, -np.sin(shear), 0], [0, np.cos(shear), 0], [0, 0, 1]])
        else:
            form, shear_matrix = 1, np.array([[np.cos(shear), 0, 0], [np.sin(shear), 1, 0], [0, 0, 1]])
        matrix = shear_matrix if matrix is None else np.dot(matrix, shear_matrix)
    if zx != 1 or zy != 1:
        zoom_matrix = np.array([[zx, 0, 0], [0, zy, 0], [0, 0, 1]])
        matrix = zoom_matrix if matrix is None else np.dot(matrix, zoom_matrix)
    cvM = None
    if matrix is not None:
        M = _offset_center(matrix, H, W)
        cvM = np.zeros_like(M[:2, :])
        cvM[:2, :2] = np.flipud(np.fliplr(M[:2, :2]))
        cvM[:2, 2] = np.flip(M[:2, 2], axis=0)
    intensity = random.uniform(-cs, cs) if cs != 0 else 0.0
    return from_matrix(cvM, H, W, float(intensity), form)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------------
def _regime(draws, regime, frames=1):
    """None: staged for `frames` >= STAGED_MIN_FRAMES where every tile's box fits, else direct; 'staged' / 'direct': forced (the tests run both)."""
    if regime is None:
        return STAGED if (draws.staged_ok and frames >= STAGED_MIN_FRAMES) else DIRECT
    if regime not in REGIMES:
        raise ValueError("regime must be None, 'staged' or 'direct' (got %r)" % (regime,))
    if REGIMES[regime] == STAGED and not draws.staged_ok:
        raise ValueError('the staged regime holds %d bytes of source per tile; these tables need more' % BOX_BYTES)
    return REGIMES[regime]


def _check(frames_u8, alphas_u8, draws, regime):
    if not isinstance(draws, AffineDraws):
        raise TypeError('draws must be an AffineDraws (got %s)' % type(draws).__name__)
    if not draws.fired:
        raise ValueError('the draws did not fire: the item takes the path without RandomAffine')
    f, flead, fn, H, W = images(frames_u8, 3, 'frames')
    if (H, W) != (draws.H, draws.W):
        raise ValueError('the draws were made for %d x %d arrays (got frames of %d x %d)' % (draws.H, draws.W, H, W))
    a = None
    if alphas_u8 is not None:
        x, lead, n, h, w = images(alphas_u8, 1, 'alphas')
        if (h, w) != (H, W):
            raise ValueError('alphas: expected %d x %d like the frames (got %d x %d)' % (H, W, h, w))
        a = (x, lead, n)
    return f, flead, fn, H, W, a, _regime(draws, regime, fn)


def _warp(frames_u8, alphas_u8, draws, regime, device):
    f, flead, fn, H, W, a, regime = _check(frames_u8, alphas_u8, draws, regime)
    f = to_device(f, device)
    dev = f.device
    n = 2 * (H + W)
    linear = int_table(draws.linear, dev, n, 'AffineDraws.linear')
    out_f = torch.empty((fn, H, W, 3), dtype=torch.uint8, device=dev)
    mm = torch.empty((fn, 2), dtype=torch.int32, device=dev)
    if fn > 0:
        hip.call('mg_affine_warp_frames', hip.ptr(f), hip.ptr(out_f), hip.ptr(linear), hip.ptr(mm), c_long(fn), c_int(H), c_int(W), c_int(regime),
                 hip.stream())
    out_a = None
    if a is not None:
        x, lead, pn = a
        x = to_device(x, dev)
        nearest = int_table(draws.nearest, dev, n, 'AffineDraws.nearest')
        out_a = torch.empty((pn, H, W), dtype=torch.uint8, device=dev)
        if pn > 0:
            hip.call('mg_affine_warp_planes', hip.ptr(x), hip.ptr(out_a), hip.ptr(nearest), c_long(pn), c_int(H), c_int(W), hip.stream())
        out_a = out_a.reshape(lead + (H, W))
    return out_f, flead, mm, out_a, dev


def warp(frames_u8, alphas_u8, draws, *, regime=None, return_minmax=False, device=None):
    """cv2.warpAffine of the stacked uint8 arrays of one item with the tables of `draws`: frames (T, H, W, 3) INTER_LINEAR, alphas (P, H, W)
    INTER_NEAREST or None (any leading dimensions), BORDER_CONSTANT 0. Returns (frames, alphas) uint8 on the device in the input layout -- the
    state before the channel shift -- and with `return_minmax` also the (T, 2) int32 min / max of each warped frame. `regime`: 'staged' /
    'direct' forces the frames' kernel form."""
    out_f, flead, mm, out_a, _ = _warp(frames_u8, alphas_u8, draws, regime, device)
    H, W = out_f.shape[1:3]
    out_f = out_f.reshape(flead + (H, W, 3))
    return (out_f, out_a, mm) if return_minmax else (out_f, out_a)


def shift_normalize(frames_u8, minmax, shift, mean=IMAGENET_MEAN, std=IMAGENET_STD, device=None):
    """channel_shift + ToTensor + Normalize of (..., H, W, 3) uint8 frames: ((float)clip(v + shift, min, max) / 255 - mean) / std with the
    add and the clip in float64. `minmax`: int32 (T, 2) per frame; `shift`: a float, or float64 [1] on the device. -> (..., 3, H, W) fp32."""
    f, flead, fn, H, W = images(frames_u8, 3, 'frames')
    f = to_device(f, device)
    dev = f.device
    mm = int_table(minmax, dev, 2 * fn, 'minmax')
    if torch.is_tensor(shift):
        if shift.dtype != torch.float64 or shift.numel() != 1:
            raise ValueError('shift must be one float64 (got %s %s)' % (shift.dtype, tuple(shift.shape)))
        hip.need_cuda(shift)
    else:
        shift = torch.from_numpy(np.asarray(shift, np.float64).reshape(1)).to(dev, non_blocking=True)
    out = torch.empty((fn, 3, H, W), dtype=torch.float32, device=dev)
    if fn > 0:
        hip.call('mg_affine_shift_normalize', hip.ptr(f), hip.ptr(out), hip.ptr(mm), hip.ptr(shift), c_long(fn), c_int(H), c_int(W),
                 float3(mean), float3(std), hip.stream())
    return out.reshape(flead + (3, H, W))


def apply(frames_u8, alphas_u8, draws, mean=IMAGENET_MEAN, std=IMAGENET_STD, *, regime=None, device=None):
    """RandomAffine of fired `draws` on the stacked uint8 arrays of one item, then ToTensor + Normalize of the frames: returns
    (image fp32 (T, 3, H, W), alphas uint8 in the input layout, or None). The uint8 warp of the frames is an intermediate of two launches;
    its per-frame min / max stay on the device between them."""
    out_f, flead, mm, out_a, dev = _warp(frames_u8, alphas_u8, draws, regime, device)
    H, W = out_f.shape[1:3]
    image = shift_normalize(out_f, mm, draws.shift if draws.shift is not None else draws.intensity, mean, std, dev)
    return image.reshape(flead + (3, H, W)), out_a
