"""NumPy restatement of the loaders' RandomAffine (maggie/dataloader/transforms.py:926-963, dataloader/utils.py:61-221: random_transform,
apply_transforms_cv, channel_shift), for the tests only -- the product never imports it.

It builds on tests/geometry_restatement.py and adds, from OpenCV's DOCUMENTED algorithm (OpenCV is not a dependency of this project: an unpinned
third-party restatement), `cv2.warpAffine` of uint8 arrays through the classic fixed-point path: the matrix inverted in double operation for
operation, the four AB_BITS = 10 tables, INTER_NEAREST with round_delta 512, INTER_LINEAR with round_delta 16, 5 fractional bits and the four
integer weights of sum 32768, BORDER_CONSTANT 0 per tap. Newer OpenCV releases carry a second INTER_LINEAR implementation; which one a given
wheel takes is not checked here.

  * `random_affine`   the reference's code path line by line on a `np.random.RandomState`; tests/golden/make_affine_golden.py runs the
                      reference's own class beside it (tests/golden/affine_pinned.npz);
  * `draws`, `tables`, `warp_linear`, `warp_nearest`, `channel_shift`, `shift_normalized`   the same from tables: what the device computes.
The seeded inputs of the fixture are regenerated here: it stores outputs only."""
import numpy as np

import geometry_restatement as R
from crop_restatement import state_digest                             # noqa: F401  (the fixture's generator digest)

INTER_NEAREST, INTER_LINEAR = R.INTER_NEAREST, R.INTER_LINEAR
AB_BITS, AB_SCALE = 10, 1024
LIMIT = 1 << 30                            # table entries are kept inside +-2^30: the sum of two of them is an int32


# ---- OpenCV, restated ----------------------------------------------------------------------------------------------------------------------------
def cv_round(a):
    """cvRound of doubles: half to even; kept inside +-2^30 (about a million pixels: far outside any image either way)."""
    return np.clip(np.rint(np.asarray(a, np.float64)), -LIMIT, LIMIT - 1).astype(np.int64)


def invert(M):
    """The six doubles of the inverse map, computed as OpenCV does (no library inverse: the bits matter)."""
    M = np.asarray(M, np.float64).reshape(-1)
    assert M.size == 6
    M0, M1, M2, M3, M4, M5 = (np.float64(v) for v in M)
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


def tables(M, H, W, interpolation):
    """(adelta [W], bdelta [W], X0 [H], Y0 [H]) int64 for a (H, W) destination."""
    m = invert(M)
    round_delta = AB_SCALE // 2 if interpolation == INTER_NEAREST else AB_SCALE // 32 // 2
    x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    adelta, bdelta = cv_round(m[0] * x * AB_SCALE), cv_round(m[3] * x * AB_SCALE)
    X0 = cv_round((m[1] * y + m[2]) * AB_SCALE) + round_delta
    Y0 = cv_round((m[4] * y + m[5]) * AB_SCALE) + round_delta
    return adelta, bdelta, X0, Y0


def _taps(src, sy, sx):
    """src[..., sy, sx, (c)] with 0 where the tap is outside; src (H, W) or (H, W, C), sy / sx int arrays of the output's shape."""
    H, W = src.shape[:2]
    inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    v = src[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)].astype(np.int64)
    return np.where(inside if src.ndim == 2 else inside[..., None], v, 0)


def warp_nearest(src, tabs):
    adelta, bdelta, X0, Y0 = tabs
    sx = (X0[:, None] + adelta[None, :]) >> AB_BITS                           # arithmetic shifts: negative coordinates floor
    sy = (Y0[:, None] + bdelta[None, :]) >> AB_BITS
    return _taps(src, sy, sx).astype(np.uint8)


def warp_linear(src, tabs):
    adelta, bdelta, X0, Y0 = tabs
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    if src.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    acc = (32 * (32 - fx) * (32 - fy) * _taps(src, sy, sx) + 32 * fx * (32 - fy) * _taps(src, sy, sx + 1) +
           32 * (32 - fx) * fy * _taps(src, sy + 1, sx) + 32 * fx * fy * _taps(src, sy + 1, sx + 1))
    return ((acc + 16384) >> 15).astype(np.uint8)


def warpAffine(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=0, borderValue=0):
    """cv2.warpAffine of a uint8 (H, W) plane or (H, W, C) image: INTER_LINEAR or INTER_NEAREST, BORDER_CONSTANT 0, no WARP_INVERSE_MAP."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3) and flags in (INTER_LINEAR, INTER_NEAREST) and borderMode == 0 and borderValue == 0
    dw, dh = int(dsize[0]), int(dsize[1])
    tabs = tables(np.asarray(M, np.float64), dh, dw, flags)
    return warp_linear(src, tabs) if flags == INTER_LINEAR else warp_nearest(src, tabs)


def cv2_standin():
    """geometry_restatement's stand-in `cv2` with warpAffine."""
    cv2 = R.cv2_standin()
    cv2.warpAffine = warpAffine
    return cv2


# ---- the reference's code path -----------------------------------------------------------------------------------------------------------------
def offset_center(matrix, x, y):
    o_x = float(x) / 2 + 0.5
    o_y = float(y) / 2 + 0.5
    offset_matrix = np.array([[1, 0, o_x], [0, 1, o_y], [0, 0, 1]])
    reset_matrix = np.array([[1, 0, -o_x], [0, 1, -o_y], [0, 0, 1]])
    return np.dot(np.dot(offset_matrix, matrix), reset_matrix)


def draws(random, h, w, p=0.1, rt=10, sh=5, zm=(0.95, 1.05), cs=0.03 * 255.):
    """RandomAffine.__call__ + random_transform as draws -> (fired, cvM (2, 3) float64 or None, intensity, shear form 0 / 1 / None). The
    calls on `random` and the NumPy calls on the matrices are the reference's, in its order."""
    if random.rand() > p:
        return False, None, 0.0, None
    theta = np.pi / 180 * random.uniform(-rt, rt) if rt else 0
    shear = np.pi / 180 * random.uniform(-sh, sh) if sh else 0
    zx, zy = (1, 1) if zm[0] == 1 and zm[1] == 1 else (random.uniform(zm[0], zm[1]), random.uniform(zm[0], zm[1]))
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
        M = offset_center(matrix, h, w)                                       # h as x and w as y: the reference's swap
        cvM = np.zeros_like(M[:2, :])
        cvM[:2, :2] = np.flipud(np.fliplr(M[:2, :2]))
        cvM[:2, 2] = np.flip(M[:2, 2], axis=0)
    intensity = random.uniform(-cs, cs) if cs != 0 else 0.0
    return True, cvM, float(intensity), form


def channel_shift(frames, intensity):
    """channel_shift on (T, H, W, 3) frames: float64, clipped per frame to the min / max over its three channels."""
    out = []
    for x in frames:
        min_x, max_x = np.min(x), np.max(x)
        out.append(np.clip(x + intensity, min_x, max_x))
    return np.stack(out)


def random_affine(frames, alphas, random, p=0.1):
    """frames (T, H, W, 3) uint8, alphas (P, H, W) uint8 -> a dict: `fired`, `matrix`, `intensity`, `form`, the uint8 warps `frames_u8` and
    `alphas`, and `frames` as the step leaves them (float64 after the shift; the uint8 input when the step is skipped)."""
    h, w = frames[0].shape[:2]
    fired, cvM, intensity, form = draws(random, h, w, p)
    out = {'fired': fired, 'matrix': cvM, 'intensity': intensity, 'form': form}
    if not fired:
        out['frames_u8'], out['alphas'], out['frames'] = frames, alphas, frames
        return out
    if cvM is not None:
        frames = np.stack([warpAffine(x, cvM, (w, h), flags=INTER_LINEAR) for x in frames])
        alphas = np.stack([warpAffine(x, cvM, (w, h), flags=INTER_NEAREST) for x in alphas])
    out['frames_u8'], out['alphas'], out['frames'] = frames, alphas, channel_shift(frames, intensity)
    return out


def minmax(frames_u8):
    """(T, 2) int32: per frame (min, max) over its pixels and channels -- the words the warp launch leaves on the device."""
    f = np.asarray(frames_u8)
    return np.stack([f.reshape(f.shape[0], -1).min(1), f.reshape(f.shape[0], -1).max(1)], 1).astype(np.int32)


def shift_normalized(frames_u8, intensity, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), mm=None):
    """channel_shift in float64, ToTensor's `.float()`, Normalize.norm in fp32: (T, H, W, 3) uint8 -> (T, 3, H, W) fp32. `mm`: (T, 2) min / max
    to clip to instead of the frames' own."""
    f = np.asarray(frames_u8)
    if mm is None:
        x = channel_shift(f, intensity)
    else:
        x = np.stack([np.clip(a + intensity, lo, hi) for a, (lo, hi) in zip(f, np.asarray(mm))])
    x = x.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
    return (x - np.asarray(mean, np.float32).reshape(1, 3, 1, 1)) / np.asarray(std, np.float32).reshape(1, 3, 1, 1)


# ---- seeded inputs (regenerated, never stored) ---------------------------------------------------------------------------------------------------
# the cases of tests/golden/affine_pinned.npz. p = 1 fires whatever rand() returns (it is drawn all the same); 'loader_fires' and 'skipped' use
# the loaders' p = 0.1 with searched seeds; the shear form and the sign of the intensity depend on `rs_seed` too, and the generator asserts them
GOLDEN = {
    'form0_up': dict(seed=801, rs_seed=4, T=1, n=2, h=40, w=56, p=1.0),
    'form1_down': dict(seed=802, rs_seed=3, T=1, n=1, h=56, w=40, p=1.0),
    'clip': dict(seed=803, rs_seed=11, T=3, n=2, h=36, w=52, p=1.0),
    'loader_fires': dict(seed=804, rs_seed=19, T=1, n=2, h=33, w=47, p=0.1),
    'skipped': dict(seed=805, rs_seed=5, T=1, n=2, h=40, w=56, p=0.1),
}


def golden_inputs(name):
    """frames (T, h, w, 3), alphas (T * n, h, w), masks (T * n, h, w) of a case."""
    c = GOLDEN[name]
    alphas = R.alphas_of(c['seed'] + 50, c['T'] * c['n'], c['h'], c['w'])
    return R.frames_of(c['seed'], c['T'], c['h'], c['w']), alphas, R.masks_of(c['seed'] + 100, alphas)


def golden_run(name):
    """`random_affine` on a case with its own seeded generator: (result dict, the generator afterwards)."""
    c = GOLDEN[name]
    frames, alphas, _ = golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    return random_affine(frames, alphas, rs, c['p']), rs
