"""NumPy restatement of the loaders' input geometry (maggie/dataloader/transforms.py:104-189: ResizeShort, PaddingMultiplyBy, Stack) and of the
evaluation wiring around it (him.py:36-65, demo/maggie_predictor.py:26-50), for the tests only -- the product never imports it.

It builds on tests/maskgen_restatement.py (the 8-bit INTER_LINEAR resize, the mask chain) and adds, again from OpenCV's DOCUMENTED behaviour
(OpenCV is not a dependency of this project: an unpinned third-party restatement):
  * resize of 3-channel interleaved arrays: every channel on its own with the same tables;
  * resize(INTER_NEAREST), the legacy rule (not INTER_NEAREST_EXACT): sx = min(floor(x * (1.0 / (dw / W))), W - 1) in double, y likewise;
  * copyMakeBorder(src, top, bottom, left, right, BORDER_CONSTANT, value=0).
`cv2_standin()` packages both with the rest of maskgen_restatement's stand-in; tests/golden/make_geometry_golden.py runs the reference's own
transform classes over it, which pins the reference's glue (tests/golden/geometry_pinned.npz), not OpenCV. `resize_short_pad` is the same chain
on uint8 arrays with no float stage: what the device computes. The seeded inputs of the fixture are regenerated here: it stores outputs only."""
import numpy as np

import groundtruth_restatement as G
import maskgen_restatement as M

INTER_NEAREST, INTER_LINEAR, BORDER_CONSTANT = M.INTER_NEAREST, M.INTER_LINEAR, 0
_mask_standin = M.cv2_standin


# ---- OpenCV, restated ----------------------------------------------------------------------------------------------------------------------------
def nearest_axis(src, dst):
    ifx = 1.0 / (dst / src)
    return np.asarray([min(int(np.floor(d * ifx)), src - 1) for d in range(dst)], np.int64)


def resize(src, dsize=(0, 0), dst=None, fx=0.0, fy=0.0, interpolation=INTER_LINEAR):
    """cv2.resize of a uint8 (H, W) plane or (H, W, C) interleaved image, INTER_LINEAR or INTER_NEAREST. The third positional argument is
    `dst`, as in OpenCV: GenMaskFromAlpha's misplaced INTER_NEAREST lands there and the interpolation stays linear."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3) and interpolation in (INTER_LINEAR, INTER_NEAREST)
    if src.ndim == 3:
        return np.stack([resize(src[:, :, c], dsize, None, fx, fy, interpolation) for c in range(src.shape[2])], axis=2)
    if interpolation == INTER_LINEAR:
        return M.resize(src, dsize, None, fx, fy, INTER_LINEAR)
    H, W = src.shape
    dh, dw, _, _ = M.resize_geometry(H, W, dsize, fx, fy)
    return src[nearest_axis(H, dh)[:, None], nearest_axis(W, dw)[None, :]]


def copyMakeBorder(src, top, bottom, left, right, borderType, value=0):
    src = np.asarray(src)
    assert borderType == BORDER_CONSTANT and min(top, bottom, left, right) >= 0
    out = np.full((src.shape[0] + top + bottom, src.shape[1] + left + right) + src.shape[2:], value, src.dtype)
    out[top:top + src.shape[0], left:left + src.shape[1]] = src
    return out


def cv2_standin():
    """maskgen_restatement's stand-in `cv2` with the multi-channel / nearest resize and copyMakeBorder."""
    cv2 = _mask_standin()
    cv2.BORDER_CONSTANT = BORDER_CONSTANT
    cv2.resize = resize
    cv2.copyMakeBorder = copyMakeBorder
    return cv2


# ---- the chain on uint8 arrays (what the device computes) ---------------------------------------------------------------------------------------
def plan(h, w, short, divisor=64):
    """(ratio, (rh, rw), (pad_h, pad_w)) of transforms.py:117-120,149-151."""
    ratio = short * 1.0 / min(w, h)
    rw, rh = (int(w * ratio), int(h * ratio)) if ratio != 1 else (w, h)
    return ratio, (rh, rw), ((divisor - rh % divisor) % divisor, (divisor - rw % divisor) % divisor)


def resize_short_pad(frames, alphas, masks, short, divisor=64):
    """frames (T, h, w, 3), alphas (P, h, w), masks (P, h, w) or None -> the same stacked, resized (linear, linear, nearest; nothing when
    ratio == 1) and padded with zeros below and to the right, plus transform_info."""
    h, w = frames[0].shape[:2]
    ratio, (rh, rw), (ph, pw) = plan(h, w, short, divisor)

    def go(xs, interpolation):
        if xs is None:
            return None
        if ratio != 1:
            xs = [resize(x, (rw, rh), interpolation=interpolation) for x in xs]
        return np.stack([copyMakeBorder(x, 0, ph, 0, pw, BORDER_CONSTANT, value=0) for x in xs])
    info = [{'name': 'resize', 'ori_size': (h, w), 'ratio': ratio}, {'name': 'padding', 'pad_size': (ph, pw)}]
    return go(frames, INTER_LINEAR), go(alphas, INTER_LINEAR), go(masks, INTER_NEAREST), info


def scaled(planes_u8, down8=False):
    """him.py:157-158,175-176 on (T, n, H, W) uint8 planes: / 255 in fp32, then F.interpolate(mode='nearest') to (H // 8, W // 8)."""
    x = np.asarray(planes_u8).astype(np.float32) / np.float32(255)
    if down8:
        H, W = x.shape[-2:]
        ys = np.minimum(np.floor(np.arange(H // 8, dtype=np.float32) * (np.float32(H) / np.float32(H // 8))).astype(np.int64), H - 1)
        xs = np.minimum(np.floor(np.arange(W // 8, dtype=np.float32) * (np.float32(W) / np.float32(W // 8))).astype(np.int64), W - 1)
        x = x[..., ys[:, None], xs[None, :]]
    return x


def normalized(frames_u8, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """ToTensor + Normalize.norm in fp32: (T, H, W, 3) uint8 -> (T, 3, H, W)."""
    x = np.asarray(frames_u8).astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
    return (x - np.asarray(mean, np.float32).reshape(1, 3, 1, 1)) / np.asarray(std, np.float32).reshape(1, 3, 1, 1)


# ---- seeded inputs (regenerated, never stored) ---------------------------------------------------------------------------------------------------
def frames_of(seed, T, h, w):
    """(T, h, w, 3) uint8: a stepped colour ramp, two soft blobs per frame (in steps of 16 grey levels) and uniform noise on 2 % of the pixels;
    never 0, so the padding is visible next to it."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((T, h, w, 3), np.float64)
    for t in range(T):
        blobs = G.soft_planes(seed * 7 + t, 2, h, w).astype(np.float64)
        for c in range(3):
            ramp = 40 + 150 * ((c + 1) * yy / max(h - 1, 1) + (3 - c) * xx / max(w - 1, 1)) / 4
            out[t, :, :, c] = np.floor((ramp + (0.3 + 0.1 * c) * blobs[c % 2] - 0.2 * blobs[(c + 1) % 2]) / 16) * 16
    noisy = rng.random((T, h, w, 1)) < 0.02
    out = np.where(noisy, out + rng.integers(-60, 61, (T, h, w, 3)), out)
    return np.clip(np.rint(out), 1, 255).astype(np.uint8)


def alphas_of(seed, n, h, w):
    """(n, h, w) uint8 soft ellipses: their fringes hold the values 1..4 that ToTensor's `< 5` rule zeroes."""
    return G.soft_planes(seed, n, h, w)


def masks_of(seed, alphas):
    """0 / 255 guidance masks: the alphas binarised, 3 % of the pixels flipped -- isolated pixels, which nearest keeps or drops whole and
    linear smears."""
    rng = np.random.default_rng(seed)
    return ((((alphas > 127) ^ (rng.random(alphas.shape) < 0.03))) * 255).astype(np.uint8)


# the cases of tests/golden/geometry_pinned.npz: the smallest shapes at which each thing can go wrong
GOLDEN = {
    'reduce_under_2x': dict(seed=601, T=1, n=2, h=37, w=53, short=24, divisor=64),       # non-integer reduction under 2x: shared rows
    'enlarge': dict(seed=602, T=1, n=2, h=45, w=61, short=96, divisor=64),
    'exact_2x': dict(seed=603, T=1, n=2, h=50, w=70, short=25, divisor=64),              # OpenCV's area path
    'reduce_over_2x': dict(seed=604, T=1, n=2, h=130, w=90, short=23, divisor=64),       # the direct regime
    'ratio_1': dict(seed=605, T=1, n=2, h=64, w=128, short=64, divisor=64),              # no resize, no padding
    'ratio_1_pad': dict(seed=606, T=1, n=2, h=48, w=80, short=48, divisor=64),           # padding only
    'ragged': dict(seed=607, T=1, n=2, h=97, w=139, short=75, divisor=16),               # ragged tiles in both axes
    'clip': dict(seed=608, T=3, n=2, h=40, w=56, short=30, divisor=64),                  # T = 3, two instances per frame
}
FP32_CASE = 'reduce_over_2x'           # the case whose normalised fp32 frames are stored too
PREDICT_CASES = ('reduce_under_2x', 'ratio_1_pad')


def pack_rows(a):
    """uint8 (..., H, W[, 3]) -> the differences between horizontal neighbours modulo 256 (the first column as it is): how the fixture stores its
    smooth images, which compress several times better that way. `unpack_rows` is the inverse."""
    a = np.asarray(a)
    assert a.dtype == np.uint8
    axis = a.ndim - (2 if a.shape[-1] == 3 and a.ndim >= 4 else 1)
    return np.diff(a, axis=axis, prepend=np.zeros_like(a.take([0], axis=axis)))


def unpack_rows(d):
    d = np.asarray(d)
    axis = d.ndim - (2 if d.shape[-1] == 3 and d.ndim >= 4 else 1)
    return np.cumsum(d, axis=axis, dtype=np.uint8)


def golden_inputs(name):
    """frames (T, h, w, 3), alphas (T * n, h, w), masks (T * n, h, w) of a case."""
    c = GOLDEN[name]
    frames = frames_of(c['seed'], c['T'], c['h'], c['w'])
    alphas = alphas_of(c['seed'] + 50, c['T'] * c['n'], c['h'], c['w'])
    return frames, alphas, masks_of(c['seed'] + 100, alphas)
