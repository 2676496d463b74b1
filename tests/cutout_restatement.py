"""A NumPy statement of the device cut-outs (maggie_amd/csrc/cutout.hip): the byte-for-byte oracle of the kernels and of
`maggie_amd.utils.cutout`, and a sequential colour-PNG encoder that is tests/pngenc_restatement.py with another filtered stream.

The estimator is the blur-fusion foreground estimator (Forte & Pitie, ICIP 2021), twice, stated on bytes: window sums as int64 from a cumulative
sum over the reflected, padded plane (exact, so the order of adding cannot matter), then the formula in float64, one NumPy operation per stated
operation, in the stated order."""
import struct

import numpy as np

import pngenc_restatement as R

RADII = (90, 6)


# ---- the window --------------------------------------------------------------------------------------------------------------------------------
def reflect(i, n):
    """BORDER_REFLECT_101 as often as needed: index i (an int array) on an axis of length n -> 0..n-1; period 2 (n - 1), n = 1 maps all to 0."""
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m < n, m, p - m)


def window_sums(plane, r):
    """Integer plane (H, W) -> int64 (H, W): the sum over [y - r//2, y - r//2 + r) x [x - r//2, x - r//2 + r) of the reflected plane."""
    p = np.asarray(plane).astype(np.int64)
    H, W = p.shape
    ys, xs = reflect(np.arange(-(r // 2), H - (r // 2) + r - 1), H), reflect(np.arange(-(r // 2), W - (r // 2) + r - 1), W)
    pad = p[ys][:, xs]                                                      # (H + r - 1, W + r - 1)
    c = np.zeros((pad.shape[0] + 1, pad.shape[1] + 1), np.int64)
    c[1:, 1:] = pad.cumsum(0).cumsum(1)
    return c[r:, r:] - c[:-r, r:] - c[r:, :-r] + c[:-r, :-r]


# ---- one pass, the estimate, the cut-out ---------------------------------------------------------------------------------------------------------
def _byte(v):
    return np.floor(np.clip(v, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def one_pass(I, F, B, a, r):
    """P(I, F, B, a, r): I, F, B uint8 (H, W, 3), a uint8 (H, W) -> (F', B') uint8 (H, W, 3)."""
    n = float(r * r)
    a64 = a.astype(np.int64)
    SA = window_sums(a64, r)
    assert SA.max() < 2 ** 32
    ba = SA.astype(np.float64) / (255.0 * n)
    dF = ba + 1e-5
    dB = (1.0 - ba) + 1e-5
    al = a.astype(np.float64) / 255.0
    Fo, Bo = np.empty(I.shape, np.uint8), np.empty(I.shape, np.uint8)
    for c in range(3):
        SFA = window_sums(F[..., c].astype(np.int64) * a64, r)
        SBA = window_sums(B[..., c].astype(np.int64) * (255 - a64), r)
        assert max(SFA.max(), SBA.max()) < 2 ** 32
        bF = (SFA.astype(np.float64) / (65025.0 * n)) / dF
        bB = (SBA.astype(np.float64) / (65025.0 * n)) / dB
        i = I[..., c].astype(np.float64) / 255.0
        t1 = al * bF
        t2 = i - t1
        t3 = (1.0 - al) * bB
        t4 = t2 - t3
        t5 = al * t4
        f = bF + t5
        Fo[..., c], Bo[..., c] = _byte(f), _byte(bB)
    return Fo, Bo


def alpha_byte(a):
    """uint8 as it is; float32 by the rule of pngenc's 'unit' mode."""
    a = np.asarray(a)
    return a if a.dtype == np.uint8 else R.to_bytes(a.astype(np.float32), 'unit')


def estimate(I, a, radii=RADII):
    """I uint8 (H, W, 3), a (H, W) uint8 or float32 -> F uint8 (H, W, 3)."""
    a = alpha_byte(a)
    F1, B1 = one_pass(I, I, I, a, radii[0])
    return one_pass(I, F1, B1, a, radii[1])[0]


def estimate_all(frames, alpha, radii=RADII):
    """frames (T, H, W, 3), alpha (T, P, H, W) -> (T, P, H, W, 3)."""
    return np.stack([np.stack([estimate(frames[t], alpha[t, p], radii) for p in range(alpha.shape[1])]) for t in range(frames.shape[0])])


def cutout(I, a, radii=RADII):
    """-> straight RGBA uint8 (H, W, 4): the estimate, the alpha byte, RGB 0 where the alpha byte is 0."""
    a = alpha_byte(a)
    out = np.concatenate([estimate(I, a, radii), a[..., None]], axis=-1)
    out[a == 0, :3] = 0
    return out


def cutout_all(frames, alpha, radii=RADII):
    return np.stack([np.stack([cutout(frames[t], alpha[t, p], radii) for p in range(alpha.shape[1])]) for t in range(frames.shape[0])])


# ---- the synthetic scene of the property check -----------------------------------------------------------------------------------------------------
def scene(H=240, W=320, seed=0):
    """A soft disc, a textured foreground, a gradient background -> (I, true F, B, a): I = q(alpha F + (1 - alpha) B)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    d = np.hypot(yy - 0.5 * H, xx - 0.5 * W)
    alpha = np.clip((0.33 * H + 12.0 - d) / 24.0, 0.0, 1.0)
    a = np.floor(alpha * 255.0 + 0.5).astype(np.uint8)
    tex = 40.0 * np.sin(xx / 5.0) * np.cos(yy / 7.0) + rng.uniform(-10, 10, (H, W))
    F = np.clip(np.stack([200.0 + tex, 60.0 + 0.5 * tex, 40.0 - 0.5 * tex], -1), 0, 255)
    B = np.stack([20.0 + 60.0 * xx / W, 120.0 + 100.0 * yy / H, 150.0 + 100.0 * xx / W], -1)
    al = (a.astype(np.float64) / 255.0)[..., None]
    I = np.floor(al * F + (1.0 - al) * B + 0.5).astype(np.uint8)
    return I, np.floor(F + 0.5).astype(np.uint8), np.floor(B + 0.5).astype(np.uint8), a


# ---- colour PNG --------------------------------------------------------------------------------------------------------------------------------------
def filtered_colour(image):
    """uint8 (h, w, C) -> the Sub-filtered scanlines, uint8 (h * (1 + C w),): row r is 01, then byte j of the row minus byte j - C."""
    p = np.asarray(image, np.uint8)
    h, w, C = p.shape
    row = p.reshape(h, w * C)
    f = np.empty((h, 1 + w * C), np.uint8)
    f[:, 0] = 1
    f[:, 1:1 + C] = row[:, :C]
    f[:, 1 + C:] = row[:, C:] - row[:, :-C]
    return f.reshape(-1)


def png_file_colour(h, w, C, stream):
    """R.png_file with the colour type 2 (RGB) or 6 (RGBA)."""
    return R.SIGNATURE + R.chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, {3: 2, 4: 6}[C], 0, 0, 0)) + R.chunk(b'IDAT', stream) + R.chunk(b'IEND', b'')


def encode_colour(image, B=R.BLOCK):
    """uint8 (h, w, 3) or (h, w, 4) -> (the PNG file, [Block]): pngenc_restatement's encoder on the colour filtered stream."""
    p = np.asarray(image, np.uint8)
    stream, blocks = R.encode_stream(filtered_colour(p), B)
    return png_file_colour(p.shape[0], p.shape[1], p.shape[2], stream), blocks


def disc_image(h, w, C, seed=0):
    """A cut-out-like image: noise inside a disc, zeros outside."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    inside = (yy - h / 2.0) ** 2 / max(h / 2.5, 1) ** 2 + (xx - w / 2.0) ** 2 / max(w / 2.5, 1) ** 2 <= 1.0
    img = rng.randint(0, 256, (h, w, C)).astype(np.uint8)
    img[~inside] = 0
    return img
