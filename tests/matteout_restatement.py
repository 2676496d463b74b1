"""The reference predictor's pixel passes behind the forward, restated in NumPy for the tests of maggie_amd/utils/matteout.py (DESIGN.md section
29). Our own code; what each function restates is cited by file:line of the reference. Nothing here imports the package.
tests/test_matteout_cpu.py holds `overlay` against live `PIL.Image.blend` and asserts that `grid` tells the contracted forms apart.

  * `composite(image, alpha, bg)`   demo/maggie_predictor.py:73-74,156: `(image * a + (1 - a) * green_bg).astype(np.uint8)` with a uint8 image, a
                                    float32 alpha and a uint8 background: two float32 products and a float32 sum, each rounded on its own, then
                                    truncated. The sum is clamped to [0, 255] first: a no-op for alphas in [0, 1], our stated choice outside.
  * `wrong_forms`                   the four evaluations a kernel could slip into: two fused multiply-adds, the algebraic form, fp64.
  * `overlay(image, mask, colour, alpha)`   demo/app.py:59-65: `Image.blend(image, palette(mask > 0), alpha)`.
  * `label_planes(label_map)`       demo/maggie_predictor.py:35-40.
  * `snap(alpha)`                   demo/maggie_predictor.py:64-65,127-128.
  * `writer_loop(pushes)`           demo/maggie_predictor.py:132-167: which composites the video loop saves under which names, push by push.
  * `grid`, `backgrounds`           the discriminating test grid."""
import os

import numpy as np

GREEN = (0, 255, 0)


def background_of(bg, shape):
    """Three bytes or a uint8 image -> a uint8 image of `shape` (H, W, 3)."""
    if np.ndim(bg) == 1:
        out = np.zeros(shape, np.uint8)                             # maggie_predictor.py:69-70: zeros_like(image), then one channel set
        out[...] = np.asarray(bg, np.uint8)
        return out
    return np.broadcast_to(np.asarray(bg, np.uint8), shape)


def composite(image, alpha, bg=GREEN):
    """image (H, W, 3) uint8, alpha (H, W) float32, bg three bytes or (H, W, 3) uint8 -> (H, W, 3) uint8."""
    assert image.dtype == np.uint8 and alpha.dtype == np.float32
    a = alpha[:, :, None]
    s = image * a + (1 - a) * background_of(bg, image.shape)       # uint8 * float32 -> float32, as in the reference
    assert s.dtype == np.float32
    return np.clip(s, 0, 255).astype(np.uint8)


def composites(frames, alphas, bg=GREEN):
    """frames (T, H, W, 3), alphas (T, P, H, W), bg three bytes or an image (H, W, 3) / (1, H, W, 3) / (T, H, W, 3) -> (T, P, H, W, 3)."""
    T, P = alphas.shape[:2]
    out = np.zeros((T, P) + frames.shape[1:], np.uint8)
    for t in range(T):
        b = bg if np.ndim(bg) in (1, 3) else bg[t if len(bg) > 1 else 0]
        for p in range(P):
            out[t, p] = composite(frames[t], alphas[t, p], b)
    return out


def _fma(x, y, z):
    """fl32(x * y + z) with one rounding, for x a byte (or 1 - a) and y, z float32 of the grid's sizes: the product (at most 8 + 24 bits) and its
    sum with z (bits between 2^8 and about 2^-40) are exact in float64, so the one rounding to float32 is the fused operation's."""
    return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(np.float32)


def wrong_forms(image, alpha, bg=GREEN):
    """{name: bytes} of the four evaluations that are NOT the reference's: what a contracting compiler or a tidy-minded author would write."""
    a = alpha[:, :, None].astype(np.float32)
    v = image.astype(np.float32)
    b = background_of(bg, image.shape).astype(np.float32)
    one = np.float32(1)
    trunc = lambda s: np.clip(s, 0, 255).astype(np.uint8)
    a64, v64, b64 = a.astype(np.float64), v.astype(np.float64), b.astype(np.float64)
    return {
        'fma(v, a, t2)': trunc(_fma(v, a, (one - a) * b)),
        'fma(1 - a, bg, t1)': trunc(_fma(one - a, b, v * a)),
        'bg + a * (v - bg)': trunc(b + a * (v - b)),
        'fp64': trunc(v64 * a64 + (1.0 - a64) * b64),
    }


def overlay(image, mask, colour=(255, 0, 255), alpha=0.5):
    """image (H, W, 3) uint8, mask (H, W) uint8 -> Image.blend(image, palette(mask > 0), alpha): Pillow's Blend.c computes
    `(UINT8)((float)in1 + alpha * ((float)in2 - (float)in1))`; the difference of two bytes is exact either way."""
    in2 = np.where(mask[:, :, None] > 0, np.asarray(colour, np.uint8), np.uint8(0)).astype(np.int32)
    in1 = image.astype(np.int32)
    s = in1.astype(np.float32) + np.float32(alpha) * (in2 - in1).astype(np.float32)
    assert s.dtype == np.float32
    return np.clip(s, 0, 255).astype(np.uint8)


def pillow_overlay(image, mask, colour=(255, 0, 255), alpha=0.5):
    """app.py:59-65 with Pillow itself."""
    from PIL import Image
    m = Image.fromarray((mask > 0).astype(np.uint8))
    m.putpalette([0, 0, 0] + [int(c) for c in colour])
    return np.array(Image.blend(Image.fromarray(image), m.convert('RGB'), alpha=alpha))


def label_planes(label_map):
    """maggie_predictor.py:35-40 -> (ids, planes uint8 (n, H, W))."""
    ids = np.unique(label_map)
    ids = ids[ids != 0]
    planes = [((label_map == i) * 255).astype(np.uint8) for i in ids]
    return [int(i) for i in ids], (np.stack(planes) if planes else np.zeros((0,) + label_map.shape, np.uint8))


def snap(alpha):
    a = alpha.copy()
    a[a <= 1.0 / 255.0] = 0.0
    a[a >= 254.0 / 255.0] = 1.0
    return a


def writer_loop(pushes, out_dir, bg=GREEN):
    """maggie_predictor.py:132-167. pushes: [(alpha (3, n, H, W) float32 -- reverse-transformed, snapped and post-processed --, frames (3, H, W, 3)
    uint8, names [3 paths], is_first, is_last)] -> per push the list of (path, composite) the loop saves, in its order."""
    all_preds, all_names, images = [], [], {}
    written = []
    for alpha, frames, names, is_first, is_last in pushes:
        for n, f in zip(names, frames):
            images[n] = f                                                   # what Image.open(image_name) would read
        if is_first:
            all_preds, all_names = list(alpha), list(names)
        else:
            all_names = all_names + list(names[2:])
            all_preds = all_preds[:-1] + list(alpha[1:])
        end_idx = 1 if not is_last else len(all_preds)
        out = []
        for name, pred in zip(all_names[:end_idx], all_preds[:end_idx]):
            for i in range(len(pred)):
                suffix = os.path.basename(name).replace('.jpg', '')
                out.append((os.path.join(out_dir, '%02d_%s.jpg' % (i, suffix)), composite(images[name], pred[i], bg)))
        written.append(out)
        if len(all_preds) > 3:
            all_preds, all_names = all_preds[-3:], all_names[-3:]
    return written


# ---- the discriminating grid ---------------------------------------------------------------------------------------------------------------
GRID_ROWS, GRID_SEED = 512, 20
SPECIAL_ALPHAS = (0.0, 1.0, 1.0 / 255.0, 254.0 / 255.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))))
CONSTANT_BACKGROUNDS = ((0, 255, 0), (255, 255, 255), (17, 99, 203))


def grid(rows=GRID_ROWS, seed=GRID_SEED):
    """(image (R + 6, 256, 3) uint8, alpha (R + 6, 256) float32): every pixel value across -- the three channels hold v, 255 - v and (v * 7) % 256
    --, `rows` seeded float32 alphas of [0, 1) plus the special ones down."""
    rs = np.random.RandomState(seed)
    col = np.concatenate([rs.random_sample(rows).astype(np.float32), np.array(SPECIAL_ALPHAS, np.float32)])
    v = np.arange(256)
    image = np.broadcast_to(np.stack([v, 255 - v, (v * 7) % 256], -1).astype(np.uint8), (len(col), 256, 3)).copy()
    alpha = np.broadcast_to(col[:, None], (len(col), 256)).copy()
    return image, alpha


def backgrounds(shape, seed=GRID_SEED + 1):
    """The four backgrounds of the grid tests: three colours and a seeded random image of `shape`."""
    return list(CONSTANT_BACKGROUNDS) + [np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)]
