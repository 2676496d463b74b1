"""NumPy restatement of the loaders' training crop (maggie/dataloader/transforms.py:191-305: RandomCropByAlpha, RandomHorizontalFlip), for the
tests only -- the product never imports it.

It builds on tests/geometry_restatement.py (its `copyMakeBorder` and `resize`: the unpinned restatement of OpenCV's documented behaviour) and
states the two classes twice:
  * `crop_flip`     the reference's code path line by line on a `np.random.RandomState` -- box, branch draw, up to three windows, the pad and
                    cv2.resize with `crop_size` in the `dsize` position, the flip draw; tests/golden/make_crop_golden.py runs the reference's own
                    classes beside it, which pins the draw order and the glue (tests/golden/crop_pinned.npz);
  * `bbox`, `first_hit`, `gather`, `padresize`   the same from a table of draws: what the device computes.
The seeded inputs of the fixture are regenerated here: it stores outputs only."""
import hashlib

import numpy as np

import geometry_restatement as R


# ---- the reference's code path -----------------------------------------------------------------------------------------------------------------
def crop_flip(frames, alphas, masks, crop_size, random, padding_prob, flip_p):
    """frames (T, H, W, 3), alphas (P, H, W), masks (P, H, W) or None, all uint8 -> a dict: the three outputs, `branch` ('crop' | 'pad'), the
    chosen `window` (x, y) and how many randint `pairs` were consumed (crop branch), `flip`, and the `box` the reference computed."""
    h, w = frames[0].shape[:2]
    if h < crop_size[0] or w < crop_size[1]:
        raise ValueError('Crop size {} is larger than image size {}'.format(crop_size, (h, w)))
    ys, xs = np.where(alphas.mean(0) > 127)
    if len(xs):
        min_x, max_x, min_y, max_y = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
    else:                                                                     # the reference's `except`: W and H, not W - 1 and H - 1
        min_x, max_x, min_y, max_y = 0, w, 0, h
    out = {'box': (min_x, max_x, min_y, max_y), 'window': None, 'pairs': 0}
    if random.rand() > padding_prob:
        out['branch'] = 'crop'
        hi_x = max(max_x - crop_size[1], min_x + 1)
        hi_y = max(max_y - crop_size[0], min_y + 1)
        for _ in range(3):
            x, y = random.randint(min_x, hi_x), random.randint(min_y, hi_y)
            x = min(x, w - crop_size[1])
            y = min(y, h - crop_size[0])
            out['pairs'] += 1
            if (alphas[:, y:y + crop_size[0], x:x + crop_size[1]] > 127).sum() > 0:
                break
        out['window'] = (int(x), int(y))
        f, a = frames[:, y:y + crop_size[0], x:x + crop_size[1], :], alphas[:, y:y + crop_size[0], x:x + crop_size[1]]
        m = None if masks is None else masks[:, y:y + crop_size[0], x:x + crop_size[1]]
    else:
        out['branch'] = 'pad'
        pad_w, pad_h = ((h - w) // 2, 0) if h > w else (0, (w - h) // 2)

        def go(xs_, interpolation):
            padded = [R.copyMakeBorder(x_, pad_h, pad_h, pad_w, pad_w, R.BORDER_CONSTANT, value=0) for x_ in xs_]
            return np.stack([R.resize(x_, tuple(crop_size), interpolation=interpolation) for x_ in padded])       # dsize = crop_size: (ch, cw) read as (w, h)
        f, a = go(frames, R.INTER_LINEAR), go(alphas, R.INTER_LINEAR)
        m = None if masks is None else go(masks, R.INTER_NEAREST)
    out['flip'] = bool(random.rand() < flip_p)
    if out['flip']:
        f, a = f[:, :, ::-1, :], a[:, :, ::-1]
        m = None if m is None else m[:, :, ::-1]
    out['frames'], out['alphas'] = np.ascontiguousarray(f), np.ascontiguousarray(a)
    out['masks'] = None if m is None else np.ascontiguousarray(m)
    return out


# ---- the same from a table of draws (what the device computes) -----------------------------------------------------------------------------------
def bbox(alphas):
    """(count, xmin, xmax, ymin, ymax) of sum_p alpha > 127 * P; (0, W, -1, H, -1) when empty -- mg_crop_bbox's contract."""
    P, H, W = alphas.shape
    ys, xs = np.where(alphas.astype(np.int64).sum(0) > 127 * P)
    if not len(xs):
        return (0, W, -1, H, -1)
    return (len(xs), int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))


def hits(alphas, windows, crop_size):
    ch, cw = crop_size
    return [int((alphas[:, y:y + ch, x:x + cw] > 127).any()) for x, y in windows]


def first_hit(alphas, windows, crop_size):
    h = hits(alphas, windows, crop_size)
    return h.index(1) if 1 in h else None


def gather(x, window, crop_size, flip):
    """x (N, H, W[, 3]) -> the (ch, cw) window at (x0, y0), columns reversed when `flip`."""
    (x0, y0), (ch, cw) = window, crop_size
    out = x[:, y0:y0 + ch, x0:x0 + cw]
    return np.ascontiguousarray(out[:, :, ::-1] if flip else out)


def padresize(x, crop_size, flip, interpolation):
    """The padding branch on (N, H, W[, 3]): zero border to the long side, cv2.resize to dsize = crop_size, then the flip."""
    H, W = x.shape[1:3]
    pad_w, pad_h = ((H - W) // 2, 0) if H > W else (0, (W - H) // 2)
    out = np.stack([R.resize(R.copyMakeBorder(p, pad_h, pad_h, pad_w, pad_w, R.BORDER_CONSTANT, value=0), tuple(crop_size), interpolation=interpolation)
                    for p in x])
    return np.ascontiguousarray(out[:, :, ::-1] if flip else out)


def state_digest(random):
    """A digest of a RandomState's full state: what the fixture stores of the generator after the two transforms."""
    name, keys, pos, has_gauss, cached = random.get_state()
    h = hashlib.sha256()
    h.update(name.encode())
    h.update(np.asarray(keys, np.uint32).tobytes())
    h.update(np.asarray([pos, has_gauss], np.int64).tobytes())
    h.update(np.float64(cached).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ---- seeded inputs (regenerated, never stored) ---------------------------------------------------------------------------------------------------
def blob(h, w, cy, cx, ry, rx, peak=255):
    """A soft ellipse: `peak` inside, a linear fringe a few pixels wide, 0 outside."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = (1.0 - np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)) * min(ry, rx)
    return np.clip(np.rint((0.5 + d / 4.0) * peak), 0, peak).astype(np.uint8)


def _alphas(c):
    h, w, P = c['h'], c['w'], c['T'] * c['n']
    kind = c['alphas']
    a = np.zeros((P, h, w), np.uint8)
    if kind == 'centre':                                                       # one blob per plane around the centre, shifted per plane
        for p in range(P):
            a[p] = blob(h, w, h * 0.5 + 3 * p, w * 0.5 - 4 * p, h * 0.22, w * 0.16)
    elif kind == 'corners':                                                    # two blobs in opposite corners, every plane
        for p in range(P):
            a[p] = np.maximum(blob(h, w, 9 + p, 12, 8, 11), blob(h, w, h - 10 - p, w - 14, 8, 12))
    elif kind == 'corner_pixels':                                              # one pixel in each of two opposite corners: three windows miss
        a[:, 0, 0] = 255
        a[:, h - 1, w - 1] = 255
        a[:, h // 2 - 6:h // 2 + 6, w // 2 - 9:w // 2 + 9] = 120              # a visible patch at or below 127: not in the box, no hit
    elif kind == 'empty':                                                      # soft shapes that never exceed 127
        for p in range(P):
            a[p] = blob(h, w, h * 0.4 + 5 * p, w * 0.55, h * 0.3, w * 0.2, peak=127)
    elif kind == 'mean_vs_any':                                                # corner blobs in every plane; one pixel at 255 in ONE plane
        for p in range(P):
            a[p] = np.maximum(blob(h, w, 10, 14 + p, 8, 11), blob(h, w, 40, w - 16 - p, 9, 12))
        a[3, c['lone'][0], c['lone'][1]] = 255
    elif kind == 'right_edge':                                                 # a blob whose box starts right of W - cw: the window is clamped
        for p in range(P):
            a[p] = blob(h, w, h * 0.5 - 2 * p, w - 22, h * 0.25, 14)
    else:
        raise KeyError(kind)
    return a


# the cases of tests/golden/crop_pinned.npz. padding_prob 0 / 1 and flip_p 0 / 1 fix the branch and the flip whatever rand() returns (it is drawn
# all the same); 'second_hit' and 'mean_vs_any' depend on their windows, so their `rs_seed` was searched for and the generator asserts the outcome
GOLDEN = {
    'first_hit': dict(seed=701, rs_seed=11, T=1, n=2, h=96, w=160, crop=(64, 64), pp=0.0, fp=1.0, alphas='centre'),
    'second_hit': dict(seed=702, rs_seed=5, T=1, n=1, h=96, w=160, crop=(64, 64), pp=0.0, fp=0.0, alphas='corners'),
    'three_misses': dict(seed=703, rs_seed=13, T=1, n=2, h=96, w=160, crop=(64, 64), pp=0.0, fp=1.0, alphas='corner_pixels'),
    'empty': dict(seed=704, rs_seed=14, T=1, n=2, h=96, w=160, crop=(48, 80), pp=0.0, fp=0.0, alphas='empty'),
    'mean_vs_any': dict(seed=705, rs_seed=0, T=3, n=2, h=96, w=160, crop=(64, 32), pp=0.0, fp=1.0, alphas='mean_vs_any', lone=(60, 70)),
    'full_size': dict(seed=706, rs_seed=16, T=1, n=2, h=96, w=160, crop=(96, 160), pp=0.0, fp=0.0, alphas='centre'),
    'clamped': dict(seed=707, rs_seed=6, T=1, n=2, h=99, w=157, crop=(64, 64), pp=0.5, fp=0.5, alphas='right_edge'),
    'pad_tall': dict(seed=708, rs_seed=18, T=1, n=2, h=96, w=70, crop=(64, 64), pp=1.0, fp=0.0, alphas='centre'),
    'pad_wide_odd': dict(seed=709, rs_seed=19, T=1, n=2, h=96, w=157, crop=(48, 80), pp=1.0, fp=1.0, alphas='centre'),
}


def golden_inputs(name):
    """frames (T, h, w, 3), alphas (T * n, h, w), masks (T * n, h, w) of a case; the masks are the binarised alphas with 3 % of the pixels
    flipped, so they differ from the alphas."""
    c = GOLDEN[name]
    alphas = _alphas(c)
    return R.frames_of(c['seed'], c['T'], c['h'], c['w']), alphas, R.masks_of(c['seed'] + 100, alphas)


def golden_run(name):
    """`crop_flip` on a case with its own seeded generator: (result dict, the generator afterwards)."""
    c = GOLDEN[name]
    frames, alphas, masks = golden_inputs(name)
    rs = np.random.RandomState(c['rs_seed'])
    return crop_flip(frames, alphas, masks, c['crop'], rs, c['pp'], c['fp']), rs
