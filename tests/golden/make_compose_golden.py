"""Writes tests/golden/compose_pinned.npz with the real Pillow (run from the repository root: python tests/golden/make_compose_golden.py).

What is pinned to what: every array here is the output of PIL.Image calls -- `resize`, `crop`, `paste`, `Image.new` -- on the inputs that
tests/compose_restatement.py makes from seeds. The image runs do what tools/synthesize_image_him.py:33-111 does and the video frames what
tools/synthesize_video_him.py:136-184 does, written from their behaviour, with a NumPy min / max box where the tools call cv2.boundingRect. The tools' own scripts
were NOT run: they import cv2, which is not installed where this was written.

The generator asserts three conditions on its inputs before it writes anything (conditions on the inputs, not measurements of the code):
  1. an edge image clamps at 0 and at 255 in both passes, and omitting the byte clamp between the passes changes its result;
  2. every area ratio compared with 0.7, 0.3, 0.85, 0.05 or 0.5 lies at least 1e-3 from its threshold, so that the device's fp64 sums (about 1e-6
     relative from NumPy's fp32 pairwise sums) cannot flip a decision;
  3. among the image runs one rejects a first draw and accepts a later one, one fails all three draws and drops the instance, one has a
     resized foreground wider than the background (no draw consumed), and one returns None."""
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import compose_restatement as R  # noqa: E402

PIL_FILTER = {'bicubic': Image.BICUBIC, 'bilinear': Image.BILINEAR}
MARGIN = 1e-3


def box_of(alpha):
    ys, xs = np.nonzero(alpha > 0)
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def pil_cut(array, box, size, flt):
    """Pillow's crop of `array` to box = (x, y, w, h) and resize to `size`, as an Image."""
    x, y, w, h = box
    return Image.fromarray(array).crop((x, y, x + w, y + h)).resize(size, flt)


def pil_layer(hw, alpha_image, corner, dtype):
    """Pillow's paste of an alpha on a black 'L' image of (h, w), over 255 in float64, stored as `dtype`."""
    sheet = Image.new('L', (hw[1], hw[0]), 0)
    sheet.paste(alpha_image, corner)
    return (np.array(sheet) / 255.0).astype(dtype)


def pil_image_run(sample_id, fgs, alphas, bg):
    """The image tool's flow (synthesize_image_him.py:33-111) with every pixel made by PIL.Image -- crop, resize (bicubic, the tool's
    default), masked paste into the composite, plain paste on black -- and the bookkeeping of the restatement (the areas are NumPy sums in
    both). Returns (result or None, history, ratios, the next draw of the state)."""
    rs = np.random.RandomState(sample_id)
    composite = Image.fromarray(bg)
    W, H = composite.size
    boxes = [box_of(a) for a in alphas]
    scales = [rs.uniform(0.5, 0.9) * H / box[3] for box in boxes]
    cut = [tuple(pil_cut(v, box, (int(box[2] * s), int(box[3] * s)), Image.BICUBIC) for v in (f, a))
           for f, a, box, s in zip(fgs, alphas, boxes, scales)]
    stack = np.zeros((len(cut), H, W), np.float32)
    alone, history, ratios = [None] * len(cut), [], []
    for i, (fg, al) in enumerate(cut):
        tries = []
        while len(tries) < 3:
            corner = R.draw_corner(rs, W - al.width, H - al.height)
            if corner is None:
                break
            layer = pil_layer((H, W), al, corner, np.float32)
            kept, seen = R.kept_fractions(stack[:i], layer)
            ratios.extend(float(k) for k in kept[seen])
            accepted = not (kept[seen] < R.KEEP_AT_LEAST).any()
            tries.append(corner + (accepted,))
            if accepted:
                stack[:i], stack[i] = R.occlude(stack[:i], layer), layer
                composite.paste(fg, corner, al)
                alone[i] = Image.new('RGB', (W, H))
                alone[i].paste(fg, corner)
                break
        history.append(tries)
    nxt = int(rs.randint(0, 2 ** 31 - 1))
    live = [j for j in range(len(cut)) if (stack[j] != 0).any()]
    if not live:
        return None, history, ratios, nxt
    return {'image': np.array(composite), 'alphas': (stack[live] * 255).astype(np.uint8),
            'fgs': np.stack([np.array(alone[j]) for j in live])}, history, ratios, nxt


def pil_video_frame(bg, fgrs, alphas, plan, level):
    """One frame of the video tool (synthesize_video_him.py:136-184) with every pixel made by PIL.Image (crop, bilinear resize, masked paste,
    the alpha on a black 'L' image): (frame, fp64 planes, hidden fractions, the largest, abort)."""
    H, W = bg.shape[:2]
    frame = Image.fromarray(bg)
    stack, hidden, most = np.zeros((len(plan['placed']), H, W), np.float64), [], 0.0
    for i, (box, (left, top, nw, nh)) in enumerate(zip(plan['boxes'], plan['placed'])):
        al = pil_cut(alphas[i], box, (nw, nh), Image.BILINEAR)
        frame.paste(pil_cut(fgrs[i], box, (nw, nh), Image.BILINEAR), (left, top), al)
        layer = pil_layer((H, W), al, (left, top), np.float64)
        under = R.occlude(stack[:i], layer)
        for before, after in zip(stack[:i], under):
            if before.sum() > 0:
                hidden.append(float(1.0 - after.sum() / (before.sum() + 1e-7)))
                if R.HIDDEN_AT_MOST[level] is not None and hidden[-1] > R.HIDDEN_AT_MOST[level]:
                    return None, None, hidden, most, True
                most = max(most, hidden[-1])
        stack[:i], stack[i] = under, layer
    return np.array(frame), stack, hidden, float(most), False


def history_array(history):
    """(instance, x, y, accepted) rows; an instance without a try has the row (instance, -1, -1, 0)."""
    rows = []
    for i, tries in enumerate(history):
        rows.extend((i, x, y, int(ok)) for x, y, ok in tries)
        if not tries:
            rows.append((i, -1, -1, 0))
    return np.array(rows, np.int32).reshape(-1, 4)


def far(values, thresholds):
    return all(abs(v - t) >= MARGIN for v in values for t in thresholds)


def find_seed(name, want):
    fgs, alphas, bg = R.image_inputs(name)
    for seed in range(2000):
        res, history, ratios, nxt = pil_image_run(seed, fgs, alphas, bg)
        if want(res, history) and far(ratios, (0.7,)):
            return seed, res, history, nxt
    raise AssertionError('no seed gives the wanted history for %r' % name)


def main():
    out = {}
    clamps = False
    resized = {(ch, name): [] for ch in (1, 3) for name in R.FILTERS}
    for i, ((h, w), (oh, ow), crop) in enumerate(R.RESIZE_CASES):
        for ch in (1, 3):
            src = R.resize_input(i, ch)
            for name in R.FILTERS:
                im = Image.fromarray(src)
                if crop is not None:
                    im = im.crop(crop)
                got = np.array(im.resize((ow, oh), PIL_FILTER[name]))
                assert (got == R.resize(src, (ow, oh), name, crop)).all(), (i, ch, name)
                resized[ch, name].append(got)
                if name == 'bicubic' and crop is None and h != oh and w != ow:
                    x = src[..., None] if ch == 1 else src
                    raw_h = R._pass(x, R.coeffs(w, ow, name), 1, clamp=False)
                    raw_v = R._pass(np.clip(raw_h, 0, 255), R.coeffs(h, oh, name), 0, clamp=False)
                    both = raw_h.min() < 0 and raw_h.max() > 255 and raw_v.min() < 0 and raw_v.max() > 255
                    clamps = clamps or (both and (R.resize(src, (ow, oh), name, clamp_between=False) != got).any())
    for (ch, name), arrays in resized.items():
        out['resize/%d/%s' % (ch, name)] = R.resize_pack(arrays)
    assert clamps, 'condition 1: no edge image clamps at 0 and 255 in both passes with a result that needs the intermediate clamp'

    for ch in (1, 3):
        dst, src, mask = R.paste_input(ch)
        pasted = []
        for xy, _ in R.PASTE_CASES:
            for masked in (0, 1):
                im = Image.fromarray(dst.copy())
                im.paste(Image.fromarray(src), xy, Image.fromarray(mask) if masked else None)
                assert (np.array(im) == R.paste(dst, src, xy, mask if masked else None)).all()
                pasted.append(np.array(im))
        out['paste/%d' % ch] = np.stack(pasted).reshape((len(R.PASTE_CASES), 2) + dst.shape)

    def rejected_then_accepted(res, history):
        return res is not None and any(len(t) >= 2 and not t[0][2] and t[-1][2] for t in history)

    def dropped(res, history):
        return res is not None and any(len(t) == 3 and not any(ok for _, _, ok in t) for t in history)

    def no_range(res, history):
        return res is not None and history[1] == [] and len(history[2]) >= 1

    def nothing(res, history):
        return res is None and all(t == [] for t in history)

    runs = [('tall', lambda res, history: res is not None and all(len(t) == 1 for t in history)), ('crowd', rejected_then_accepted),
            ('crowd', dropped), ('wide', no_range), ('all_wide', nothing)]
    for k, (name, want) in enumerate(runs):
        seed, res, history, nxt = find_seed(name, want)
        out['image/%d/seed' % k] = np.array(seed)
        out['image/%d/name' % k] = np.array(name)
        out['image/%d/history' % k] = history_array(history)
        out['image/%d/next' % k] = np.array(nxt)
        out['image/%d/none' % k] = np.array(res is None)
        if res is not None:
            for key, v in res.items():
                out['image/%d/%s' % (k, key)] = v
        print('image run', k, name, 'seed', seed, 'history', history)

    for level in R.VIDEO_LEVELS:
        fgrs, alphas, bg, boxes = R.video_inputs(level)
        for seed in range(2000):                                            # the first seed whose frame is kept, overlaps, and is far from a threshold
            rs = np.random.RandomState(seed)
            plan = R.plan_video(rs, level, bg.shape[:2], boxes, n_bg_frames=7)
            if min(p[2] for p in plan['placed']) < 1 or min(p[3] for p in plan['placed']) < 1:
                continue
            frame, planes, occ, most, abort = pil_video_frame(bg, fgrs, alphas, plan, level)
            if not abort and most > 0.06 and far(occ, (0.3, 0.85, 0.05, 0.5)) and far([most], (0.05, 0.5)):
                break
        else:
            raise AssertionError('no seed gives a kept frame for %r' % level)
        out['video/%s/seed' % level] = np.array(seed)
        out['video/%s/placed' % level] = np.array(plan['placed'], np.int32)
        out['video/%s/start' % level] = np.array(plan['start_bg_frame'])
        out['video/%s/next' % level] = np.array(int(rs.randint(0, 2 ** 31 - 1)))
        out['video/%s/frame' % level] = frame
        out['video/%s/planes' % level] = (planes * 255).astype(np.uint8)
        out['video/%s/planes_f64' % level] = planes[:, ::7, ::5].copy()       # a sparse sample of the fp64 planes, bit for bit
        out['video/%s/max_occluded' % level] = np.array(most)
        print('video', level, 'placed', plan['placed'], 'occluded', occ)

    path = os.path.join(HERE, 'compose_pinned.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    assert os.path.getsize(path) < 100 * 1024


if __name__ == '__main__':
    main()
