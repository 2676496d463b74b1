"""Device time of one `compose.synthesize_image` at the image tool's real scale (maggie_amd.utils.compose, csrc/compose.hip): a 1920 x 1080
background and three instances cropped from 1024-high foregrounds. Warm, every call bracketed by its own event pair, the candidates alternated
call by call (tools/_timing.py): the launches one at a time on the first instance's geometry, then the whole item (its host control and its
read-backs lie between the events too). With `--pillow` the same item is timed with PIL.Image calls on ONE core of the host instead (the
generator's `pil_image_run`, tests/golden/make_compose_golden.py); no GPU is needed for that.
usage: python tools/compose_bench.py [reps] | python tools/compose_bench.py --pillow [reps]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np

import compose_restatement as R

BG_HW, FG_HW = (1080, 1920), (1024, 768)
BOXES = [(100, 40, 520, 960), (60, 20, 600, 990), (150, 60, 480, 900)]
SEED = 0


def inputs():
    srcs = [R.person(FG_HW[0], FG_HW[1], box, k) for k, box in enumerate(BOXES)]
    return [f for f, _ in srcs], [a for _, a in srcs], R.background(0, BG_HW)


def pillow(reps):
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_compose_golden as G
    fgs, alphas, bg = inputs()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        res, history, _, _ = G.pil_image_run(SEED, fgs, alphas, bg)
        ts.append(time.perf_counter() - t0)
    print('Pillow, one core of %d: median %.1f ms, min %.1f ms over %d runs; history %s' % (os.cpu_count(), np.median(ts) * 1e3, min(ts) * 1e3,
                                                                                           reps, history))


def device(reps):
    import torch

    from _timing import timed
    from maggie_amd.utils import compose
    dev = torch.device('cuda:0')
    fgs, alphas, bg = inputs()
    fgs, alphas, bg = [torch.from_numpy(f).to(dev) for f in fgs], [torch.from_numpy(a).to(dev) for a in alphas], torch.from_numpy(bg).to(dev)
    x, y, w, h = BOXES[0]
    scale = 0.7 * BG_HW[0] / h
    size, crop = (int(w * scale), int(h * scale)), (x, y, x + w, y + h)
    tables = compose.ResizeTables((w, h), size).to(dev)
    f, a = compose.pil_resize(fgs[0], size, crop=crop, tables=tables), compose.pil_resize(alphas[0], size, crop=crop, tables=tables)
    image, canvas = bg.clone(), torch.zeros_like(bg)
    planes = torch.rand((3,) + BG_HW, device=dev)
    fns = [
        ('alpha_box (16-byte read-back)', lambda: compose.alpha_box(alphas[0])),
        ('pil_resize RGB fused %dx%d -> %dx%d' % (w, h, size[0], size[1]), lambda: compose.pil_resize(fgs[0], size, crop=crop, tables=tables)),
        ('pil_resize RGB two_pass', lambda: compose.pil_resize(fgs[0], size, crop=crop, tables=tables, regime='two_pass')),
        ('pil_resize L fused', lambda: compose.pil_resize(alphas[0], size, crop=crop, tables=tables)),
        ('pil_resize L two_pass', lambda: compose.pil_resize(alphas[0], size, crop=crop, tables=tables, regime='two_pass')),
        ('try_place n_prev 2 (168-byte read-back)', lambda: compose.try_place(planes, a, (300, 200), 2)),
        ('commit idx 2', lambda: compose.commit(image, canvas, planes, f, a, (300, 200), 2)),
        ('paste RGB masked', lambda: compose.paste(image, f, (300, 200), a)),
        ('planes_u8 3 planes', lambda: compose.planes_u8(planes)),
        ('synthesize_image, the whole item', lambda: compose.synthesize_image(SEED, fgs, alphas, bg)),
    ]
    print('background %d x %d, foregrounds %d x %d, boxes %s; %d calls each' % (BG_HW[1], BG_HW[0], FG_HW[1], FG_HW[0], BOXES, reps))
    print('%-52s %10s %10s %10s %10s' % ('call', 'median us', 'min us', 'p25 us', 'p75 us'))
    for (name, _), (med, mn, lo, hi) in zip(fns, timed([fn for _, fn in fns], reps, warmup=3)):
        print('%-52s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    print('history', compose.synthesize_image(SEED, fgs, alphas, bg)['history'])


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if a != '--pillow']
    reps = int(args[0]) if args else 20
    pillow(reps) if '--pillow' in sys.argv else device(reps)
