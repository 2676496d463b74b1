"""Device time of the guidance-mask chain (maggie_amd.utils.maskgen, csrc/maskgen.hip) for one training item of each kind: 8 instance planes of
512 x 512 (image: binarise + morphology, down / up, cut) and 24 planes (video, T = 8 x 3 instances: the same plus the drop-out with its one
read-back), warm, device-resident draws, every call bracketed by its own event pair. Beside it the parent's nearest equivalent as a sanity
bound: the grey-scale ellipse pass `groundtruth.dilate_erode` at k = 29 on the same planes, alternated with the chain in the same loop.
The worst draw of the morphology stage (k = 29 twice on every plane) is timed on its own.
usage: python tools/maskgen_bench.py [reps]"""
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import groundtruth as G
from maggie_amd.utils import maskgen as MG

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def soft(rs, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    ry, rx = rs.uniform(H / 10, H / 4), rs.uniform(W / 12, W / 5)
    cy, cx = rs.uniform(0.2 * H, 0.8 * H), rs.uniform(0.2 * W, 0.8 * W)
    d = (1.0 - np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)) * min(ry, rx)
    return np.clip(np.rint((0.5 + d / 6.0) * 255), 0, 255).astype(np.uint8)


def main():
    rs = np.random.RandomState(0)
    H = W = 512
    rows = []
    for kind, P in (('image', 8), ('video', 24)):
        planes = torch.from_numpy(np.stack([soft(rs, H, W) for _ in range(P)])).to(dev)
        noise = torch.from_numpy(rs.randint(0, 256, size=(P, H, W)).astype(np.uint8)).to(dev)
        draws = MG.draw_chain(np.random.RandomState(1), random.Random(1), P, H, W, from_alpha=kind == 'video').to(dev)
        worst = MG.morph_table(127.0, 29, 29, 'dilate_erode', P)
        worst_dev = torch.from_numpy(worst).to(dev)
        ones = torch.ones((P,), dtype=torch.int32, device=dev)
        cut = draws.cut
        kn = G.draws(29, 1, P)
        st = MG.stats(planes)
        for seed in range(64):                                            # the first seed whose draw takes the branch and zeroes something
            sel = MG.draw_dropout(np.random.RandomState(seed), st.cpu().numpy())
            if (sel[:, 0] >= 0).any():
                break
        sel = torch.from_numpy(sel).to(dev)
        names = ['%s chain, %d x 512^2 (3 launches, drawn parameters)' % (kind, P), '  morphology alone, worst draw (k = 29 dilate + erode, every plane)',
                 '  the same on uniform noise', '  down / up alone, every plane', '  cut alone', '  statistics alone (drop-out, first phase)',
                 '  drop alone (second phase, %d entries; with its copy of the planes)' % int((sel[:, 0] >= 0).sum()),
                 'parent: groundtruth.dilate_erode k = 29 (grey-scale ellipse), same planes', '  the same on uniform noise']
        fns = [lambda: MG.synthesize(planes, draws), lambda: MG.binarize_morph(planes, worst_dev), lambda: MG.binarize_morph(noise, worst_dev),
               lambda: MG.down_up(planes, ones), lambda: MG.cut(planes, cut), lambda: MG.stats(planes), lambda: MG.drop(planes, sel, st),
               lambda: G.dilate_erode(planes, kn), lambda: G.dilate_erode(noise, kn)]
        rows += list(zip(names, [t[:2] for t in timed(fns, REPS)]))
        if kind == 'video':                                               # with the drop-out: a host synchronisation inside, so a host clock
            dd = MG.draw_chain(np.random.RandomState(1), random.Random(1), P, H, W, dropout=True, from_alpha=True).to(dev)
            dr = np.random.RandomState(2)
            for _ in range(10):
                MG.synthesize(planes, dd, dr)
            torch.cuda.synchronize()
            ts = []
            for _ in range(REPS):
                t = time.perf_counter()
                MG.synthesize(planes, dd, dr)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t) * 1e6)
            rows.append(('video chain with the drop-out (read-back inside; host clock, synchronised)', (float(np.median(ts)), float(np.min(ts)))))
    print('%-82s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us'))
    for name, (med, mn) in rows:
        print('%-82s %10.1f %10.1f' % (name, med, mn))


if __name__ == '__main__':
    main()
