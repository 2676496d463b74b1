"""Device time of MESSDdt (maggie_amd.utils.metric.MESSDdt, csrc/flow.hip) at a video-evaluation shape: a window of F = 3 frames of 3
instances at 720 x 1280, warm, every call bracketed by its own event pair, the candidates alternated call by call:
  * `MESSDdt.update` as evaluation calls it (scratch allocation, 6 x 6 + 4 launches, one read of 6 doubles);
  * the flow alone (`flow.farneback` of the 6 plane pairs) and the reduction alone (the flow handed in);
  * the split over the kernels of one `update`, from the profiler's kernel records (sums over the pyramid's levels).
The reference's path (cv2 in a process pool, torch on the CPU) cannot run in this build, so there is no ratio to report.
usage: python tools/flow_bench.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import flow
from maggie_amd.utils import metric as dm

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 20
F, N, H, W = 3, 3, 720, 1280


def main():
    import flow_restatement as R                                   # the seeded moving pattern of the tests
    rng = np.random.default_rng(0)
    gt = np.empty((F, N, H, W), np.float32)
    for n in range(N):
        gt[:, n] = np.stack(R.frames(H, W, [((2.3 + n) * t, (-1.2 + 0.5 * n) * t) for t in range(F)], n)).astype(np.float32) / np.float32(255)
    pred = np.clip(gt + rng.normal(0, 0.05, gt.shape), 0, 1).astype(np.float32)
    pred, gt = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    tri = torch.from_numpy(rng.integers(0, 3, (F, N, H, W)).astype(np.float32)).to(dev)
    u8 = (gt * 255.0).to(torch.uint8)
    m = dm.MESSDdt()
    m.update(pred, gt, tri, keep_flow=True)
    given = m.last_flow
    print('score of the window %.4f; levels %d; scratch %.1f MiB' % (m.score, flow.levels_of(H, W), flow.messddt_scratch(F, N, H, W, dev).numel() / 2 ** 20))
    names = ['MESSDdt.update (F %d, N_i %d, %d x %d)' % (F, N, H, W), '  flow alone (farneback, %d pairs)' % ((F - 1) * N),
             '  reduction alone (flow handed in)']
    fns = [lambda: m.update(pred, gt, tri), lambda: flow.farneback(u8[:-1], u8[1:]), lambda: m.update(pred, gt, tri, flow=given)]
    print('%-60s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in zip(names, timed(fns, REPS, warmup=3)):
        print('%-60s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        m.update(pred, gt, tri)
        torch.cuda.synchronize()
    rows = [(e.key, e.count, e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total) for e in prof.key_averages()]
    rows = sorted([r for r in rows if r[2] > 0], key=lambda r: -r[2])
    total = sum(r[2] for r in rows) or 1.0
    print('%-60s %6s %10s %6s' % ('kernels of one update', 'calls', 'us', '%'))
    for key, count, us in rows:
        print('%-60s %6d %10.1f %6.1f' % (key[:60], count, us, 100.0 * us / total))


if __name__ == '__main__':
    main()
