"""Time of the device PNG encode (maggie_amd.utils.pngenc, csrc/pngenc.hip) on three workloads of seeded synthetic mattes -- soft-edged
ellipses, fp32 in [0, 1] on the device, as the evaluation leaves them: one 512 x 512 plane, one 1080 x 1920 plane, and the video
evaluation's window of 3 frames x 10 instances at 1080 x 1920. Warm, every call bracketed by its own event pair (the read-backs, the CRC and
the chunk framing lie between its events too), the candidates alternated call by call:
  * `pngenc.encode_planes(x, mode='unit')` from the device planes to complete files in host memory;
  * the parent's only path: `.cpu()` of the fp32 planes, `(a * 255).astype('uint8')`, and one Pillow `save(compress_level=1)` per plane.
    The reference calls cv2.imwrite there; cv2 is not installed where this was written, so the comparison is with Pillow.
Neither side writes to disk. The tool first asserts that Pillow reads back from the device's files what the host path encodes. Then the
device time per entry point, from `hip.enable_timing`.
usage: python tools/pngenc_bench.py [reps]"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import pngenc

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100


def matte(rs, h, w):
    """A few soft-edged ellipses: 1 inside, 0 outside, a ramp a few pixels wide between."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.zeros((h, w))
    for _ in range(3):
        cy, cx = rs.uniform(0.25, 0.75) * h, rs.uniform(0.25, 0.75) * w
        ry, rx = rs.uniform(0.1, 0.3) * h, rs.uniform(0.1, 0.3) * w
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        a = np.maximum(a, np.clip((1.0 - d) * min(ry, rx) / 4.0, 0.0, 1.0))
    return a.astype(np.float32)


def host_path(x):
    planes = (x.cpu().numpy() * 255).astype('uint8')
    out = []
    for p in planes:
        buf = io.BytesIO()
        Image.fromarray(p).save(buf, 'PNG', compress_level=1)
        out.append(buf.getvalue())
    return out


def main():
    rs = np.random.RandomState(0)
    work = [('one 512 x 512 plane', 1, 512, 512), ('one 1080 x 1920 plane', 1, 1080, 1920), ('3 frames x 10 instances, 1080 x 1920', 30, 1080, 1920)]
    rows, kept = [], []
    for name, P, h, w in work:
        x = torch.from_numpy(np.stack([matte(rs, h, w) for _ in range(P)])).to(dev)
        files = pngenc.encode_planes(x, mode='unit')
        want = (x.cpu().numpy() * 255).astype('uint8')
        for f, p in zip(files, want):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), p)      # the same pixels as the host path writes
        ref = host_path(x)
        fns = [lambda x=x: pngenc.encode_planes(x, mode='unit'), lambda x=x: host_path(x)]
        reps = max(REPS // (4 if P > 1 else 1), 5)
        names = ['%s: pngenc.encode_planes; %d KB of files (Pillow level 1: %d KB), %d blocks, 2 read-backs' %
                 (name, sum(len(f) for f in files) >> 10, sum(len(f) for f in ref) >> 10, P * pngenc.blocks_of(h, w)),
                 '  parent: .cpu(), (a * 255).astype(uint8), Pillow save(compress_level=1) per plane (%d calls)' % reps]
        rows += list(zip(names, timed(fns, reps)))
        kept.append((name, x))
    print('%-110s %10s %10s %10s %10s' % ('workload', 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-110s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    entries = ['mg_pngenc_size', 'mg_pngenc_emit']
    for name, x in kept:
        hip.enable_timing(entries)
        for _ in range(10):
            pngenc.encode_planes(x, mode='unit')
        torch.cuda.synchronize()
        rec = hip.disable_timing()['records']
        print('device time per entry point, %s (event pairs around the launches, median of 10 calls, us): ' % name +
              ', '.join('%s %.1f' % (e[3:], np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]])) for e in entries))


if __name__ == '__main__':
    main()
