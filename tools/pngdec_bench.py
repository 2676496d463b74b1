"""Time of the device PNG decode (maggie_amd.utils.pngdec, csrc/pngdec.hip) on three workloads of seeded synthetic mattes -- soft-edged
ellipses, mostly 0 and 255, saved by Pillow at its defaults: one 512 x 512 file, one 1080 x 1920 file and a clip of 8 x 3 files at 512 x 512.
Warm, every call bracketed by its own event pair (host work of a call -- the chunk walk, the upload, the read-back -- lies between its
events too), the candidates alternated call by call:
  * `pngdec.decode_planes` from the files' bytes;
  * the parent's only path: `Image.open(...).convert("L")` per file on the host plus the host -> device copy.
The tool first asserts that both give the same bytes. Then the device time per entry point, from `hip.enable_timing`.
usage: python tools/pngdec_bench.py [reps]"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import pngdec

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def matte(rs, h, w):
    """A few soft-edged ellipses: 255 inside, 0 outside, a ramp a few pixels wide between."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    a = np.zeros((h, w))
    for _ in range(3):
        cy, cx = rs.uniform(0.25, 0.75) * h, rs.uniform(0.25, 0.75) * w
        ry, rx = rs.uniform(0.1, 0.3) * h, rs.uniform(0.1, 0.3) * w
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        a = np.maximum(a, np.clip((1.0 - d) * min(ry, rx) / 4.0, 0.0, 1.0))
    return np.round(a * 255).astype(np.uint8)


def png(x):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'PNG')
    return buf.getvalue()


def pillow(datas):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('L')) for d in datas])).to(dev)


def main():
    rs = np.random.RandomState(0)
    work = [('one 512 x 512 file', [png(matte(rs, 512, 512))]), ('one 1080 x 1920 file', [png(matte(rs, 1080, 1920))]),
            ('a clip of 8 x 3 files, 512 x 512', [png(matte(rs, 512, 512)) for _ in range(24)])]
    rows = []
    for name, datas in work:
        assert torch.equal(pngdec.decode_planes(datas), pillow(datas))      # the same bytes as the codec
        fns = [lambda d=datas: pngdec.decode_planes(d), lambda d=datas: pillow(d)]
        r = pngdec.decode_stats(datas)
        names = ['%s (%d KB): pngdec.decode_planes; rounds %d (longest file), %d tokens, %d blocks, %d read-back' %
                 (name, sum(len(d) for d in datas) >> 10, int(r.rounds.max()), int(r.tokens.sum()), int(r.blocks.sum()), r.readbacks),
                 '  parent: Image.open().convert("L") on the host, host -> device']
        rows += list(zip(names, timed(fns, REPS)))
    print('%-110s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-110s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    entries = ['mg_pngdec_inflate', 'mg_pngdec_unfilter']
    for name, datas in work:
        hip.enable_timing(entries)
        for _ in range(20):
            pngdec.decode_planes(datas)
        torch.cuda.synchronize()
        rec = hip.disable_timing()['records']
        print('device time per entry point, %s (event pairs around the launches, median of 20 calls, us): ' % name +
              ', '.join('%s %.1f' % (e[3:], np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]])) for e in entries))


if __name__ == '__main__':
    main()
