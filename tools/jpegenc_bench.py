"""Time of the device JPEG encode (maggie_amd.utils.jpegenc, csrc/jpegenc.hip) at quality 75 on four workloads of seeded synthetic frames -- a
smooth scene with texture and noise, uint8 on the device, as `compose` leaves a canvas: one 512 x 512 frame, one 1080 x 1920 frame, and clips
of 8 and of 24 frames at 1080 x 1920. Warm, every call bracketed by its own event pair (the read-backs and the header lie between its events
too), the candidates alternated call by call:
  * `jpegenc.encode_clip(x, 75)` from the device frames to complete files in host memory;
  * the only thing that does the same job without it: `.cpu()` of the pixels and one `PIL.Image.save(buf, 'JPEG', quality=75)` per frame.
Neither side writes to disk. The tool first asserts that the device's files are Pillow's byte for byte. Then the device time per entry
point, from `hip.enable_timing`.
usage: python tools/jpegenc_bench.py [reps]"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import jpegenc

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 100


def scene(rs, h, w):
    """Gradients, a few soft discs, a fine texture and sensor-like noise: a file of about a tenth of the pixels at quality 75."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([60 + 120 * xx / w + 30 * yy / h, 200 - 100 * yy / h, 90 + 60 * np.sin(xx / 37.0) * np.cos(yy / 23.0)], -1)
    for _ in range(4):
        cy, cx, r = rs.uniform(0.2, 0.8) * h, rs.uniform(0.2, 0.8) * w, rs.uniform(0.05, 0.2) * min(h, w)
        d = np.clip((r - np.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)) / 6.0, 0, 1)[..., None]
        img = img * (1 - d) + d * rs.uniform(0, 255, 3)
    img += 12 * np.sin(xx / 2.3 + yy / 3.1)[..., None] + rs.normal(0, 4, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def host_path(x):
    out = []
    for f in x.cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(f).save(buf, 'JPEG', quality=75)
        out.append(buf.getvalue())
    return out


def main():
    rs = np.random.RandomState(0)
    work = [('one 512 x 512 frame', 1, 512, 512), ('one 1080 x 1920 frame', 1, 1080, 1920), ('a clip of 8, 1080 x 1920', 8, 1080, 1920),
            ('a clip of 24, 1080 x 1920', 24, 1080, 1920)]
    rows, kept = [], []
    base = {}
    for name, T, h, w in work:
        if (h, w) not in base:
            base[(h, w)] = scene(rs, h, w)
        x = torch.from_numpy(np.stack([np.roll(base[(h, w)], 7 * t, 1) for t in range(T)])).to(dev)
        files = jpegenc.encode_clip(x, 75)
        ref = host_path(x)
        assert files == ref, name                                             # Pillow's bytes
        fns = [lambda x=x: jpegenc.encode_clip(x, 75), lambda x=x: host_path(x)]
        reps = max(REPS // (4 if T > 1 else 1), 5)
        names = ['%s: jpegenc.encode_clip; %d KB of files, %d blocks, 2 read-backs' % (name, sum(len(f) for f in files) >> 10, T * jpegenc.blocks_of(h, w)),
                 '  host: .cpu() of the pixels, Pillow save(quality=75) per frame (%d calls)' % reps]
        rows += list(zip(names, timed(fns, reps)))
        kept.append((name, x))
    print('%-100s %10s %10s %10s %10s' % ('workload', 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-100s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    entries = ['mg_jpegenc_coef', 'mg_jpegenc_bits', 'mg_jpegenc_pack', 'mg_jpegenc_stuff']
    for name, x in kept:
        hip.enable_timing(entries)
        for _ in range(10):
            jpegenc.encode_clip(x, 75)
        torch.cuda.synchronize()
        rec = hip.disable_timing()['records']
        print('device time per entry point, %s (event pairs around the launches, median of 10 calls, us): ' % name +
              ', '.join('%s %.1f' % (e[3:], np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]])) for e in entries))


if __name__ == '__main__':
    main()
