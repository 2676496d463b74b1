"""Time of the device JPEG decode (maggie_amd.utils.jpegdec, csrc/jpegdec.hip) on three workloads: one 512 x 512 file, one 1080 x 1920 file and
a clip of 8 files at 512 x 512, all quality 90, 4:2:0, written by Pillow from a smooth-plus-noise picture made here. Warm, every call
bracketed by its own event pair (host work of a call -- the marker walk, the upload, the read-back -- lies between its events too), the
candidates alternated call by call:
  * `jpegdec.decode` / `decode_clip` from the files' bytes;
  * the parent's only alternative: `Image.open(...).convert("RGB")` per file on the host plus the host -> device copy.
The tool first asserts that both give the same bytes. Then a sweep of `sub_bytes` over the powers of two `mg_jpegdec_limits` allows, with the
rounds, launches and read-backs each used; the default `sub_bytes` is the sweep's best on the 1080p file.
usage: python tools/jpegdec_bench.py [reps]"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import jpegdec

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def picture(rs, h, w, t=0):
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([60 + 0.3 * xx + 0.1 * yy + 5 * t, 200 - 0.25 * yy, 90 + 60 * (((xx + 8 * t) // 64 + yy // 48) % 2)], -1)
    return np.clip(base + rs.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)


def jpeg(x):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', quality=90, subsampling=2)
    return buf.getvalue()


def pillow(datas):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas])).to(dev)


def main():
    rs = np.random.RandomState(0)
    work = [('one 512 x 512 file', [jpeg(picture(rs, 512, 512))]), ('one 1080 x 1920 file', [jpeg(picture(rs, 1080, 1920))]),
            ('a clip of 8 files, 512 x 512', [jpeg(picture(rs, 512, 512, t)) for t in range(8)])]
    rows = []
    for name, datas in work:
        assert torch.equal(jpegdec.decode_clip(datas), pillow(datas))       # the same bytes as the codec
        fns = [lambda d=datas: jpegdec.decode_clip(d), lambda d=datas: pillow(d)]
        r = jpegdec.decode_stats(datas)
        names = ['%s (%d KB): jpegdec.decode_clip, sub_bytes %d; %d rounds, %d launches, %d read-back(s)' %
                 (name, sum(len(d) for d in datas) >> 10, jpegdec.DEFAULT_SUB, r.rounds, r.launches, r.readbacks),
                 '  parent: Image.open().convert("RGB") on the host, host -> device']
        rows += list(zip(names, timed(fns, REPS)))
    print('%-110s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-110s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    entries = ['mg_jpegdec_sync', 'mg_jpegdec_coef', 'mg_jpegdec_dcsum', 'mg_jpegdec_idct', 'mg_jpeg_rgb']
    for name, datas in work:
        hip.enable_timing(entries)
        for _ in range(20):
            jpegdec.decode_clip(datas)
        torch.cuda.synchronize()
        rec = hip.disable_timing()['records']
        print('device time per entry point, %s (event pairs around the launches, median of 20 calls, us): ' % name +
              ', '.join('%s %.1f x %d' % (e[3:], np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]]), len(rec[e]) // 20) for e in entries))
    subs = [s for s in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096) if jpegdec.MIN_SUB <= s <= jpegdec.MAX_SUB]
    for name, datas in work[:2]:
        print('sub_bytes sweep, %s (%d calls each, alternated)' % (name, REPS))
        stats = [jpegdec.decode_stats(datas, sub_bytes=s) for s in subs]
        res = timed([lambda d=datas, s=s: jpegdec.decode_clip(d, sub_bytes=s) for s in subs], REPS, warmup=3)
        print('%10s %14s %8s %9s %10s %10s %10s' % ('sub_bytes', 'subsequences', 'rounds', 'launches', 'read-backs', 'median us', 'min us'))
        for s, st, (med, mn, _, _) in zip(subs, stats, res):
            print('%10d %14d %8d %9d %10d %10.1f %10.1f' % (s, st.subsequences, st.rounds, st.launches, st.readbacks, med, mn))


if __name__ == '__main__':
    main()
