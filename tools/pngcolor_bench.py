"""Time of the device PNG frame decode (maggie_amd.utils.pngcolor, csrc/pngcolor.hip) at 1080 x 1920 on seeded synthetic images: a
photograph-like one (smooth colour fields, edges and sensor noise) and an alpha-like one (soft-edged ellipses, mostly 0 and 255), as RGB 8 and
RGBA 8 files saved by Pillow at its defaults; the photograph quantised to a palette of 256; the photograph as an RGB 8 Adam7 file (Sub filter
on every row: Pillow writes no Adam7); the alpha-like one as grey 16 (decoded as an L plane). One file, and a clip of 24 (4 distinct images, 6 times
each). Warm, every call bracketed by its own event pair (host work of a call -- the chunk walk, the upload, the read-back -- lies between its
events too), the candidates alternated call by call:
  * `pngcolor.decode_frames` / `decode_planes` from the files' bytes;
  * the parent's only path: `Image.open(...).convert("RGB")` / `.convert("L")` per file on the host plus the host -> device copy.
The tool first asserts that both give the same bytes. Then the device time per entry point, from `hip.enable_timing`.
usage: python tools/pngcolor_bench.py [reps of one file] [reps of a clip]"""
import io
import os
import struct
import sys
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import pngcolor

dev = torch.device('cuda:0')
REPS1 = int(sys.argv[1]) if len(sys.argv) > 1 else 30
REPS24 = int(sys.argv[2]) if len(sys.argv) > 2 else 5
H, W = 1080, 1920


def photo(rs):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    c = []
    for k in range(3):
        f = 128 + 60 * np.sin(xx / rs.uniform(60, 300) + rs.uniform(0, 6)) * np.cos(yy / rs.uniform(60, 300)) + 40 * np.sin((xx + yy) / rs.uniform(20, 80))
        f += 50 * ((xx // rs.randint(150, 400) + yy // rs.randint(150, 400)) % 2)          # edges
        c.append(f + rs.normal(0, 3, (H, W)))                                           # sensor noise
    return np.clip(np.stack(c, -1), 0, 255).astype(np.uint8)


def matte(rs):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.zeros((H, W))
    for _ in range(3):
        cy, cx = rs.uniform(0.25, 0.75) * H, rs.uniform(0.25, 0.75) * W
        ry, rx = rs.uniform(0.1, 0.3) * H, rs.uniform(0.1, 0.3) * W
        d = np.sqrt(((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2)
        a = np.maximum(a, np.clip((1.0 - d) * min(ry, rx) / 4.0, 0.0, 1.0))
    return a


def save(im):
    buf = io.BytesIO()
    im.save(buf, 'PNG')
    return buf.getvalue()


def chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body))


def adam7(x):
    """uint8 (h, w, 3) -> an RGB 8 Adam7 file, Sub filter on every row of every pass."""
    raw = []
    for x0, y0, dx, dy in pngcolor.ADAM7:
        sub = x[y0::dy, x0::dx].reshape(len(range(y0, H, dy)), -1)
        if sub.size:
            f = sub.copy()
            f[:, 3:] -= sub[:, :-3]
            raw.append(np.concatenate([np.ones((f.shape[0], 1), np.uint8), f], 1).tobytes())
    return pngcolor.SIGNATURE + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 1)) + chunk(b'IDAT', zlib.compress(b''.join(raw))) + \
        chunk(b'IEND', b'')


def pillow(datas, mode):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(d)).convert(mode)) for d in datas])).to(dev)


def main():
    rs = np.random.RandomState(0)
    photos, mattes = [photo(rs) for _ in range(4)], [matte(rs) for _ in range(4)]
    grey = [np.round(m * 255).astype(np.uint8) for m in mattes]
    kinds = [('RGB 8, photograph', 'RGB', [save(Image.fromarray(p)) for p in photos]),
             ('RGB 8, alpha-like', 'RGB', [save(Image.fromarray(np.repeat(g[..., None], 3, -1))) for g in grey]),
             ('RGBA 8, photograph + alpha', 'RGB', [save(Image.fromarray(np.concatenate([p, g[..., None]], -1), 'RGBA')) for p, g in zip(photos, grey)]),
             ('RGBA 8, alpha-like', 'RGB', [save(Image.fromarray(np.repeat(g[..., None], 4, -1), 'RGBA')) for g in grey]),
             ('palette 8, photograph', 'RGB', [save(Image.fromarray(p).quantize(256)) for p in photos]),
             ('RGB 8 Adam7, photograph', 'RGB', [adam7(p) for p in photos]),
             ('grey 16, alpha-like', 'L', [save(Image.fromarray(np.round(m * 65535).astype(np.uint16))) for m in mattes])]
    rows = []
    for name, mode, four in kinds:
        for label, datas, reps in (('one file', four[:1], REPS1), ('clip of 24', four * 6, REPS24)):
            plan = pngcolor.parse(datas[0])
            assert (plan.height, plan.width) == (H, W)
            device = (lambda d=datas: pngcolor.decode_frames(d)) if mode == 'RGB' else (lambda d=datas: pngcolor.decode_planes(d))
            assert torch.equal(device(), pillow(datas, mode))          # the same bytes as the codec
            r = pngcolor.decode_stats(datas, planes=mode == 'L')
            names = ['%s, %s (%d KB, type %d depth %d interlace %d): pngcolor; rounds %d (longest file), %d read-back' %
                     (name, label, sum(len(d) for d in datas) >> 10, plan.color_type, plan.depth, plan.interlace, int(r.rounds.max()), r.readbacks),
                     '  parent: Image.open().convert("%s") on the host, host -> device' % mode]
            rows += list(zip(names, timed([device, lambda d=datas, m=mode: pillow(d, m)], reps, warmup=2)))
    print('%-120s %10s %10s %10s %10s' % ('workload at %d x %d (%d / %d calls each)' % (H, W, REPS1, REPS24), 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-120s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))
    entries = ['mg_pngcolor_inflate', 'mg_pngcolor_unfilter', 'mg_pngcolor_convert']
    for name, mode, four in kinds:
        for label, datas in (('one file', four[:1]), ('clip of 24', four * 6)):
            hip.enable_timing(entries)
            for _ in range(5):
                pngcolor.decode_stats(datas, planes=mode == 'L')
            torch.cuda.synchronize()
            rec = hip.disable_timing()['records']
            print('device time per entry point, %s, %s (event pairs around the launches, median of 5 calls, us): ' % (name, label) +
                  ', '.join('%s %.1f' % (e[3:], np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]])) for e in entries))


if __name__ == '__main__':
    main()
