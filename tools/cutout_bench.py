"""Time of the device cut-outs (maggie_amd.utils.cutout, csrc/cutout.hip) and of the colour PNG writer (`pngenc.encode_images`) on the
predictor's workload of seeded synthetic data: one 1080 x 1920 uint8 frame on the device and the fp32 alpha of 5 instances at full size, as
`matteout.composite` leaves it. Warm, every call bracketed by its own event pair, the candidates alternated call by call:
  (a) `cutout.estimate_foreground(frame, alpha)`: the byte conversion and four launches for the five planes;
  (b) `cutout.cutout(frame, alpha)`: the same with the RGBA store;
  (c) the host form of the same statement: `.cpu().numpy()` of the fp32 alpha and tests/cutout_restatement.py's NumPy (cumulative sums, fp64);
  (d) `pngenc.encode_images` of the five RGBA cut-outs, from the device tensor to complete files in host memory;
  (e) the host path to the same files: `.cpu().numpy()` of the cut-outs and one Pillow `save(compress_level=1)` per image.
Neither side writes to disk. The tool first asserts that (b) equals (c) byte for byte and that Pillow reads (d)'s files back as the cut-outs.
Then the device time per entry point from `hip.enable_timing`, and the bytes the two passes must move.
usage: python tools/cutout_bench.py [reps]"""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from PIL import Image

import cutout_restatement as C
from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import cutout, pngenc

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
HBM_GBS = 8000.0                                                    # MI355X: 8 TB/s peak


def scene(rs, P, H, W):
    """A smooth, textured frame and P soft-edged blobs (1 inside, 0 outside, a ramp of some twenty pixels between)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frame = np.stack([128 + 100 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0 - c) + rs.uniform(-12, 12, (H, W)) for c in range(3)], -1)
    blobs = [np.clip((0.22 * H - np.hypot(yy - rs.uniform(0.3, 0.7) * H, xx - rs.uniform(0.2, 0.8) * W)) / 20.0 + 0.5, 0, 1) for _ in range(P)]
    return np.clip(frame, 0, 255).astype(np.uint8), np.stack(blobs).astype(np.float32)


def host_estimate(frame, alpha):
    a = alpha.cpu().numpy()
    f = frame.cpu().numpy()
    return np.stack([C.cutout(f, p) for p in a])


def host_files(cut):
    out = []
    for im in cut.cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, 'PNG', compress_level=1)
        out.append(buf.getvalue())
    return out


def main():
    rs = np.random.RandomState(0)
    P, H, W = 5, 1080, 1920
    f_np, a_np = scene(rs, P, H, W)
    frame, alpha = torch.from_numpy(f_np).to(dev), torch.from_numpy(a_np).to(dev)
    cut = cutout.cutout(frame, alpha)[0]
    want = host_estimate(frame, alpha)
    assert np.array_equal(cut.cpu().numpy(), want), 'the device cut-outs are not the statement\'s'
    files = pngenc.encode_images(cut)
    for f, im in zip(files, want):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), im)
    ref = host_files(cut)
    fast = timed([lambda: cutout.estimate_foreground(frame, alpha), lambda: cutout.cutout(frame, alpha)], REPS, warmup=3)
    files_t = timed([lambda: pngenc.encode_images(cut), lambda: host_files(cut)], max(REPS // 3, 5), warmup=2)
    slow = timed([lambda: host_estimate(frame, alpha)], 3, warmup=1)
    rows = [('(a) cutout.estimate_foreground, radii (90, 6)', fast[0]), ('(b) cutout.cutout, radii (90, 6)', fast[1]),
            ('(c) host: .cpu().numpy() of %.1f MB fp32 alpha + the NumPy statement (3 calls)' % (a_np.nbytes / 1e6), slow[0]),
            ('(d) pngenc.encode_images of the 5 RGBA cut-outs: %d KB of files, %d blocks, 2 read-backs' % (sum(len(f) for f in files) >> 10, P * pngenc.blocks_of(H, 4 * W)), files_t[0]),
            ('(e) host: .cpu().numpy() of %.1f MB RGBA + Pillow save(compress_level=1) per image: %d KB of files' % (P * H * W * 4 / 1e6, sum(len(f) for f in ref) >> 10), files_t[1])]
    print('one 1080 x 1920 frame, P = 5')
    print('%-118s %12s %12s %12s %12s' % ('', 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, r in rows:
        print('  %-116s %12.1f %12.1f %12.1f %12.1f' % ((name,) + r))
    entries = ['mg_cutout_alpha_bytes', 'mg_cutout_estimate', 'mg_pngenc_size_rgb', 'mg_pngenc_emit_rgb']
    hip.enable_timing(entries)
    for _ in range(10):
        pngenc.encode_images(cutout.cutout(frame, alpha)[0])
    torch.cuda.synchronize()
    rec = hip.disable_timing()['records']
    med = {e: float(np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]])) for e in entries}
    print('device time per entry point (event pairs around the launches, median of 10 calls, us): ' + ', '.join('%s %.1f' % (e[3:], med[e]) for e in entries))
    n = P * H * W
    # per pass: the row kernel reads 7 bytes a pixel (F, B, a; the frame twice in pass one) and writes 28; the column kernel reads the 28 at
    # least once, 4 bytes of frame and alpha, and writes 6 (pass one) or 4 (the RGBA)
    least = n * ((7 + 28) + (28 + 4 + 6)) + n * ((7 + 28) + (28 + 4 + 4))
    print('the two passes move at least %.0f MB (row sums written and read once): %.0f GB/s at the measured time, %.1f %% of the %.0f GB/s HBM rate'
          % (least / 1e6, least / med['mg_cutout_estimate'] / 1e3, 100 * least / med['mg_cutout_estimate'] / 1e3 / HBM_GBS, HBM_GBS))


if __name__ == '__main__':
    main()
