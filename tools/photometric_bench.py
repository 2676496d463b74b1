"""Device time of the photometric steps (maggie_amd.utils.photometric, csrc/photometric.hip) on the crop of one training item of each kind:
an image item (one 512 x 512 frame) and a video item (8 frames), warm, device-resident draws, every call bracketed by its own event pair, the
candidates alternated call by call:
  * `apply(normalize=True)` with all three steps (tone curve, noise, JPEG at quality 35);
  * the JPEG round trip alone, raw uint8;
  * the parent's only alternative for the JPEG step: device -> host copy, `PIL.Image.save(quality)` / `PIL.Image.open` per frame, host ->
    device copy (skipped with a note where Pillow is absent).
The tool first asserts that the variants agree bit for bit (the all-three variant against Pillow on the host-side curve and noise).
usage: python tools/photometric_bench.py [reps]"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import photometric
from maggie_amd.utils.preprocess import normalize_frames

try:
    from PIL import Image
except ImportError:
    Image = None

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
H, W, QUALITY = 512, 512, 35


def pillow(x):
    out = np.empty_like(x)
    for t in range(x.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(x[t]).save(buf, format='JPEG', quality=QUALITY)
        buf.seek(0)
        out[t] = np.asarray(Image.open(buf))
    return out


def picture(rs, T):
    """Frames with structure and grain (a codec's time depends on its input): gradients, a few edges, noise."""
    yy, xx = np.mgrid[0:H, 0:W]
    frames = []
    for t in range(T):
        base = np.stack([60 + 0.3 * xx + 0.1 * yy + 5 * t, 200 - 0.25 * yy, 90 + 60 * (((xx + 8 * t) // 64 + yy // 48) % 2)], -1)
        frames.append(np.clip(base + rs.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8))
    return np.stack(frames)


def main():
    rs = np.random.RandomState(0)
    lut = np.clip(255 * (np.arange(256) / 255.) ** 0.8, 0, 255).astype(np.uint8)[None].repeat(3, 0)
    noise = np.clip(np.round(rs.normal(0, 10, (H, W, 1))), -255, 255).astype(np.int16)
    rows = []
    for kind, T in (('image', 1), ('video', 8)):
        host = picture(rs, T)
        frames = torch.from_numpy(host).to(dev)
        all_three = photometric.PhotoDraws(lut, noise, QUALITY).to(dev)
        only_jpeg = photometric.PhotoDraws(quality=QUALITY).to(dev)

        def full():
            return photometric.apply(frames, all_three, normalize=True)

        def jpeg():
            return photometric.apply(frames, only_jpeg)

        def parent():
            return torch.from_numpy(pillow(frames.cpu().numpy())).to(dev)
        names = ['%s item: apply(normalize=True), curve + noise + JPEG (%d x %d x %d)' % (kind, T, H, W), '  JPEG round trip alone, raw uint8',
                 '  parent: device -> host, Pillow save / open, host -> device']
        fns = [full, jpeg, parent]
        if Image is None:
            print('Pillow is not installed: the parent variant and the bit comparison against it are skipped')
            names, fns = names[:2], fns[:2]
        else:
            assert torch.equal(jpeg(), parent())                            # the same bits as the codec
            toned = np.stack([lut[c][host[..., c]] for c in range(3)], -1)
            noisy = np.clip(toned.astype(np.int32) + noise, 0, 255).astype(np.uint8)
            assert torch.equal(full(), normalize_frames(torch.from_numpy(pillow(noisy)).to(dev)))
        rows += list(zip(names, timed(fns, REPS)))
    print('%-90s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-90s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))


if __name__ == '__main__':
    main()
