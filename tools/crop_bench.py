"""Device time of the training crop (maggie_amd.utils.crop, csrc/crop.hip) for one training item of each kind after ResizeShort(576) +
PaddingMultiplyBy(64): an image item (one 576 x 768 frame, 8 instance planes of alphas and of masks) and a video item (8 frames, 24 planes),
cropped to 512 x 512 and flipped, warm, device-resident draws, every call bracketed by its own event pair, the candidates alternated call by
call:
  * `apply(normalize=True)` on the crop branch with the gather's own Normalize epilogue, and with the raw gather followed by
    `normalize_frames` (crop.FUSED_NORMALIZE on / off: which one is the default follows from these two lines);
  * the parent's nearest equivalent: torch slicing, `flip` and `contiguous()` on the device, then `normalize_frames`;
  * the padding branch, which has no parent equivalent: its line stands alone;
  * the two questions of `draw_on_device` on their own (box, three candidate windows), without their read-backs.
usage: python tools/crop_bench.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import crop
from maggie_amd.utils.preprocess import normalize_frames

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
H, W, CROP = 576, 768, (512, 512)


def main():
    rs = np.random.RandomState(0)
    rows = []
    for kind, T, P in (('image', 1, 8), ('video', 8, 24)):
        frames = torch.from_numpy(rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)).to(dev)
        alphas = torch.from_numpy(rs.randint(0, 256, size=(P, H, W)).astype(np.uint8)).to(dev)
        masks = torch.from_numpy((rs.rand(P, H, W) < 0.5).astype(np.uint8) * 255).to(dev)
        x0, y0 = 131, 37
        cd = crop.CropDraws('crop', H, W, CROP, True, 512, 512, window=np.asarray([x0, y0, 1], np.int32), pairs=1).to(dev)
        pad_h, pad_w, oh, ow, linear, nearest = crop.pad_tables(H, W, CROP, True)
        pd = crop.CropDraws('pad', H, W, CROP, True, oh, ow, pad=(pad_h, pad_w), linear=linear, nearest=nearest).to(dev)
        windows = torch.tensor([[x0, y0], [0, 0], [256, 64]], dtype=torch.int32, device=dev)

        def fused(on):
            def run():
                saved, crop.FUSED_NORMALIZE = crop.FUSED_NORMALIZE, on
                try:
                    return crop.apply(frames, alphas, masks, cd, normalize=True)
                finally:
                    crop.FUSED_NORMALIZE = saved
            return run

        def parent():
            f = frames[:, y0:y0 + 512, x0:x0 + 512].flip(2).contiguous()
            a = alphas[:, y0:y0 + 512, x0:x0 + 512].flip(2).contiguous()
            m = masks[:, y0:y0 + 512, x0:x0 + 512].flip(2).contiguous()
            return normalize_frames(f), a, m
        a, b, c = fused(True)(), fused(False)(), parent()
        assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a, b, c))              # the three candidates give the same bits
        names = ['%s item: apply(normalize=True), gather with the Normalize epilogue (%d + 2 x %d images)' % (kind, T, P),
                 '  apply(normalize=True), raw gather + normalize_frames', '  parent: torch slice + flip + contiguous, normalize_frames',
                 '  padding branch: apply(normalize=True) (pad %d + resize 576 x 768 -> 512 x 512)' % pad_h,
                 '  box of the alphas (mg_crop_bbox, no read-back)', '  three candidate windows (mg_crop_hits, no read-back)']
        fns = [fused(True), fused(False), parent, lambda: crop.apply(frames, alphas, masks, pd, normalize=True), lambda: crop.bbox(alphas),
               lambda: crop.window_hits(alphas, windows, CROP)]
        rows += list(zip(names, timed(fns, REPS)))
    print('%-100s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-100s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))


if __name__ == '__main__':
    main()
