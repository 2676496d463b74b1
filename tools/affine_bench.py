"""Device time of RandomAffine (maggie_amd.utils.affine, csrc/affine.hip) for one training item of each kind after the 512 x 512 crop: an image
item (one frame, 8 instance planes of alphas) and a video item (8 frames, 24 planes), at the reference's parameter extremes (10 degrees, 5
degrees of shear, zoom 0.95 / 1.05), warm, device-resident draws, every call bracketed by its own event pair, the candidates alternated call
by call:
  * `apply` with the frames' staged regime (the tile's source box in LDS) and with the direct regime (four global taps per pixel): which one
    is the default for how many frames (affine.STAGED_MIN_FRAMES) follows from these two lines;
  * the parent's only equivalent: the crops copied device -> host and an fp32 image of the same size copied host -> device (pinned buffers),
    and NOTHING for the warp itself, which the parent cannot do without OpenCV -- a floor for the parent, not its cost;
  * the three launches on their own: the nearest warp of the planes, the linear warp of the frames (both regimes), the shift + Normalize.
usage: python tools/affine_bench.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import affine

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
H = W = 512


def extreme_matrix():
    """rotation 10 degrees . shear 5 degrees (first form) . zoom (0.95, 1.05) about the reference's offset centre, as `affine.draw` composes it."""
    t, s = np.pi / 180 * 10, np.pi / 180 * 5
    rot = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    sh = np.array([[1, -np.sin(s), 0], [0, np.cos(s), 0], [0, 0, 1]])
    m = affine._offset_center(np.dot(np.dot(rot, sh), np.array([[0.95, 0, 0], [0, 1.05, 0], [0, 0, 1]])), H, W)
    cvM = np.zeros_like(m[:2, :])
    cvM[:2, :2] = np.flipud(np.fliplr(m[:2, :2]))
    cvM[:2, 2] = np.flip(m[:2, 2], axis=0)
    return cvM


def main():
    rs = np.random.RandomState(0)
    rows = []
    d = affine.from_matrix(extreme_matrix(), H, W, 5.25)
    assert d.staged_ok
    print('largest staged box: %d of %d bytes' % (affine.box_bytes(d.linear, H, W), affine.BOX_BYTES))
    d = d.to(dev)
    for kind, T, P in (('image', 1, 8), ('video', 8, 24)):
        frames = torch.from_numpy(rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)).to(dev)
        alphas = torch.from_numpy(rs.randint(0, 256, size=(P, H, W)).astype(np.uint8)).to(dev)
        host_f, host_a = torch.empty(frames.shape, dtype=torch.uint8).pin_memory(), torch.empty(alphas.shape, dtype=torch.uint8).pin_memory()
        host_image = torch.zeros((T, 3, H, W), dtype=torch.float32).pin_memory()
        dev_image, dev_a = torch.empty((T, 3, H, W), dtype=torch.float32, device=dev), torch.empty_like(alphas)

        def parent():
            host_f.copy_(frames, non_blocking=True)
            host_a.copy_(alphas, non_blocking=True)
            dev_image.copy_(host_image, non_blocking=True)
            dev_a.copy_(host_a, non_blocking=True)
        a, b = affine.apply(frames, alphas, d, regime='staged'), affine.apply(frames, alphas, d, regime='direct')
        assert all(torch.equal(x, y) for x, y in zip(a, b))                   # the two regimes give the same bits
        warped, _, mm = affine.warp(frames, None, d, return_minmax=True)
        names = ['%s item: apply, staged regime (%d frames, %d planes)' % (kind, T, P), '  apply, direct regime',
                 '  parent floor: crops device -> host, fp32 image + planes host -> device, no warp',
                 '  planes alone (mg_affine_warp_planes)', '  frames alone, staged (mg_affine_warp_frames)', '  frames alone, direct',
                 '  shift + Normalize alone (mg_affine_shift_normalize)']
        fns = [lambda: affine.apply(frames, alphas, d, regime='staged'), lambda: affine.apply(frames, alphas, d, regime='direct'), parent,
               lambda: affine.warp(frames[:0], alphas, d), lambda: affine.warp(frames, None, d, regime='staged'),
               lambda: affine.warp(frames, None, d, regime='direct'), lambda: affine.shift_normalize(warped, mm, d.shift)]
        rows += list(zip(names, timed(fns, REPS)))
    print('%-100s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, (med, mn, lo, hi) in rows:
        print('%-100s %10.1f %10.1f %10.1f %10.1f' % (name, med, mn, lo, hi))


if __name__ == '__main__':
    main()
