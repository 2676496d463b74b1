"""Device time of MotionBlur (maggie_amd.utils.motion, csrc/motion.hip) on the crop of one video training item: 8 frames of 512 x 512 and the
alpha planes of the clip (8 frames x 3 instances), warm, device-resident table, every call bracketed by its own event pair, the candidates
alternated call by call. For ksize 3, 25 and 49, a full diagonal (the largest halo a ksize has: n = ksize taps, a ksize x ksize box) and a
full horizontal line (no extra rows):
  * the frames' launch, raw uint8 and with the Normalize epilogue;
  * the planes' launch.
Next to each time: the bytes the launch must move (input once, output once) and the time those bytes take at the measured HBM copy rate of
6.29 TB/s (MI355X; 8 TB/s is the datasheet's). The event pair also spans the host side of the call (the checks and one ctypes launch), so a
time near the launch overhead says little about the kernel. There is no parent to compare with: the step had no device form.
usage: python tools/motion_bench.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import motion

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
T, INST, H, W = 8, 3, 512, 512
HBM = 6.29e12


def main():
    rs = np.random.RandomState(0)
    frames = torch.from_numpy(rs.randint(0, 256, (T, H, W, 3)).astype(np.uint8)).to(dev)
    planes = torch.from_numpy(rs.randint(0, 256, (T * INST, H, W)).astype(np.uint8)).to(dev)
    names, fns, moved = [], [], []
    for ksize in (3, 25, 49):
        for shape, p0, p1 in (('diagonal', (0, 0), (ksize - 1, ksize - 1)), ('horizontal', (0, ksize // 2), (ksize - 1, ksize // 2))):
            d = motion.MotionDraws(motion.line_kernel(ksize, p0, p1)).to(dev)
            for what, fn, nbytes in (('frames raw', lambda d=d: motion.blur_frames(frames, d), 2 * frames.numel()),
                                     ('frames norm', lambda d=d: motion.blur_frames(frames, d, normalize=True), 5 * frames.numel()),
                                     ('planes', lambda d=d: motion.blur_planes(planes, d), 2 * planes.numel())):
                names.append('ksize %2d %-10s %-11s' % (ksize, shape, what))
                fns.append(fn)
                moved.append(nbytes)
    print('%d frames of %d x %d x 3, %d planes; %d calls each' % (T, H, W, T * INST, REPS))
    print('%-36s %10s %10s %10s %10s %10s %12s' % ('launch', 'median us', 'min us', 'p25 us', 'p75 us', 'MB moved', 'us at HBM'))
    for name, (med, mn, lo, hi), nbytes in zip(names, timed(fns, REPS), moved):
        print('%-36s %10.1f %10.1f %10.1f %10.1f %10.2f %12.2f' % (name, med, mn, lo, hi, nbytes / 1e6, nbytes / HBM * 1e6))


if __name__ == '__main__':
    main()
