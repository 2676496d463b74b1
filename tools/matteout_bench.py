"""Time of the device matte output (maggie_amd.utils.matteout, csrc/matteout.hip) on three workloads of seeded synthetic data -- a uint8 frame on
the device and the network's fp32 alpha at ResizeShort(576) + PaddingMultiplyBy(64), as the predictor has them behind the forward: one
1080 x 1920 frame with 5 instances, a clip of 3 such frames, one 512 x 512 frame with 2 instances. Warm, every call bracketed by its own event
pair, the candidates alternated call by call:
  (a)  `matteout.composite(frame, alpha, transform_info=info, snap=True, fused=True)`: one launch from the network-size alpha to the composites;
  (a2) the two-launch form, which `composite` takes by default: `reverse_transform_tensor(snap=True)`, then the identity composite;
  (b)  what the package offered before: `reverse_transform_tensor(snap=True)`, then the reference's expression in torch ops on the device;
  (c)  the reference's host path: the reverse transform on the device, `.cpu().numpy()`, the snapping and the NumPy loop of
       demo/maggie_predictor.py:63-76.
The tool first asserts that (a), (a2) and (c)'s formula applied to (a)'s alpha give the same bytes. Then the bytes each form moves and the
fraction of the HBM rate (a) reaches.
usage: python tools/matteout_bench.py [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from _timing import timed
from maggie_amd.utils import geometry, matteout
from maggie_amd.utils.postprocessing import reverse_transform_tensor

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
HBM_GBS = 8000.0                                                    # MI355X: 8 TB/s peak


def torch_ops(frames, alpha):
    """(image * a + (1 - a) * green_bg).astype(uint8) in torch ops: frames (T, H, W, 3) uint8, alpha (T, P, H, W) fp32."""
    a = alpha[..., None]
    bg = torch.zeros_like(frames)
    bg[..., 1] = 255
    return (frames[:, None] * a + (1 - a) * bg[:, None]).to(torch.uint8)


def host_path(frames, pred, info):
    alpha = reverse_transform_tensor(pred, info).cpu().numpy()
    alpha[alpha <= 1.0 / 255.0] = 0.0
    alpha[alpha >= 254.0 / 255.0] = 1.0
    images = frames.cpu().numpy()
    out = []
    for t in range(alpha.shape[0]):
        green = np.zeros_like(images[t])
        green[:, :, 1] = 255
        for i in range(alpha.shape[1]):
            a = alpha[t, i][:, :, None]
            out.append((images[t] * a + (1 - a) * green).astype(np.uint8))
    return out


def main():
    rs = np.random.RandomState(0)
    work = [('one 1080 x 1920 frame, P = 5', 1, 5, 1080, 1920), ('a clip of 3, 1080 x 1920, P = 5', 3, 5, 1080, 1920), ('one 512 x 512 frame, P = 2', 1, 2, 512, 512)]
    rows = []
    for name, T, P, H, W in work:
        plan = geometry.plan(H, W, 576, 64)
        info = plan.transform_info
        h, w = plan.out_h, plan.out_w
        frames = torch.from_numpy(rs.randint(0, 256, size=(T, H, W, 3)).astype(np.uint8)).to(dev)
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
        blobs = [np.clip(1.3 - np.hypot(yy - rs.uniform(0.2, 0.8) * h, xx - rs.uniform(0.2, 0.8) * w) / (0.3 * h), 0, 1) for _ in range(T * P)]
        pred = torch.from_numpy(np.stack(blobs).astype(np.float32).reshape(T, P, h, w)).to(dev)
        fused, alpha = matteout.composite(frames, pred, transform_info=info, snap=True, return_alpha=True, fused=True)
        two = matteout.composite(frames, pred, transform_info=info, snap=True)
        ref = host_path(frames, pred, info)
        want = np.stack([(frames[t].cpu().numpy() * a[:, :, None] + (1 - a[:, :, None]) * np.array([0, 255, 0], np.uint8)).astype(np.uint8)
                         for t in range(T) for a in alpha[t].cpu().numpy()])
        assert np.array_equal(fused.cpu().numpy().reshape(want.shape), want), name
        diff_two = int((two != fused).sum())                                  # the existing reverse transform contracts: its alpha differs by an ulp here and there
        diff_ref = int((np.stack(ref) != want).sum())
        fns = [lambda: matteout.composite(frames, pred, transform_info=info, snap=True, fused=True),
               lambda: matteout.composite(frames, pred, transform_info=info, snap=True),
               lambda: torch_ops(frames, reverse_transform_tensor(pred, info, snap=True)),
               lambda: host_path(frames, pred, info)]
        reps = max(REPS // T, 5)
        res = timed(fns, reps, warmup=3)
        crop = (h - plan.pad_h) * (w - plan.pad_w)
        moved = T * H * W * 3 + T * P * (H * W * 3 + crop * 4)                 # the frame once, every composite once, the cropped alpha once
        labels = ['(a)  composite(fused=True), one launch: %.1f MB moved' % (moved / 1e6),
                  '(a2) composite() by default, reverse transform + identity composite: %.1f MB moved; %d bytes differ from (a)' % ((moved + 2 * T * P * H * W * 4) / 1e6, diff_two),
                  '(b)  reverse transform + torch ops',
                  '(c)  host: .cpu().numpy() of %.1f MB fp32 + the NumPy loop (%d calls); %d bytes differ from (a)' % (T * P * H * W * 4 / 1e6, reps, diff_ref)]
        rows.append((name, None))
        rows += list(zip(labels, res))
        for k, mv in ((0, moved), (1, moved + 2 * T * P * H * W * 4)):
            rows.append(('     (%s) reaches %.0f GB/s, %.1f %% of the %.0f GB/s HBM rate' % (('a', 'a2')[k], mv / res[k][0] / 1e3, 100 * mv / res[k][0] / 1e3 / HBM_GBS, HBM_GBS), None))
    print('%-110s %10s %10s %10s %10s' % ('workload', 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, r in rows:
        print(name if r is None else '  %-108s %10.1f %10.1f %10.1f %10.1f' % ((name,) + r))


if __name__ == '__main__':
    main()
