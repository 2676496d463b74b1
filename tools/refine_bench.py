"""Time of the device matte refinement (maggie_amd.utils.refine, csrc/refine.hip) on the predictor's workload of seeded synthetic data: one
2160 x 3840 uint8 frame on the device and the fp32 alpha of 5 instances at the network's size, 576 x 1024 (`ResizeShort(576)`, no padding at
this size). Warm, every call bracketed by its own event pair, the candidates alternated call by call:
  (a) `refine.refine(frame, alpha, transform_info=..., snap=True)`: the guide's resize, the byte conversion, six launches at low resolution and
      one at full size;
  (b) the same with `as_float=True` (what `predict_image(refine=True)` calls);
  (c) `postprocessing.reverse_transform_tensor(alpha, transform_info, snap=True)`, the call `refine` replaces: one bilinear launch, fp32 out;
  (d) the host form of the statement: `.cpu().numpy()` of the frame, the guide and the alpha and tests/refine_restatement.py's NumPy.
The tool first asserts that the device bytes equal the statement's on a small case (a 270 x 480 frame at 144 x 256). Then the device time per
entry point from `hip.enable_timing`, and the full-size kernel's share of the HBM rate for the H W (3 + P) bytes a frame it must move
(DESIGN.md section 36).
usage: python tools/refine_bench.py [reps]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import refine_restatement as R
from _timing import timed
from maggie_amd import hip
from maggie_amd.utils import geometry, postprocessing, refine

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
HBM_GBS = 8000.0                                                    # MI355X: 8 TB/s peak


def scene(rs, P, H, W, h, w, ph, pw):
    """A smooth, textured frame and, at the network's size (h, w) inside (ph, pw) planes, P soft-edged blobs."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frame = np.stack([128 + 100 * np.sin(xx / 37.0 + c) * np.cos(yy / 23.0 - c) + rs.uniform(-12, 12, (H, W)) for c in range(3)], -1)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    alpha = np.zeros((P, ph, pw), np.float32)
    for k in range(P):
        alpha[k, :h, :w] = np.clip((0.22 * h - np.hypot(yy - rs.uniform(0.3, 0.7) * h, xx - rs.uniform(0.2, 0.8) * w)) / 6.0 + 0.5, 0, 1)
    return np.clip(frame, 0, 255).astype(np.uint8), alpha


def host_refine(frame, alpha, plan):
    f = frame.cpu().numpy()
    g = geometry.resize(frame, (plan.rw, plan.rh), 'linear', channels=3).cpu().numpy()
    a = alpha.cpu().numpy()[:, :plan.rh, :plan.rw]
    return np.stack([R.refine(f, g, p, snap=True) for p in a])


def case(rs, P, H, W):
    plan = geometry.plan(H, W, 576 if H > 1000 else 144, 64)
    f_np, a_np = scene(rs, P, H, W, plan.rh, plan.rw, plan.out_h, plan.out_w)
    return plan, torch.from_numpy(f_np).to(dev), torch.from_numpy(a_np).to(dev)


def main():
    rs = np.random.RandomState(0)
    plan, frame, alpha = case(rs, 2, 270, 480)
    got = refine.refine(frame, alpha, transform_info=plan.transform_info, snap=True)[0]
    assert np.array_equal(got.cpu().numpy(), host_refine(frame, alpha, plan)), 'the device bytes are not the statement\'s'
    P, H, W = 5, 2160, 3840
    plan, frame, alpha = case(rs, P, H, W)
    info = plan.transform_info
    print('one %d x %d frame, P = %d, network size %d x %d (planes of %d x %d)' % (H, W, P, plan.rh, plan.rw, plan.out_h, plan.out_w))
    fast = timed([lambda: refine.refine(frame, alpha, transform_info=info, snap=True),
                  lambda: refine.refine(frame, alpha, transform_info=info, snap=True, as_float=True),
                  lambda: postprocessing.reverse_transform_tensor(alpha, info, snap=True)], REPS, warmup=3)
    slow = timed([lambda: host_refine(frame, alpha, plan)], 1, warmup=0)
    rows = [('(a) refine.refine, radius 5, eps 1e-4, snap: uint8 out', fast[0]), ('(b) refine.refine, as_float: fp32 out', fast[1]),
            ('(c) postprocessing.reverse_transform_tensor(snap=True): bilinear, fp32 out', fast[2]),
            ('(d) host: .cpu().numpy() of the frame, the guide and the alpha + the NumPy statement (1 call)', slow[0])]
    print('%-100s %12s %12s %12s %12s' % ('', 'median us', 'min us', 'p25 us', 'p75 us'))
    for name, r in rows:
        print('  %-98s %12.1f %12.1f %12.1f %12.1f' % ((name,) + r))
    entries = ['mg_resize_u8', 'mg_cutout_alpha_bytes', 'mg_refine_coefficients', 'mg_refine_apply']
    hip.enable_timing(entries)
    for _ in range(10):
        refine.refine(frame, alpha, transform_info=info, snap=True)
    torch.cuda.synchronize()
    rec = hip.disable_timing()['records']
    med = {e: float(np.median([a.elapsed_time(b) * 1e3 for a, b, _, _ in rec[e]])) for e in entries}
    print('device time per entry point (event pairs around the launches, median of 10 calls, us): ' + ', '.join('%s %.1f' % (e[3:], med[e]) for e in entries))
    least = H * W * (3 + P)
    rate = least / med['mg_refine_apply'] / 1e3
    print('the full-size launch must move %.1f MB (the frame read once, %d planes written): %.0f GB/s at the measured time, %.1f %% of the %.0f GB/s HBM rate'
          % (least / 1e6, P, rate, 100 * rate / HBM_GBS, HBM_GBS))
    print('refine / reverse_transform_tensor: %.2f x the time' % (fast[0][0] / fast[2][0]))


if __name__ == '__main__':
    main()
