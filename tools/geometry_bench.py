"""Device time of the input geometry (maggie_amd.utils.geometry, csrc/geometry.hip) for one evaluation item at two sizes: a realistic one,
1365 x 2048 -> short 768 (768 x 1152, a 1.78x reduction: the shared-rows regime) and a large reduction, 3000 x 4000 -> short 768 (768 x 1024,
3.9x: the direct regime), one frame and 4 instance planes, warm, tables resident, every call bracketed by its own event pair.
Timed: `eval_item`'s image path (resize + pad + normalise fused) in the host's regime and, where legal, in the other one; each
epilogue on its own (raw uint8 frames, raw alpha planes, alphas to fp32 slots, masks through the composed 1/8 index map).
Beside them the two yardsticks that predate this code:
  * the traffic bound: (bytes the launch must read + bytes it writes) / the HBM bandwidth a float4 copy reaches on this part;
  * `normalize_frames` alone at the output size: the floor the fused frame path cannot beat (it writes the same fp32 tensor).
No pass or fail on time. Every timed step runs in a child process under its own time limit.
usage: python tools/geometry_bench.py [reps]          (python tools/geometry_bench.py --one SIZE STEP reps: one step, in-process)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29            # measured float4 copy bandwidth of an MI355X (8.0 TB/s on paper)
SIZES = {'1365x2048': (1365, 2048), '3000x4000': (3000, 4000)}
N_INST = 4
STEPS = ('image', 'image_other_regime', 'raw_frames', 'raw_alphas', 'alpha_slots', 'mask_down8', 'normalize_frames_alone')
STEP_LIMIT = 120               # seconds per timed step


def one(size, step, reps):
    import numpy as np
    import torch
    from _timing import timed
    from maggie_amd.utils import geometry as GE
    from maggie_amd.utils.preprocess import normalize_frames
    dev = torch.device('cuda:0')
    h, w = SIZES[size]
    p = GE.plan(h, w, 768, 64)
    rs = np.random.RandomState(0)
    frames = torch.from_numpy(rs.randint(0, 256, size=(1, h, w, 3)).astype(np.uint8)).to(dev)
    planes = torch.from_numpy(rs.randint(0, 256, size=(1, N_INST, h, w)).astype(np.uint8)).to(dev)
    out_px, src_px = p.out_h * p.out_w, h * w
    other = 'direct' if p.tables['regime'] == GE.SHARED_ROWS else ('shared' if p.tables['rows_read'] <= GE.MAX_ROWS else None)
    # bytes a launch must move: sources are read once at reductions under 2x; beyond, only the rows and columns the taps name
    fx, fy = min(1.0, 2.0 * p.rw / w), min(1.0, 2.0 * p.rh / h)
    if step == 'image':
        fn, moved = (lambda: GE.resize_pad_normalize(frames, p)), src_px * 3 * fx * fy + out_px * 12
    elif step == 'image_other_regime':
        if other is None:
            return {'skipped': 'the shared-rows regime is not legal at this ratio'}
        fn, moved = (lambda: GE.resize_pad_normalize(frames, p, regime=other)), src_px * 3 * fx * fy + out_px * 12
    elif step == 'raw_frames':
        fn, moved = (lambda: GE.resize_short_pad(frames, short_size=p)), src_px * 3 * fx * fy + out_px * 3
    elif step == 'raw_alphas':
        fn, moved = (lambda: GE.resize_pad_planes_u8(planes, p)), N_INST * (src_px * fx * fy + out_px)
    elif step == 'alpha_slots':
        fn, moved = (lambda: GE.resize_pad_planes(planes, p, thresh=5)), N_INST * (src_px * fx * fy + out_px * 4)
    elif step == 'mask_down8':
        fn, moved = (lambda: GE.resize_pad_planes(planes, p, interpolation='nearest', down8=True)), N_INST * (out_px // 64) * 5
    else:
        padded = torch.from_numpy(rs.randint(0, 256, size=(1, p.out_h, p.out_w, 3)).astype(np.uint8)).to(dev)
        fn, moved = (lambda: normalize_frames(padded)), out_px * 15
    median, fastest = timed([fn], reps)[0][:2]
    return {'median_us': median, 'min_us': fastest, 'bytes': float(moved), 'bound_us': moved / (HBM_COPY_TBS * 1e12) * 1e6,
            'regime': 'shared' if p.tables['regime'] == GE.SHARED_ROWS else 'direct', 'out': [p.out_h, p.out_w]}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--one':
        print('RESULT ' + json.dumps(one(sys.argv[2], sys.argv[3], int(sys.argv[4]))))
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    print('%-22s %-24s %10s %10s %10s %8s %9s' % ('size (%d calls each)' % reps, 'step', 'median us', 'min us', 'bound us', 'x bound', 'x normalize'))
    for size in SIZES:
        rows = {}
        for step in STEPS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--one', size, step, str(reps)], capture_output=True, text=True,
                                   timeout=STEP_LIMIT)
            except subprocess.TimeoutExpired:
                print('%-22s %-24s exceeded its %d s limit: stopping' % (size, step, STEP_LIMIT))
                sys.exit(3)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                print('%-22s %-24s failed with status %d: stopping' % (size, step, r.returncode))
                sys.exit(4)                                                # nothing more is started on the device after a failed step
            rows[step] = json.loads(line[0][7:])
        floor = rows['normalize_frames_alone']['median_us']
        for step in STEPS:
            r = rows[step]
            if 'skipped' in r:
                print('%-22s %-24s %s' % (size, step, r['skipped']))
                continue
            vs = ('%9.2f' % (r['median_us'] / floor)) if step.startswith('image') else ''
            print('%-22s %-24s %10.1f %10.1f %10.1f %8.1f %s' % ('%s (%s)' % (size, r['regime']), step, r['median_us'], r['min_us'], r['bound_us'],
                                                               r['median_us'] / r['bound_us'], vs))


if __name__ == '__main__':
    main()
