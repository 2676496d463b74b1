"""The timing harness of the stage benches (crop, affine, maskgen, photometric, geometry, groundtruth): every call bracketed by its own event
pair, the candidates alternated call by call after a warm-up."""
import numpy as np
import torch


def timed(fns, reps, warmup=10):
    """Per callable (median, minimum, p25, p75) -- the quartiles are the run-to-run spread -- of the microseconds between the event pair
    around every call. Host work a callable does lies between its events too."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b) * 1e3)
    return [(float(np.median(t)), float(np.min(t)), float(np.percentile(t, 25)), float(np.percentile(t, 75))) for t in ts]
