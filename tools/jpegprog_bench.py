"""Time of the device progressive JPEG decode (maggie_amd.utils.jpegprog, csrc/jpegprog.hip) on one 1080 x 1920 file and on a clip of 24, at
quality 75 and 90, 4:2:0, written by Pillow with `progressive=True` from the smooth-plus-noise picture of tools/jpegdec_bench.py. Warm, every
call bracketed by its own event pair (host work of a call -- the marker walk, the upload, the read-back -- lies between its events too), the
candidates alternated call by call:
  * `jpegprog.decode_clip` from the files' bytes;
  * the parent's only way: `Image.open(...).convert("RGB")` per file on the host plus the host -> device copy;
  * for context, `jpegdec.decode_clip` on the baseline twins (the same pictures saved without `progressive`).
The tool first asserts that all three give the same bytes. Then the chain launch alone, and each kind of chain alone (DC, Y, Cb, Cr: one wave
per file each), with device buffers prepared outside the events: where the time of a call goes.
usage: python tools/jpegprog_bench.py [reps]"""
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageFile

from _timing import timed
from jpegdec_bench import picture
from maggie_amd.utils import jpegdec, jpegprog

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 24)          # a progressive file leaves the encoder in one piece


def jpeg(x, quality, progressive):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', quality=quality, subsampling=2, progressive=progressive)
    return buf.getvalue()


def pillow(datas):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas])).to(dev)


def chain_times(datas, reps):
    """Median microseconds of the chain launch alone: all chains, then the chains of one kind only."""
    plans = [jpegprog.parse(d) for d in datas]
    joined, scans, chains, _ = jpegprog.pack(plans, datas)
    h, w, layout = plans[0].geometry
    T = len(datas)
    blob = torch.frombuffer(bytearray(joined), dtype=torch.uint8).to(dev)
    d_scans = torch.from_numpy(scans).to(dev)
    coef = torch.zeros((T, jpegdec.geometry(h, w, layout)[0], 64), dtype=torch.int16, device=dev)
    info = torch.zeros((T,), dtype=torch.int32, device=dev)
    # a chain's kind from its first scan record: Ss == 0 is the DC chain, else the AC chain of component word 464
    kind = np.where(scans[chains[:, 1], 459] == 0, -1, scans[chains[:, 1], 464])
    subsets = [('all chains', chains)] + [(n, chains[kind == k]) for k, n in ((-1, 'DC'), (0, 'Y'), (1, 'Cb'), (2, 'Cr'))]

    def launch(d_chains):                                      # a chain needs nothing of another: an AC chain reads and writes its own band only
        def fn():
            coef.zero_()
            jpegprog.launch_chains(blob, d_scans, d_chains, coef, info, T, h, w, layout)
        return fn
    out = []
    for name, sub in subsets:
        res = timed([launch(torch.from_numpy(np.ascontiguousarray(sub)).to(dev))], reps, warmup=3)[0]
        out.append((name, len(sub), sum(int(scans[a:a + n, 457].sum()) for _, a, n, _ in sub), res[0]))
    assert int(info.sum()) == 0
    return out


def main():
    rs = np.random.RandomState(0)
    single = picture(rs, 1080, 1920)
    clip = [picture(rs, 1080, 1920, t) for t in range(24)]
    print('%-118s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'median us', 'min us', 'p25 us', 'p75 us'))
    for q in (75, 90):
        for name, xs in (('one 1080 x 1920 file', [single]), ('a clip of 24 files, 1080 x 1920', clip)):
            prog, base = [jpeg(x, q, True) for x in xs], [jpeg(x, q, False) for x in xs]
            want = pillow(prog)
            assert torch.equal(jpegprog.decode_clip(prog), want) and torch.equal(jpegdec.decode_clip(base), want)
            fns = [lambda d=prog: jpegprog.decode_clip(d), lambda d=prog: pillow(d), lambda d=base: jpegdec.decode_clip(d), lambda d=base: pillow(d)]
            r = jpegprog.decode_stats(prog)
            names = ['%s, quality %d (%d KB progressive): jpegprog.decode_clip; %d chains, %d launches, %d read-back' %
                     (name, q, sum(len(d) for d in prog) >> 10, r.chains, r.launches, r.readbacks),
                     '  parent: Image.open().convert("RGB") of the progressive files on the host, host -> device',
                     '  context: jpegdec.decode_clip of the baseline twins (%d KB)' % (sum(len(d) for d in base) >> 10),
                     '  context: Image.open().convert("RGB") of the baseline twins on the host, host -> device']
            for n, (med, mn, lo, hi) in zip(names, timed(fns, REPS, warmup=3)):
                print('%-118s %10.1f %10.1f %10.1f %10.1f' % (n, med, mn, lo, hi))
            print('  the chain launch alone (median us): ' + '; '.join('%s: %d waves, %d KB, %.1f' % (n, c, b >> 10, t)
                                                                        for n, c, b, t in chain_times(prog, max(5, REPS // 4))))


if __name__ == '__main__':
    main()
