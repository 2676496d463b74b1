"""Time of the device decode of the other chroma samplings (maggie_amd.utils.jpegsamp) on one 1080 x 1920 file and on a clip of 24, at quality
75 and 90, from the smooth-plus-noise picture of tools/jpegdec_bench.py: 4:2:2 baseline and 4:2:2 progressive written by Pillow, 4:4:0 baseline
written by the writer of tests/jpegsamp_restatement.py (Pillow writes no 4:4:0; the writer is plain Python, so the 4:4:0 clip cycles four files).
Warm, every call bracketed by its own event pair (the marker walk, the upload and the read-back of a call lie between its events too), the
candidates alternated call by call:
  * `jpegsamp.decode_clip` from the files' bytes;
  * the parent's only way: `Image.open(...).convert("RGB")` per file on the host plus the host -> device copy, same machine, same files;
  * the yardstick: `jpegdec.decode_clip` / `jpegprog.decode_clip` on the 4:2:0 files of the same pictures, quality and kind -- the same entropy
    kernels, so the time per coded byte should match; the inverse transform and the colour kernel move 2 bytes per pixel in where 4:2:0 moves 1.5.
The tool first asserts that the device and Pillow give the same bytes.
usage: python tools/jpegsamp_bench.py [reps]"""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch
from PIL import Image, ImageFile

import jpegsamp_restatement as S
from _timing import timed
from jpegdec_bench import picture
from maggie_amd.utils import jpegdec, jpegprog, jpegsamp

dev = torch.device('cuda:0')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 24)          # a progressive file leaves the encoder in one piece


def jpeg(x, quality, subsampling, progressive=False):
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', quality=quality, subsampling=subsampling, progressive=progressive)
    return buf.getvalue()


def pillow(datas):
    return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(d)).convert('RGB')) for d in datas])).to(dev)


def main():
    rs = np.random.RandomState(0)
    single = picture(rs, 1080, 1920)
    clip = [picture(rs, 1080, 1920, t) for t in range(24)]
    print('%-112s %8s %10s %10s %10s %10s' % ('workload (%d calls each)' % REPS, 'KB', 'median us', 'min us', 'p25 us', 'us / KB'))
    for q in (75, 90):
        for name, xs in (('one file', [single]), ('clip of 24', clip)):
            forms = (('4:2:2 baseline', [jpeg(x, q, 1) for x in xs], [jpeg(x, q, 2) for x in xs], jpegdec),
                     ('4:2:2 progressive', [jpeg(x, q, 1, True) for x in xs], [jpeg(x, q, 2, True) for x in xs], jpegprog),
                     ('4:4:0 baseline', [S.write_baseline(x, 1, 2, quality=q) for x in xs[:4]] * (len(xs) // min(len(xs), 4)),
                      [jpeg(x, q, 2) for x in xs], jpegdec))
            for form, files, yard, mod in forms:
                assert torch.equal(jpegsamp.decode_clip(files), pillow(files)) and torch.equal(mod.decode_clip(yard), pillow(yard))
                fns = [lambda d=files: jpegsamp.decode_clip(d), lambda d=files: pillow(d), lambda d=yard, m=mod: m.decode_clip(d)]
                names = ['%s, 1080 x 1920, quality %d, %s: jpegsamp.decode_clip' % (name, q, form),
                         '  parent: Image.open().convert("RGB") of the same files on the host, host -> device',
                         '  yardstick: %s.decode_clip of the 4:2:0 files of the same pictures' % mod.__name__.rsplit('.', 1)[1]]
                sizes = [sum(len(d) for d in files) / 1024.0] * 2 + [sum(len(d) for d in yard) / 1024.0]
                for n, kb, (med, mn, lo, hi) in zip(names, sizes, timed(fns, REPS, warmup=3)):
                    print('%-112s %8.0f %10.1f %10.1f %10.1f %10.2f' % (n, kb, med, mn, lo, med / kb))
                if mod is jpegdec:                             # the synchronisation of the two baseline decodes: where their times differ
                    a, b = jpegsamp.decode_stats(files), jpegdec.decode_stats(yard)
                    print('  synchronisation: jpegsamp %d subsequences, %d rounds, %d launches, %d read-backs; yardstick %d, %d, %d, %d' %
                          (a.subsequences, a.rounds, a.launches, a.readbacks, b.subsequences, b.rounds, b.launches, b.readbacks))


if __name__ == '__main__':
    main()
