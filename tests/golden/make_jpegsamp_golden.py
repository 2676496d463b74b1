"""Generate tests/golden/jpegsamp_pinned.npz WITH PILLOW ITSELF:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpegsamp_golden.py

For each case of PINNED (names of `jpegsamp_restatement.CASES`) the file holds the JPEG stream (`<case>.stream`, uint8: Pillow's own for the
4:2:2 cases, the writers' of tests/jpegsamp_restatement.py -- Pillow's coefficients recoded at another sampling -- for 4:4:0 and 4:1:1) and the
pixels Pillow decodes from it (`<case>.pixels`, `Image.open(...).convert('RGB')`); `versions` records the Pillow and libjpeg(-turbo) versions.
Data only. The generator asserts that the restatement equals Pillow on every case."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import jpegsamp_restatement as S                               # noqa: E402
from make_jpegdec_golden import versions                       # noqa: E402

# a dozen small streams: every sampling, baseline and progressive, every quality of the list, odd sizes, restart markers
PINNED = ['422_1x1_uniform_pillow_qua1', '422_8x17_binary_pillow_qua1', '422_17x23_flat_pillow_qua90', '422_37x53_uniform_pillow_qua90_rsb1',
          '422_23x17_smooth_pillow_proT_qua90', '422_37x53_uniform_pillow_proT_qua90_rsb1', '440_4x4_binary_base_qua90', '440_8x17_binary_base_qua1',
          '440_37x53_uniform_base_qua90_ri3', '440_17x23_flat_prog_qua100', '411_5x33_uniform_base_qua1', '411_37x53_uniform_base_qua90_ri1',
          '411_9x4_smooth_prog_qua90']


def main():
    out = {}
    for name in PINNED:
        data = S.stream(name)
        y = S.pillow(data)
        assert np.array_equal(S.decode(data), y), '%s: the restatement differs from Pillow' % name
        out[name + '.stream'], out[name + '.pixels'] = np.frombuffer(data, np.uint8), y
    out['versions'] = np.asarray(versions())
    path = os.path.join(HERE, 'jpegsamp_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 64 * 1024, size
    print('wrote %s (%d bytes, %s)' % (path, size, out['versions']))


if __name__ == '__main__':
    main()
