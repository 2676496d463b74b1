"""Generate tests/golden/jpegprog_pinned.npz WITH PILLOW ITSELF:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpegprog_golden.py

For each case of PINNED (names of `jpegprog_restatement.CASES` / `RESTART`) the file holds the progressive JPEG stream Pillow wrote
(`<case>.stream`, uint8) and the pixels Pillow decodes from it (`<case>.pixels`, `Image.open(...).convert('RGB')`); `versions` records the
Pillow and libjpeg(-turbo) versions. The streams are data written by Pillow from seeded NumPy inputs. The generator asserts that the
restatement equals Pillow on every case."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import jpegprog_restatement as J                               # noqa: E402
from make_jpegdec_golden import versions                       # noqa: E402

# a dozen small streams: every layout, every quality of the list, odd sizes, and every restart form
PINNED = ['1x1_uniform_2_q1', '8x8_flat_L_q50', '9x4_uniform_0_q90', '17x23_binary_2_q100', '33x65_smooth_2_q50', '37x53_uniform_0_q90',
          '16x16_smooth_L_q90', '16x16_binary_L_q1', '37x53_uniform_2_q90_blocks1', '64x48_smooth_0_q50_rows1', '33x65_binary_L_q100_blocks1',
          '64x48_smooth_2_q50_rows1']


def main():
    out = {}
    for name in PINNED:
        data = J.named(name)
        y = J.pillow(data)
        assert np.array_equal(J.decode(data), y), '%s: the restatement differs from Pillow' % name
        out[name + '.stream'], out[name + '.pixels'] = np.frombuffer(data, np.uint8), y
    out['versions'] = np.asarray(versions())
    path = os.path.join(HERE, 'jpegprog_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 58 * 1024, size                              # the limit of make_jpegdec_golden.py
    print('wrote %s (%d bytes, %s)' % (path, size, out['versions']))


if __name__ == '__main__':
    main()
