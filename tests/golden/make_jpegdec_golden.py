"""Generate tests/golden/jpegdec_pinned.npz WITH PILLOW ITSELF:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpegdec_golden.py

For each case of PINNED (names of `jpegdec_restatement.CASES`) the file holds the JPEG stream Pillow wrote (`<case>.stream`, uint8) and the
pixels Pillow decodes from it (`<case>.pixels`, `Image.open(...).convert('RGB')`); `versions` records the Pillow and libjpeg(-turbo) versions.
The streams are data written by Pillow from seeded NumPy inputs. The generator asserts that the restatement equals Pillow on every case."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import jpegdec_restatement as R                                # noqa: E402

# a dozen small streams: every layout, standard and optimised tables, every restart form, both extreme quantisation tables
PINNED = ['1x1_uniform_2_qua1', '8x8_flat_L_qua50', '9x4_uniform_0_qua90', '17x23_binary_2_qua100', '33x65_flat_2_qua50',
          '37x53_uniform_0_optT_qua90', '16x16_flat_L_optT_qua90', '37x53_uniform_2_qua90_res1', '16x16_flat_0_optT_qua50_res3',
          '64x48_smooth_2_qua50_res1', '33x65_binary_2_qta255', '33x65_binary_0_qta1']


def versions():
    import PIL
    from PIL import features
    return 'Pillow %s; libjpeg_turbo %s; jpg %s' % (PIL.__version__, features.version_feature('libjpeg_turbo'), features.version('jpg'))


def main():
    out = {}
    for name in PINNED:
        data = R.stream(*R.CASES[name])
        y = R.pillow(data)
        assert np.array_equal(R.decode(data), y), '%s: the restatement differs from Pillow' % name
        out[name + '.stream'], out[name + '.pixels'] = np.frombuffer(data, np.uint8), y
    out['versions'] = np.asarray(versions())
    path = os.path.join(HERE, 'jpegdec_pinned.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 58 * 1024, size
    print('wrote %s (%d bytes, %s)' % (path, size, out['versions']))


if __name__ == '__main__':
    main()
