"""Generate tests/golden/jpegenc_pinned.npz WITH PILLOW ITSELF:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_jpegenc_golden.py

For each case of PINNED (names of `jpegenc_restatement.CASES`, plus two table cases) the file holds the input frame (`<case>.frame`, uint8
(h, w, 3)), the quality or the (2, 64) table (`<case>.quality`) and the bytes Pillow wrote for it (`<case>.file`, uint8: the whole file of
`Image.fromarray(frame).save(buf, 'JPEG', quality=q)`); `versions` records the Pillow and libjpeg(-turbo) versions. The inputs are seeded NumPy
arrays, the files data written by Pillow. The generator asserts that the restatement equals Pillow on every case."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import jpegenc_restatement as R                                # noqa: E402

# ten small inputs: the 1 x 1 file, every combination of a dummy column / row, an exact MCU, sizes past one kernel tile, the crafted inputs with
# their stuffed bytes, both extreme quantisation tables
PINNED = ['1x1_random_q75', '8x8_binary_q100', '9x4_smooth_q21', '17x23_random_q50', '16x16_binary_q1', '33x65_random_q80', '37x53_smooth_q75',
          '48x48_blocks_q100', '48x48_checker_q75']
TABLES = {'33x65_binary_t1': (33, 65, 'binary', [[1] * 64] * 2), '33x65_binary_t255': (33, 65, 'binary', [[255] * 64] * 2)}


def versions():
    import PIL
    from PIL import features
    return 'Pillow %s; libjpeg_turbo %s; jpg %s' % (PIL.__version__, features.version_feature('libjpeg_turbo'), features.version('jpg'))


def pinned_cases():
    """name -> (frame, quality or table)"""
    out = {}
    for name in PINNED:
        h, w, kind, q, seed = R.CASES[name]
        out[name] = (R.image(h, w, kind, seed), q)
    for name, (h, w, kind, t) in TABLES.items():
        out[name] = (R.image(h, w, kind, 100 * h + w), np.asarray(t, np.int32))
    return out


def main():
    out = {}
    for name, (x, q) in pinned_cases().items():
        data = R.pillow(x, q)
        assert R.file_bytes(x, q) == data, '%s: the restatement differs from Pillow' % name
        out[name + '.frame'], out[name + '.quality'], out[name + '.file'] = x, np.asarray(q, np.int32), np.frombuffer(data, np.uint8)
    out['versions'] = np.asarray(versions())
    path = os.path.join(HERE, 'jpegenc_pinned.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d bytes, %s' % (path, os.path.getsize(path), out['versions']))


if __name__ == '__main__':
    main()
