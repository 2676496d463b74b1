"""Writes tests/golden/pngdec_pinned.npz: the Pillow-written files of tests/pngdec_restatement.py `pillow_cases` (`file_<name>`, the bytes) and
what `Image.open(...).convert("L")` returned for each when the fixture was made (`l_<name>`). Pillow 12.2.0 wrote it."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pngdec_restatement as R                              # noqa: E402

if __name__ == '__main__':
    out = {}
    for name, data in R.pillow_cases().items():
        out['file_' + name] = np.frombuffer(data, np.uint8)
        out['l_' + name] = R.pillow(data)
    path = os.path.join(HERE, 'pngdec_pinned.npz')
    np.savez_compressed(path, **out)
    print(path, len(out) // 2, 'files', os.path.getsize(path), 'bytes')
