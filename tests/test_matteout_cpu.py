"""What the GPU tests of maggie_amd/utils/matteout.py rest on, checked without a GPU: the overlay restatement against Pillow itself, the
condition that the composite grid tells a contracted evaluation from the reference's, and the argument checks of every public function."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import matteout_restatement as R                                      # noqa: E402
from maggie_amd import hip                                            # noqa: E402
from maggie_amd.utils import matteout                                 # noqa: E402

BLEND_ALPHAS = (0.5, 0.25, 0.3, 0.7, 0.1, 0.9, 1.0 / 3.0, 0.0, 1.0)


def all_pairs():
    """(image (256, 256, 3), masks): every (in1, in2) byte pair appears -- channel 0 runs in1 across against the colour 255 and against 0, channels
    1 and 2 against colours that run down the rows are made by the callers through `colour`."""
    v = np.arange(256, dtype=np.uint8)
    return np.broadcast_to(v[None, :, None], (256, 256, 3)).copy()


@pytest.mark.parametrize('alpha', BLEND_ALPHAS)
def test_overlay_restatement_is_pillows_blend_for_all_byte_pairs(alpha):
    image = all_pairs()
    on = np.full((256, 256), 255, np.uint8)
    on[::2, ::3] = 1                                                       # any value > 0 counts
    for c in range(0, 256, 3):                                             # the colour's three channels cover in2 = c, c + 1, c + 2; mask on
        colour = (c, min(c + 1, 255), min(c + 2, 255))
        assert np.array_equal(R.overlay(image, on, colour, alpha), R.pillow_overlay(image, on, colour, alpha)), (alpha, colour)
    off = np.zeros((256, 256), np.uint8)                                   # mask off: in2 = 0
    assert np.array_equal(R.overlay(image, off, (255, 0, 255), alpha), R.pillow_overlay(image, off, (255, 0, 255), alpha)), alpha
    mixed = (np.arange(256 * 256).reshape(256, 256) % 5 == 0).astype(np.uint8) * 7
    assert np.array_equal(R.overlay(image, mixed, (255, 0, 255), alpha), R.pillow_overlay(image, mixed, (255, 0, 255), alpha)), alpha


def test_grid_tells_the_contracted_forms_from_the_reference():
    """A condition on the INPUT of the GPU tests: for the background bytes 255, 99 and 203 each of the four wrong evaluations differs from the
    restatement in at least one byte of the grid, so a kernel that contracts (or tidies the algebra, or widens to fp64) cannot pass."""
    image, alpha = R.grid()
    assert image.shape == (R.GRID_ROWS + 6, 256, 3) and alpha.dtype == np.float32
    for ch in range(3):
        assert sorted(set(image[0, :, ch].tolist())) == list(range(256)), ch
    for bg, channels in (((0, 255, 0), {1: 255}), ((255, 255, 255), {0: 255, 1: 255, 2: 255}), ((17, 99, 203), {1: 99, 2: 203})):
        want = R.composite(image, alpha, bg)
        for name, got in R.wrong_forms(image, alpha, bg).items():
            for ch, byte in channels.items():
                n = int((got[:, :, ch] != want[:, :, ch]).sum())
                print('background %3d, channel %d, %-20s: %d of %d bytes differ' % (byte, ch, name, n, want[:, :, ch].size))
                assert n >= 1, (bg, ch, name)
    # background 0 cannot discriminate (t2 is 0 and the sum exact): stated, so that nobody leans on that channel
    want = R.composite(image, alpha, (0, 255, 0))
    for name, got in R.wrong_forms(image, alpha, (0, 255, 0)).items():
        if name != 'fp64':
            assert np.array_equal(got[:, :, 0], want[:, :, 0]), name
    # the special alphas: 0 and 1 give the background and the image themselves
    rows = R.GRID_ROWS
    assert np.array_equal(want[rows], R.background_of((0, 255, 0), image.shape)[rows]) and np.array_equal(want[rows + 1], image[rows + 1])
    # 255 * a + (1 - a) * 255 never reaches 256
    a = alpha[:, :1]
    assert float((np.float32(255) * a + (1 - a) * np.float32(255)).max()) < 256.0


def test_restated_label_split_and_writer_loop():
    m = np.zeros((5, 7), np.int32)
    m[1:3, 2:5], m[4, 0], m[0, 6] = 7, 255, 3
    ids, planes = R.label_planes(m)
    assert ids == [3, 7, 255] and planes.shape == (3, 5, 7) and planes.dtype == np.uint8
    assert planes[1].sum() == 255 * 6 and planes[0, 0, 6] == 255 and planes[2, 4, 0] == 255
    ids, planes = R.label_planes(np.zeros((2, 3), np.uint8))
    assert ids == [] and planes.shape == (0, 2, 3)
    # four clips of frames (0 1 2) (1 2 3) (2 3 4) (3 4 5): frame 0 is saved twice, then 1, and the last push saves what is stored
    rs = np.random.RandomState(0)
    frames = rs.randint(0, 256, size=(6, 4, 5, 3)).astype(np.uint8)
    pushes = [(rs.random_sample((3, 2, 4, 5)).astype(np.float32), frames[c:c + 3], ['d/f%d.jpg' % k for k in range(c, c + 3)], c == 0, c == 3)
              for c in range(4)]
    written = R.writer_loop(pushes, 'out')
    names = [[os.path.basename(p) for p, _ in w] for w in written]
    assert names[0] == ['00_f0.jpg', '01_f0.jpg'] and names[1] == names[0] and names[2] == ['00_f1.jpg', '01_f1.jpg']
    assert names[3] == ['%02d_f%d.jpg' % (i, k) for k in (2, 3, 4, 5) for i in range(2)]
    assert np.array_equal(written[3][2][1], R.composite(frames[3], pushes[2][0][1][0]))          # frame 3 is kept as frame t of clip 2, not as t+1 of clip 1


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
F = np.zeros((4, 6, 3), np.uint8)
A = torch.zeros((2, 4, 6))
NO_GPU = not torch.cuda.is_available()


def _no_device_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('an argument error must be raised before anything touches the device')
    monkeypatch.setattr(hip, 'call', boom)
    monkeypatch.setattr(matteout, 'to_device', boom)


BAD = {
    'composite: float frames': (TypeError, lambda: matteout.composite(F.astype(np.float32), A)),
    'composite: frames of 4 channels': (ValueError, lambda: matteout.composite(np.zeros((4, 6, 4), np.uint8), A)),
    'composite: 5-d frames': (ValueError, lambda: matteout.composite(np.zeros((1, 1, 4, 6, 3), np.uint8), A)),
    'composite: alpha an array': (TypeError, lambda: matteout.composite(F, A.numpy())),
    'composite: alpha fp64': (TypeError, lambda: matteout.composite(F, A.double())),
    'composite: alpha 2-d': (ValueError, lambda: matteout.composite(F, A[0])),
    'composite: planes do not divide': (ValueError, lambda: matteout.composite(np.zeros((3, 4, 6, 3), np.uint8), torch.zeros((2, 2, 4, 6)))),
    'composite: size without transform': (ValueError, lambda: matteout.composite(F, torch.zeros((2, 8, 8)))),
    'composite: size with transform': (ValueError, lambda: matteout.composite(F, torch.zeros((2, 8, 8)), transform_info=[{'name': 'resize', 'ori_size': (5, 6)}])),
    'composite: padding eats the plane': (ValueError, lambda: matteout.composite(F, A, transform_info=[{'name': 'padding', 'pad_size': (4, 0)}])),
    'composite: colour of two': (ValueError, lambda: matteout.composite(F, A, (0, 255))),
    'composite: colour 256': (ValueError, lambda: matteout.composite(F, A, (0, 256, 0))),
    'composite: colour of floats': (TypeError, lambda: matteout.composite(F, A, (0.0, 1.0, 0.0))),
    'composite: background of another size': (ValueError, lambda: matteout.composite(F, A, np.zeros((4, 7, 3), np.uint8))),
    'composite: background of two frames for one': (ValueError, lambda: matteout.composite(F, A, np.zeros((2, 4, 6, 3), np.uint8))),
    'composite: float background': (TypeError, lambda: matteout.composite(F, A, np.zeros((4, 6, 3), np.float32))),
    'overlay: int32 masks': (TypeError, lambda: matteout.overlay(F, np.zeros((4, 6), np.int32))),
    'overlay: masks of another size': (ValueError, lambda: matteout.overlay(F, np.zeros((4, 7), np.uint8))),
    'overlay: alpha 1.5': (ValueError, lambda: matteout.overlay(F, np.zeros((4, 6), np.uint8), alpha=1.5)),
    'overlay: alpha nan': (ValueError, lambda: matteout.overlay(F, np.zeros((4, 6), np.uint8), alpha=float('nan'))),
    'overlay: alpha a string': (TypeError, lambda: matteout.overlay(F, np.zeros((4, 6), np.uint8), alpha='0.5')),
    'overlay: colour -1': (ValueError, lambda: matteout.overlay(F, np.zeros((4, 6), np.uint8), (-1, 0, 0))),
    'label_planes: int64': (TypeError, lambda: matteout.label_planes(np.zeros((4, 6), np.int64))),
    'label_planes: a list': (TypeError, lambda: matteout.label_planes([[0, 1]])),
    'label_planes: 3-d': (ValueError, lambda: matteout.label_planes(np.zeros((1, 4, 6), np.uint8))),
    'predict_image: frame 4-d': (ValueError, lambda: matteout.predict_image(None, F[None], np.zeros((4, 6), np.uint8))),
    'predict_image: instances a list': (TypeError, lambda: matteout.predict_image(None, F, [[0]])),
    'predict_image: label map of another size': (ValueError, lambda: matteout.predict_image(None, F, np.zeros((4, 7), np.uint8))),
    'predict_image: planes of another size': (ValueError, lambda: matteout.predict_image(None, F, np.zeros((2, 4, 7), np.uint8))),
    'predict_image: float planes': (TypeError, lambda: matteout.predict_image(None, F, np.zeros((2, 4, 6), np.float32))),
    'save_composites: 3-d': (ValueError, lambda: matteout.save_composites(F, 'out', 'x')),
    'save_composites: float': (TypeError, lambda: matteout.save_composites(F[None].astype(np.float32), 'out', 'x')),
    'save_overlay: names do not match': (ValueError, lambda: matteout.save_overlay(F, 'out', ['a', 'b'])),
    'save_overlay: float': (TypeError, lambda: matteout.save_overlay(F.astype(np.float32), 'out', 'a')),
    'writer: colour': (ValueError, lambda: matteout.VideoMatteWriter('out', background=(0, 0))),
    'writer: alpha clip 4-d': (ValueError, lambda: matteout.VideoMatteWriter('out').push(torch.zeros((3, 2, 4, 6)), [], np.zeros((3, 4, 6, 3), np.uint8),
                                                                                        ['a', 'b', 'c'], True, True)),
    'writer: two names for three frames': (ValueError, lambda: matteout.VideoMatteWriter('out').push(torch.zeros((1, 3, 2, 4, 6)), [], np.zeros((3, 4, 6, 3), np.uint8),
                                                                                                    ['a', 'b'], True, True)),
    'writer: a name that is no string': (TypeError, lambda: matteout.VideoMatteWriter('out').push(torch.zeros((1, 3, 2, 4, 6)), [], np.zeros((3, 4, 6, 3), np.uint8),
                                                                                                  ['a', 'b', 3], True, True)),
}


@pytest.mark.parametrize('case', sorted(BAD))
def test_argument_errors_come_before_any_device_call(case, monkeypatch):
    _no_device_call(monkeypatch)
    exc, fn = BAD[case]
    with pytest.raises(exc):
        fn()


GOOD = {
    'composite': lambda: matteout.composite(F, A),
    'composite with transform_info': lambda: matteout.composite(F, torch.zeros((2, 8, 8)), transform_info=[{'name': 'resize', 'ori_size': (4, 6)},
                                                                                                         {'name': 'padding', 'pad_size': (2, 0)}]),
    'overlay': lambda: matteout.overlay(F, np.zeros((4, 6), np.uint8)),
    'label_planes': lambda: matteout.label_planes(np.zeros((4, 6), np.uint8)),
    'predict_image from a label map': lambda: matteout.predict_image(lambda b: b, F, np.ones((4, 6), np.uint8)),
    'predict_image from planes': lambda: matteout.predict_image(lambda b: b, F, np.zeros((1, 4, 6), np.uint8)),
    'save_composites': lambda: matteout.save_composites(F[None], 'never_written', 'x'),
    'save_overlay': lambda: matteout.save_overlay(F, 'never_written', 'x'),
    'writer': lambda: matteout.VideoMatteWriter('never_written').push(torch.zeros((1, 3, 2, 4, 6)), [], np.zeros((3, 4, 6, 3), np.uint8),
                                                                      ['a.jpg', 'b.jpg', 'c.jpg'], True, True),
}


@pytest.mark.skipif(not NO_GPU, reason='with a GPU these calls succeed: tests/test_gpu_matteout.py')
@pytest.mark.parametrize('case', sorted(GOOD))
def test_without_a_gpu_every_function_raises_the_products_error(case):
    with pytest.raises(hip.MaggieHipError):
        GOOD[case]()
    assert not os.path.exists('never_written')
