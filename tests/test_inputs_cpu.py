"""The input-side contract the device stages share (maggie_amd/utils/_inputs.py), without a GPU: the uint8 check, the shape checks, the draw
tables, the no-GPU error, and the order "argument errors before anything touches the device" at the stages' entry points. The message texts
are the ones the stages raised when each carried its own copy of these helpers."""
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from maggie_amd.hip import MaggieHipError                             # noqa: E402
from maggie_amd.utils import _inputs as I                             # noqa: E402
from maggie_amd.utils import affine, crop, maskgen, photometric, preprocess       # noqa: E402

NO_GPU = 'MaGGIe HIP kernels need a GPU; there is no CPU fallback'
NO_GPU_CPU_TENSOR = 'MaGGIe HIP kernels need a GPU (got a CPU tensor and no device); there is no CPU fallback'


def _raises(kind, text):
    return pytest.raises(kind, match='^' + re.escape(text) + '$')


def _no_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')


def test_uint8_check_on_arrays_tensors_and_other_types():
    a = np.arange(12, dtype=np.uint8).reshape(3, 4)[:, ::2]
    t = I.check_u8(a)
    assert t.dtype == torch.uint8 and t.is_contiguous() and np.array_equal(t.numpy(), a)
    x = torch.zeros((2, 2), dtype=torch.uint8)
    assert I.check_u8(x) is x
    with _raises(TypeError, 'expected uint8 planes, got int32'):
        I.check_u8(np.zeros((2, 2), np.int32))
    with _raises(TypeError, 'expected uint8 planes, got torch.float32'):
        I.check_u8(torch.zeros((2, 2)))
    with _raises(TypeError, 'expected a uint8 tensor or array, got list'):
        I.check_u8([[0, 1]])
    with _raises(TypeError, 'expected uint8 pixels, got torch.int16'):         # the wording of preprocess: an array's dtype reads as torch's
        preprocess.normalize_frames(np.zeros((1, 2, 2, 3), np.int16))
    with _raises(TypeError, 'expected uint8 pixels, got torch.float32'):
        preprocess.scale_planes(torch.zeros((1, 1, 2, 2)))


def test_images_rank_and_channels():
    x, lead, n, H, W = I.images(np.zeros((2, 5, 4, 6, 3), np.uint8), 3, 'frames')
    assert (lead, n, H, W) == ((2, 5), 10, 4, 6) and tuple(x.shape) == (2, 5, 4, 6, 3)
    assert I.images(torch.zeros((4, 6), dtype=torch.uint8), 1, 'alphas')[1:] == ((), 1, 4, 6)
    with _raises(ValueError, 'frames: expected (..., H, W, 3) (got shape (4, 3))'):
        I.images(np.zeros((4, 3), np.uint8), 3, 'frames')
    with _raises(ValueError, 'alphas: expected (..., H, W) (got shape (4,))'):
        I.images(np.zeros((4,), np.uint8), 1, 'alphas')
    with _raises(ValueError, 'frames: frames must have 3 channels (got shape (2, 4, 4))'):
        I.images(np.zeros((2, 4, 4), np.uint8), 3, 'frames')
    with _raises(ValueError, 'masks: the source must have at least one pixel (got 0 x 4)'):
        I.images(np.zeros((2, 0, 4), np.uint8), 1, 'masks')
    with _raises(TypeError, 'expected uint8 planes, got float64'):
        I.images(np.zeros((2, 4, 4)), 1, 'masks')


def test_int_table_and_lut_table_reject_wrong_dtype_size_and_shape():
    with _raises(ValueError, 'CropDraws.window must hold 3 ints (got int32 (4,))'):
        I.int_table(np.zeros((4,), np.int32), 'cpu', 3, 'CropDraws.window')
    with _raises(ValueError, 'CropDraws.window must hold 3 ints (got float64 (3,))'):
        I.int_table(np.zeros((3,)), 'cpu', 3, 'CropDraws.window')
    with _raises(ValueError, 'minmax must be int32 with 4 entries (got torch.int64 (2, 2))'):
        I.int_table(torch.zeros((2, 2), dtype=torch.int64), 'cpu', 4, 'minmax')
    with _raises(ValueError, 'minmax must be int32 with 4 entries (got torch.int32 (3, 2))'):
        I.int_table(torch.zeros((3, 2), dtype=torch.int32), 'cpu', 4, 'minmax')
    with pytest.raises(MaggieHipError):                                        # a table that is a tensor must live on the device already
        I.int_table(torch.zeros((4,), dtype=torch.int32), 'cpu', 4, 'minmax')
    t = I.int_table(np.arange(6, dtype=np.int64).reshape(2, 3)[:, ::-1], 'cpu', 6, 'a table')         # an array is converted and uploaded
    assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == [[2, 1, 0], [5, 4, 3]]
    good = np.zeros((3, 256), np.uint8)
    assert I.lut_table(None) is None and I.lut_table(None, 'cpu') is None and I.lut_table(good) is good
    assert torch.equal(I.lut_table(good, 'cpu'), torch.zeros((3, 256), dtype=torch.uint8))
    for bad, got in ((np.zeros((3, 256), np.int32), 'int32 (3, 256)'), (np.zeros((256, 3), np.uint8), 'uint8 (256, 3)'),
                     (torch.zeros((3, 256), dtype=torch.int16), 'torch.int16 (3, 256)'), (torch.zeros((3, 255), dtype=torch.uint8), 'torch.uint8 (3, 255)')):
        for device in (None, 'cpu'):
            with _raises(ValueError, 'lut must be uint8 of shape (3, 256) (got %s)' % got):
                I.lut_table(bad, device)
        with _raises(ValueError, 'lut must be uint8 of shape (3, 256) (got %s)' % got):
            photometric.PhotoDraws(lut=bad)
    assert [v for v in I.float3((0.5, 0.25, 2.0))] == [0.5, 0.25, 2.0]
    assert I.upload(None, 'cpu') is None and I.upload(np.arange(4)[::2], 'cpu').tolist() == [0, 2]
    assert preprocess.IMAGENET_MEAN is I.IMAGENET_MEAN and preprocess.IMAGENET_STD is I.IMAGENET_STD
    assert photometric.IMAGENET_MEAN == (0.485, 0.456, 0.406) and crop.IMAGENET_STD == (0.229, 0.224, 0.225)


def _draws():
    cd = crop.draw(np.random.RandomState(1), 32, 48, (16, 16), 0.0, 0.5, lambda: (0, 48, -1, 32, -1), lambda w: None)
    ad = affine.from_matrix([[1., 0., 0.5], [0., 1., 0.5]], 32, 48, 1.5)
    pd = photometric.PhotoDraws(np.zeros((3, 256), np.uint8), np.zeros((32, 48, 1), np.int16), 50)
    md = maskgen.draw_chain(np.random.RandomState(1), random.Random(1), 2, 32, 48)
    return cd, ad, pd, md


def test_no_gpu_is_a_maggie_error_not_a_torch_error():
    _no_gpu()
    with _raises(MaggieHipError, NO_GPU):
        I.resolve_device()
    for device in ('cuda', 'cuda:0', torch.device('cuda', 0)):
        with _raises(MaggieHipError, NO_GPU):
            I.resolve_device(device)
        with _raises(MaggieHipError, NO_GPU):
            I.resolve_device(device, like=torch.zeros(1))
    for device in (None, 'cuda', 'cuda:0'):
        with _raises(MaggieHipError, NO_GPU_CPU_TENSOR):
            I.to_device(torch.zeros((2, 2), dtype=torch.uint8), device)
    for draws in _draws():
        for device in (None, 'cuda', 'cuda:0'):
            with _raises(MaggieHipError, NO_GPU):
                draws.to(device)
    for fn in (lambda: preprocess.normalize_frames(np.zeros((1, 2, 2, 3), np.uint8)), lambda: preprocess.scale_planes(np.zeros((1, 1, 2, 2), np.uint8))):
        with _raises(MaggieHipError, NO_GPU):
            fn()


def test_argument_errors_of_the_stages_arrive_before_the_no_gpu_error():
    _no_gpu()
    cd, ad, pd, md = _draws()
    f, a = np.zeros((1, 32, 48, 3), np.uint8), np.zeros((2, 32, 48), np.uint8)
    # the good calls get as far as the device ...
    for fn in (lambda: crop.apply(f, a, a, cd), lambda: affine.apply(f, a, ad), lambda: photometric.apply(f, pd), lambda: maskgen.synthesize(a, md)):
        with _raises(MaggieHipError, NO_GPU_CPU_TENSOR):
            fn()
    # ... and every argument error comes first
    with _raises(TypeError, 'draws must be a CropDraws (got AffineDraws)'):
        crop.apply(f, a, a, ad)
    with _raises(ValueError, 'the draws were made for 32 x 48 arrays (got frames of 48 x 32)'):
        crop.apply(f.reshape(1, 48, 32, 3), a, None, cd)
    with _raises(ValueError, 'masks: expected 32 x 48 like the frames (got 16 x 48)'):
        crop.apply(f, a, a[:, :16], cd)
    with _raises(ValueError, 'lut must be uint8 of shape (3, 256) (got int64 (3, 256))'):
        crop.apply(f, a, None, cd, lut=np.zeros((3, 256), np.int64))
    with _raises(TypeError, 'expected uint8 planes, got float32'):
        crop.apply(f.astype(np.float32), a, None, cd)
    with _raises(TypeError, 'draws must be an AffineDraws (got CropDraws)'):
        affine.apply(f, a, cd)
    with _raises(ValueError, 'the draws did not fire: the item takes the path without RandomAffine'):
        affine.apply(f, a, affine.AffineDraws(False, 32, 48))
    with _raises(ValueError, 'alphas: expected 32 x 48 like the frames (got 16 x 48)'):
        affine.apply(f, a[:, :16], ad)
    with _raises(ValueError, 'frames: frames must have 3 channels (got shape (2, 32, 48))'):
        affine.apply(a, None, ad)
    with _raises(TypeError, 'draws must be a PhotoDraws (got MaskDraws)'):
        photometric.apply(f, md)
    with _raises(ValueError, 'the noise was drawn for 32 x 48 frames (got frames of 16 x 48)'):
        photometric.apply(f[:, :16], pd)
    with _raises(ValueError, 'frames: expected (..., H, W, 3) (got shape (48, 3))'):
        photometric.apply(f[0, 0], pd)
    with _raises(TypeError, 'draws must be a MaskDraws (got PhotoDraws)'):
        maskgen.synthesize(a, pd)
    with _raises(ValueError, 'the draws were made for 2 planes of 32 x 48 (got 3 of 32 x 48)'):
        maskgen.synthesize(np.zeros((3, 32, 48), np.uint8), md)
    with _raises(TypeError, 'expected uint8 planes, got int16'):
        maskgen.synthesize(a.astype(np.int16), md)
    with _raises(ValueError, 'expected (..., H, W) planes (got shape (48,))'):
        maskgen.synthesize(a[0, 0], md)
