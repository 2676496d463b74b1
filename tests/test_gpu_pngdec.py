"""The device PNG decoder (maggie_amd.utils.pngdec, csrc/pngdec.hip) against zlib and live Pillow, which tests/test_pngdec_cpu.py holds equal to
the sequential restatement of tests/pngdec_restatement.py: the inflated bytes first, then the L plane, so that a wrong pixel points at the
right kernel. Well-formed streams only; every comparison is exact."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pngdec_restatement as R                                        # noqa: E402
from maggie_amd.utils import geometry, pngdec                         # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pngdec_pinned.npz')
_CASES, _REF = {}, {}


def cases():
    if not _CASES:
        _CASES.update(R.all_cases())
    return _CASES


def ref(name):
    """(file, inflated bytes, L plane) of a case: computed once, never modified."""
    if name not in _REF:
        d = cases()[name]
        _REF[name] = (d, zlib.decompress(R.walk(d)[2]), R.pillow(d))
    return _REF[name]


def check(r, names):
    """`raw` first, then the planes, of a `Decoded` against the references of `names`."""
    assert (r.status == 0).all() and r.readbacks == 1
    raw = r.raw.cpu().numpy()
    out = r.out.cpu().numpy()
    for k, n in enumerate(names):
        _, want_raw, want = ref(n)
        assert r.raw_sizes[k] == len(want_raw) and raw[k, :len(want_raw)].tobytes() == want_raw, (n, 'inflated bytes')
        assert out[k].shape == want.shape and np.array_equal(out[k], want), (n, 'pixels')
        assert (int(r.info[k, 4]) & 0xffffffff) == zlib.adler32(want_raw) and r.info[k, 4] == r.info[k, 5], (n, 'Adler-32')


@pytest.mark.parametrize('part', range(4))
def test_decode_is_exact_on_the_list(part):
    for name in list(cases())[part::4]:
        d = ref(name)[0]
        check(pngdec.decode_stats([d]), [name])
        out = pngdec.decode(d)
        assert out.dtype == torch.uint8 and out.is_cuda and out.dim() == 2 and np.array_equal(out.cpu().numpy(), ref(name)[2]), name


def test_decode_planes_of_three_and_of_mixed_colour_types():
    by_size = {}
    for n, d in cases().items():
        by_size.setdefault(R.walk(d)[0][:2], []).append(n)
    groups = [g for g in by_size.values() if len(g) > 1]
    assert any(len({R.walk(cases()[n])[0][3] for n in g}) == 4 for g in groups)      # grey, grey + alpha, RGB and RGBA in one launch
    for g in groups:
        check(pngdec.decode_stats([ref(n)[0] for n in g]), g)
        three = g[:3] if len(g) >= 3 else (g + g)[:3]
        planes = pngdec.decode_planes([ref(n)[0] for n in three])
        assert planes.shape == (3,) + ref(g[0])[2].shape and np.array_equal(planes.cpu().numpy(), np.stack([ref(n)[2] for n in three]))
    # into a destination of the caller's, reshaped to (T, n_i, h, w)
    g = max(groups, key=len)[:6]
    h, w = ref(g[0])[2].shape
    dst = torch.full((2, 3, h, w), 9, dtype=torch.uint8, device='cuda')
    got = pngdec.decode_planes([ref(n)[0] for n in g], out=dst)
    assert got.data_ptr() == dst.data_ptr() and np.array_equal(dst.cpu().numpy().reshape(6, h, w), np.stack([ref(n)[2] for n in g]))
    with pytest.raises(ValueError, match='out must be'):
        pngdec.decode_planes([ref(n)[0] for n in g], out=dst[:1])


def test_fixture_key_by_key():
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith('file_'))
    assert len(names) >= 12
    for name in names:
        got = pngdec.decode(z['file_' + name].tobytes())
        assert np.array_equal(got.cpu().numpy(), z['l_' + name]), name


def test_stream_at_an_odd_offset_between_guards():
    for name, front in (('wrap', 13), ('rgba', 1), ('p_bits2', 7), ('l_stored', 3), ('far_match', 2)):
        d, want_raw, want = ref(name)
        plan = pngdec.parse(d)
        blob = torch.frombuffer(bytearray(b'\xff' * front + plan.stream + b'\xff' * 29), dtype=torch.uint8).cuda()
        r = pngdec.run(blob, pngdec.record(plan, front)[None], plan.height, plan.width, guard=64)
        check(r, [name])
        assert len(r.guards) == 4 and all(bool((g == 0xA5).all()) for g in r.guards), name
        tail = r.raw.cpu().numpy()[0, len(want_raw):]
        assert (tail == 0xA5).all(), name                      # nothing behind the file's own bytes either


def test_stored_block_behind_a_huffman_block_where_the_stage_is_refilled():
    # 32 files of one size in one launch, their streams at every offset mod 4: the bit reader hands bytes back right behind a refill of the stage
    files = [R.huffman_then_stored(3328, literals, nine, empty) for literals in range(130, 400, 39) for nine in (0, 3, 5, 6) for empty in (0, 1)][:32]
    r = pngdec.decode_stats(files)
    raw = r.raw.cpu().numpy()
    for k, d in enumerate(files):
        want = zlib.decompress(R.walk(d)[2])
        assert r.status[k] == 0 and raw[k, :len(want)].tobytes() == want and r.blocks[k] == 3 + k % 2, k
    assert np.array_equal(r.out.cpu().numpy(), np.stack([R.pillow(d) for d in files]))


def test_round_count_is_the_restatement_s():
    for name in list(cases()):
        if name == 'large':
            continue                                           # its restatement takes seconds on the host; tests/test_pngdec_cpu.py runs it
        d = ref(name)[0]
        _, rounds, blocks, tokens = R.inflate_rounds(R.walk(d)[2], len(ref(name)[1]))
        r = pngdec.decode_stats([d])
        assert r.rounds[0] <= rounds and r.blocks[0] == blocks and r.tokens[0] == tokens, (name, r.rounds[0], rounds)


def test_decode_planes_feeds_resize_short_pad():
    names = ['f4_c0_130x67', 'f3_c6_130x67', 'f1_c2_130x67', 'f2_c4_130x67']
    alphas = pngdec.decode_planes([ref(n)[0] for n in names]).reshape(2, 2, 130, 67)
    want = np.stack([ref(n)[2] for n in names]).reshape(2, 2, 130, 67)
    frames = np.repeat(want[:, 0, :, :, None], 3, -1)
    a = geometry.resize_short_pad(torch.from_numpy(frames).cuda(), alphas, alphas, short_size=96, divisor=32)
    b = geometry.resize_short_pad(frames, want, want, short_size=96, divisor=32)
    assert a[1].shape == b[1].shape and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])
