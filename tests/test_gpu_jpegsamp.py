"""The device decoder of the other chroma samplings (maggie_amd.utils.jpegsamp: 4:2:2, 4:4:0, 4:1:1; layouts 3 to 5 of csrc/jpegdec.hip and
jpegprog.hip, and mg_jpeg_rgb_hv of photometric.hip) against the restatement of tests/jpegsamp_restatement.py, which tests/test_jpegsamp_cpu.py holds against
Pillow itself: the coefficients first, then the component planes, then the pixels, so that a wrong pixel points at the right kernel.
Well-formed streams only; every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))

import jpegdec_restatement as R                                       # noqa: E402
import jpegsamp_restatement as S                                      # noqa: E402
import make_jpegsamp_golden as G                                      # noqa: E402
from helpers import load_golden                                       # noqa: E402
from maggie_amd.utils import geometry, jpegdec, jpegprog, jpegsamp    # noqa: E402
from maggie_amd.utils._inputs import IMAGENET_MEAN, IMAGENET_STD      # noqa: E402
from maggie_amd.utils.preprocess import normalize_frames              # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(S.CASES)
PARTS = S.parts(8)
SPECIAL = [n for n in NAMES if any(k in n for k in ('_ri', 'rs', 'opt', 'qta')) and 'pro' not in n]
_REF = {}


def ref(name):
    """(stream, coefficients, planes [Y, Cb, Cr] over whole MCUs, pixels) of a case: computed once, never modified."""
    if name not in _REF:
        data = S.stream(name)
        coef = S.coefficients(data)
        _REF[name] = (data, coef, [p.astype(np.uint8) for p in S.planes_of(data, coef)], S.pixels(data, coef))
    return _REF[name]


def check(name, sub_bytes=None):
    data, coef, planes, px = ref(name)
    samp, h, w = S.CASES[name][:3]
    r = jpegsamp.decode_stats([data], sub_bytes=sub_bytes)
    assert np.array_equal(r.coef.cpu().numpy().reshape(-1, 64), coef), (name, sub_bytes, 'coefficients')
    for k, got in enumerate(S.device_planes(r.planes.cpu().numpy(), 1, h, w, *S.SAMPLINGS[samp])):
        assert np.array_equal(got[0], planes[k]), (name, sub_bytes, 'plane %d' % k)
    assert r.out.shape == (1,) + px.shape and np.array_equal(r.out[0].cpu().numpy(), px), (name, sub_bytes, 'pixels')
    assert r.readbacks >= 1
    return r


@pytest.mark.parametrize('part', range(8))
def test_decode_stats_equals_the_restatement_on_the_list(part):
    for name in PARTS[part]:
        check(name)


@pytest.mark.parametrize('part', range(8))
def test_decode_equals_the_pixels_on_the_list(part):
    for name in PARTS[part]:
        data, _, _, px = ref(name)
        out = jpegsamp.decode(data)
        assert out.dtype == torch.uint8 and out.is_cuda and out.shape == px.shape and np.array_equal(out.cpu().numpy(), px), name


@pytest.mark.parametrize('sub_bytes', R.SUB_BYTES)
def test_every_sub_bytes_gives_the_same_coefficients(sub_bytes):
    assert len(SPECIAL) >= 30
    for name in SPECIAL:
        r = check(name, sub_bytes)
        assert r.rounds <= r.subsequences and r.launches <= -(-r.subsequences // jpegdec.THREADS) + 2


def _clips():
    out = []
    for samp in S.SAMPLINGS:
        out.append([n for n in NAMES if n.startswith(samp + '_37x53') and 'pro' not in n][:3])
        out.append([n for n in NAMES if n.startswith(samp + '_64x48') and 'pro' not in n][-3:])
    out.append(['422_37x53_binary_pillow_proT_qua90', '422_37x53_uniform_pillow_proT_qua90_rsb1', '422_37x53_flat_pillow_proT_qua50'])
    return out


@pytest.mark.parametrize('names', _clips())
def test_decode_clip_takes_per_file_tables_restarts_and_scripts(names):
    assert len(names) == 3 and len({tuple(sorted((k, v) for k, v in S.CASES[n][5].items() if k[:2] in ('ri', 're'))) for n in names}) > 1
    datas = [ref(n)[0] for n in names]
    want = np.stack([ref(n)[3] for n in names])
    r = jpegsamp.decode_stats(datas, sub_bytes=29)
    assert np.array_equal(r.coef.cpu().numpy(), np.stack([ref(n)[1] for n in names]))
    assert np.array_equal(r.out.cpu().numpy(), want) and r.readbacks >= 1 and (r.readbacks == 1 or 'pro' not in names[0])
    out = jpegsamp.decode_clip(datas)
    assert out.shape == want.shape and np.array_equal(out.cpu().numpy(), want)
    norm = jpegsamp.decode_clip(datas, normalize=True)
    assert norm.shape == (3, 3) + want.shape[1:3] and np.array_equal(norm.cpu().numpy(), R.P.normalize(want, IMAGENET_MEAN, IMAGENET_STD))


@pytest.mark.parametrize('name', ['422_64x48_smooth_pillow_qua50_rsb1', '440_64x48_smooth_base_qua50_ri3', '411_64x48_smooth_base_qua50_ri1',
                                  '422_37x53_uniform_pillow_proT_qua90_rsb1', '440_37x53_binary_prog_qua1', '411_17x23_flat_prog_qua100'])
def test_normalize_epilogue(name):
    data, _, _, px = ref(name)
    mean, std = (0.4, 0.5, 0.6), (0.2, 0.25, 0.3)
    for m, s in ((IMAGENET_MEAN, IMAGENET_STD), (mean, std)):
        out = jpegsamp.decode(data, normalize=True, mean=m, std=s)
        assert out.dtype == torch.float32 and out.shape == (3,) + px.shape[:2]
        assert np.array_equal(out.cpu().numpy(), R.P.normalize(px[None], m, s)[0])
        if px.shape[0] * px.shape[1] % 4 == 0:                              # where normalize_frames is defined
            assert torch.equal(out, normalize_frames(jpegsamp.decode(data), m, s))


@pytest.mark.parametrize('name', G.PINNED)
def test_fixture_key_by_key(name):
    d = load_golden('jpegsamp_pinned.npz')
    out = jpegsamp.decode(d[name + '.stream'].tobytes())
    assert np.array_equal(out.cpu().numpy(), d[name + '.pixels'])


@pytest.mark.parametrize('name', ['422_37x53_uniform_pillow_qua90_rsb1', '440_37x53_uniform_base_qua90_ri3', '411_37x53_uniform_base_qua90_ri1',
                                  '422_37x53_uniform_pillow_proT_qua90_rsb1', '440_17x23_flat_prog_qua100', '411_37x53_binary_prog_qua1'])
def test_odd_offset_inside_a_larger_buffer_and_guarded_outputs(name):
    data, coef, _, px = ref(name)
    plan = jpegsamp.parse(data)
    h, w, layout = plan.geometry
    for pad in (1, 3, 7):
        blob = torch.from_numpy(np.frombuffer(b'\xff' * pad + data + b'\xff\x00\xd0' * 11, np.uint8).copy()).cuda()
        for normalize in (False, True):
            n = h * w * 3
            guard = torch.full((n + 64,), 7, dtype=torch.float32 if normalize else torch.uint8, device='cuda')
            if plan.kind == 'baseline':
                r = jpegdec.run(blob, jpegdec.record(plan, pad)[None], h, w, layout, sub_bytes=29, normalize=normalize, out=guard[13:13 + n])
            else:
                scans, chains = jpegprog.records(plan, pad, 0, 0)
                r = jpegprog.run(blob, scans, chains, plan.qtables[None], h, w, layout, normalize=normalize, out=guard[13:13 + n])
            assert np.array_equal(r.coef.cpu().numpy()[0], coef)
            got = guard.cpu().numpy()
            assert (got[:13] == 7).all() and (got[13 + n:] == 7).all()
            want = R.P.normalize(px[None], IMAGENET_MEAN, IMAGENET_STD)[0] if normalize else px
            assert np.array_equal(got[13:13 + n].reshape(want.shape), want)
            guard.fill_(7)                                                  # the public `out=`: a slice of a guard-filled tensor
            jpegsamp.decode(data, normalize=normalize, out=guard[16:16 + n])
            got = guard.cpu().numpy()
            assert (got[:16] == 7).all() and (got[16 + n:] == 7).all() and np.array_equal(got[16:16 + n].reshape(want.shape), want)


def test_load_clip_of_a_mixed_list_equals_pillow_frame_by_frame(monkeypatch):
    from PIL import Image
    import io
    x = R.image(37, 53, 'uniform', 11, 0)

    def save(**kw):
        buf = io.BytesIO()
        Image.fromarray(x).save(buf, 'JPEG', **kw)
        return buf.getvalue()
    datas = [save(quality=90, subsampling=1, progressive=True), save(quality=75, subsampling=2), save(quality=90, subsampling=1),
             save(quality=50, subsampling=1), save(quality=50, subsampling=1, progressive=True), save(quality=50, subsampling=2)]
    want = np.stack([R.pillow(d) for d in datas])
    calls = []
    for mod, fn in ((jpegdec, 'run'), (jpegprog, 'run')):
        real = getattr(mod, fn)
        at = 4 if mod is jpegdec else 6                                      # where `layout` stands among run's arguments
        monkeypatch.setattr(mod, fn, lambda *a, _real=real, _m=mod.__name__.rsplit('.', 1)[1], _at=at, **k: (calls.append((_m, a[_at])), _real(*a, **k))[1])
    out = jpegsamp.load_clip(datas)
    assert out.shape == want.shape and out.dtype == torch.uint8 and np.array_equal(out.cpu().numpy(), want)
    assert calls == [('jpegprog', jpegsamp.L422), ('jpegdec', jpegdec.L420), ('jpegdec', jpegsamp.L422)]      # one launch set per group
    norm = jpegsamp.load_clip(datas, normalize=True)
    assert np.array_equal(norm.cpu().numpy(), R.P.normalize(want, IMAGENET_MEAN, IMAGENET_STD))
    for d, y in zip(datas, want):
        assert np.array_equal(jpegsamp.load(d).cpu().numpy(), y)


def test_decode_feeds_resize_short_pad():
    for name in ('422_64x48_smooth_pillow_qua50_rsb1', '440_64x48_smooth_base_qua50_ri3'):
        data = ref(name)[0]
        a = geometry.resize_short_pad(jpegsamp.decode_clip([data]), short_size=96, divisor=32)
        b = geometry.resize_short_pad(R.pillow(data)[None], short_size=96, divisor=32)
        assert a[0].shape == b[0].shape and torch.equal(a[0], b[0])


def test_load_clip_crosses_all_six_layouts_in_both_kinds(monkeypatch):
    """One baseline and one progressive 37 x 53 file of each of the six layouts, from the case lists of the three restatements (each has all
    its kinds at 37 x 53, the progressive grey file included), shuffled with a fixed seed: every frame equals its restatement's pixels, and
    `jpegdec.run` and `jpegprog.run` are each entered once per layout. Twelve groups of one file each come out in input order whatever the
    shuffle, so the same clip is then decoded with every file twice, the second copies shuffled among the first: still twelve launch sets,
    and the frames have to be permuted back."""
    import jpegprog_restatement as J
    files = []
    for mode in (2, 0, 'L'):
        files.append((R, R.stream(*R.CASES['37x53_uniform_%s_qua90' % mode])))
        files.append((J, J.stream(*J.CASES['37x53_uniform_%s_q90' % mode])))
    for name in ('422_37x53_uniform_base_qua90_ri3', '440_37x53_uniform_base_qua90_ri3', '411_37x53_uniform_base_qua90_ri3',
                 '422_37x53_uniform_pillow_proT_qua90_rsb1', '440_37x53_binary_prog_qua1', '411_37x53_binary_prog_qua1'):
        files.append((S, S.stream(name)))
    want = [m.pixels(d, m.coefficients(d)) for m, d in files]
    assert len(files) == 12 and all(px.shape == (37, 53, 3) for px in want)
    calls = []
    for mod, at in ((jpegdec, 4), (jpegprog, 6)):                          # where `layout` stands among run's arguments
        real = mod.run
        monkeypatch.setattr(mod, 'run', lambda *a, _real=real, _m=mod.__name__.rsplit('.', 1)[1], _at=at, **k: (calls.append((_m, a[_at])), _real(*a, **k))[1])
    six = [jpegdec.L420, jpegdec.L444, jpegdec.GREY, jpegsamp.L422, jpegsamp.L440, jpegsamp.L411]
    rs = np.random.RandomState(20)
    for order in (rs.permutation(12), rs.permutation(24) % 12):
        del calls[:]
        out = jpegsamp.load_clip([files[k][1] for k in order])
        assert out.shape == (len(order), 37, 53, 3) and out.dtype == torch.uint8
        got = out.cpu().numpy()
        for i, k in enumerate(order):
            assert np.array_equal(got[i], want[k]), (i, k)
        assert len(calls) == 12 and sorted(calls) == sorted([(m, l) for m in ('jpegdec', 'jpegprog') for l in six])
