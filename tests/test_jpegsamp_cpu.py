"""Host side of the device decoder of the other chroma samplings (maggie_amd.utils.jpegsamp: 4:2:2, 4:4:0, 4:1:1): the restatement and its two
writers against live Pillow on every case; `parse` on the list and on what it must refuse; argument errors before any launch; the dispatch of
`load_clip`; the C entries' argument errors at layouts 3, 4 and 5; and the kernel sources themselves compiled for the host (one thread per GPU thread) under the
address and undefined-behaviour sanitizers as a stand-alone program, on the case list, at both epilogues, and on hostile streams. No GPU needed."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jpegdec_restatement as R                                       # noqa: E402
import jpegsamp_restatement as S                                      # noqa: E402
from maggie_amd.utils import jpegdec, jpegprog, jpegsamp              # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(S.CASES)
LAYOUT = {'422': jpegsamp.L422, '440': jpegsamp.L440, '411': jpegsamp.L411}
MEAN, STD = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])


# ---- the restatement and the writers -------------------------------------------------------------------------------------------------------------
def test_the_case_list_is_the_one_the_issue_names():
    for samp in S.SAMPLINGS:
        mine = [c for c in S.CASES.values() if c[0] == samp]
        base = [c for c in mine if not c[5].get('progressive') and c[4] != 'prog']
        assert {c[1:3] for c in base} == set(S.SIZES) and len(S.SIZES) == 23
        assert {c[5].get('quality') for c in base} >= {1, 50, 90, 100} and {c[3] for c in base} == set(R.KINDS)
        for size in ((37, 53), (64, 48)):
            kw = [c[5] for c in base if c[1:3] == size]
            assert {k.get('ri') for k in kw} >= {1, 3} and {k['qtables'][0][0] for k in kw if 'qtables' in k} == {1, 255}
            assert any(k.get('ri') == -(-size[1] // (8 * S.SAMPLINGS[samp][0])) for k in kw)            # a restart per MCU row
        prog = {c[1:3] for c in mine if c[5].get('progressive') or c[4] == 'prog'}
        assert prog == (set(S.SIZES) if samp == '422' else set(S.PROG_SIZES))
    p422 = [c[5] for c in S.CASES.values() if c[0] == '422' and c[4] == 'pillow']
    assert any(k.get('optimize') for k in p422) and {k.get('restart_marker_blocks') for k in p422} >= {1, 3}
    assert any(k.get('restart_marker_rows') == 1 for k in p422) and any(k.get('progressive') and k.get('restart_marker_blocks') for k in p422)
    assert {k['quality'] for k in p422 if k.get('progressive')} == {50, 90}
    assert all(c[4] != 'pillow' for c in S.CASES.values() if c[0] != '422')


@pytest.mark.parametrize('part', range(4))
def test_restatement_equals_live_pillow(part):
    """Pillow's own 4:2:2 files (baseline, and progressive with its ten-scan script) and the writers' 4:4:0 / 4:1:1 files; the writer-made 4:2:2
    files tie the writers to Pillow's own."""
    pytest.importorskip('PIL')
    for name in S.parts(4)[part]:
        data = S.stream(name)
        assert np.array_equal(S.decode(data), S.pillow(data)), name


def test_the_scripts_are_the_ones_the_issue_names():
    pytest.importorskip('PIL')
    import jpegprog_restatement as PR
    full = PR.script(S.stream('422_17x23_uniform_pillow_proT_qua90'))
    assert len(full) == 10 and any(s[3] for s in full)                      # Pillow's script: refinement scans
    assert PR.script(S.stream('440_17x23_flat_prog_qua100')) == [((0, 1, 2), 0, 0, 0, 0)] + [((c,), 1, 63, 0, 0) for c in range(3)]
    for samp, (hs, vs) in S.SAMPLINGS.items():
        name = [n for n in NAMES if n.startswith(samp + '_37x53') and 'pro' not in n][0]
        assert S.header(S.stream(name))['comps'][0][1:3] == (hs, vs)


def test_the_fancy_rules_are_used():
    """4:4:0 at h = 4 and 8: the neighbour of the last real chroma row is that row, not the block's padding row below it."""
    pytest.importorskip('PIL')
    hit = 0
    for name in NAMES:
        samp, h, w = S.CASES[name][:3]
        if samp == '440' and (h, w) in ((4, 4), (8, 8), (4, 9)):
            data = S.stream(name)
            coef = S.coefficients(data)
            cb = S.planes_of(data, coef)[1]
            ch = -(-h // 2)
            hit += not np.array_equal(cb[ch - 1, :w], cb[ch, :w])
    assert hit >= 1


# ---- parse -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('part', range(2))
def test_parse_returns_layout_kind_and_tables(part):
    pytest.importorskip('PIL')
    for name in NAMES[part::2]:
        data, samp = S.stream(name), S.CASES[name][0]
        hdr = S.header(data)
        plan = jpegsamp.parse(data)
        assert plan.geometry == (hdr['h'], hdr['w'], LAYOUT[samp]) and plan.sampling == (S.SAMPLINGS[samp], (1, 1), (1, 1)), name
        assert plan.kind == ('progressive' if S.progressive(data) else 'baseline')
        for k, comp in enumerate(hdr['comps']):
            assert np.array_equal(plan.qtables[k], hdr['quant'][comp[3]])
        if plan.kind == 'baseline':
            assert isinstance(plan, jpegdec.JpegPlan) and (plan.offset, plan.length, plan.restart_interval) == (hdr['offset'], hdr['length'], hdr['ri'])
            assert plan.mcus == S.geometry(hdr)[3] * S.geometry(hdr)[4]
            for kind in ('dc', 'ac'):
                for i, (counts, values) in hdr[kind].items():
                    assert np.array_equal(getattr(plan, kind)[i][0], counts) and np.array_equal(getattr(plan, kind)[i][1], values)
            rec = jpegdec.record(plan, 0)
            hs, vs = S.SAMPLINGS[samp]
            sel = plan.selectors
            assert rec[912:918].tolist() == ([sel[0][0] | sel[0][1] << 4] * (hs * vs) + [s[0] | s[1] << 4 for s in sel[1:]] + [0] * 6)[:6]
        else:
            import jpegprog_restatement as PR
            assert isinstance(plan, jpegprog.ProgPlan) and plan.script == PR.script(data)
            assert [c[0] for c in plan.chains] == ['dc', 'ac', 'ac', 'ac'] and sorted(k for c in plan.chains for k in c[2]) == list(range(len(plan.scans)))
        for f in (jpegdec.parse, jpegprog.parse):                         # the two existing parsers keep refusing these files
            with pytest.raises(jpegdec.Unsupported):
                f(data)


def _save(x, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(x).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def _resample(data, *hv):
    """The sampling bytes of the frame header replaced (the scan no longer fits: only `parse` may see such a file)."""
    d = bytearray(data)
    sof = d.index(b'\xff\xc0') if b'\xff\xc0' in d else d.index(b'\xff\xc2')
    for k, b in enumerate(hv):
        d[sof + 11 + 3 * k] = b
    return bytes(d)


def test_parse_rejects_what_the_device_does_not_decode():
    pytest.importorskip('PIL')
    x = R.image(17, 23, 'smooth', 1, 2)
    for kw in (dict(subsampling=2), dict(subsampling=0), dict(subsampling=2, progressive=True), dict(subsampling=0, progressive=True)):
        with pytest.raises(jpegdec.Unsupported, match='use jpegdec'):
            jpegsamp.parse(_save(x, quality=80, **kw))
    with pytest.raises(jpegdec.Unsupported, match='use jpegdec'):
        jpegsamp.parse(_save(x[..., 0], quality=80))
    good = _save(x, quality=80, subsampling=1)
    prog = _save(x, quality=80, subsampling=1, progressive=True)
    assert jpegsamp.parse(good).layout == jpegsamp.L422 and jpegsamp.parse(prog).layout == jpegsamp.L422
    for src in (good, prog):
        for hv, text in (((0x42,), r'\(4, 2\)'), ((0x41, 0x21), r'\(2, 1\)'), ((0x21, 0x11, 0x12), r'\(1, 2\)\)'), ((0x22, 0x21, 0x21), r'\(2, 2\), \(2, 1\)'),
                         ((0x31,), r'\(3, 1\)'), ((0x14,), r'\(1, 4\)')):
            with pytest.raises(jpegdec.Unsupported, match='sampling.*' + text):
                jpegsamp.parse(_resample(src, *hv))
        assert jpegsamp.parse(_resample(src, 0x12)).layout == jpegsamp.L440 and jpegsamp.parse(_resample(src, 0x41)).layout == jpegsamp.L411
    # what the two existing parsers refuse, a sample of the cases of their own tests
    g = bytearray(good)
    sof = g.index(b'\xff\xc0')
    bad = bytearray(g); bad[sof + 4] = 12
    with pytest.raises(jpegdec.Unsupported, match='12-bit'):
        jpegsamp.parse(bytes(bad))
    bad = bytearray(g)
    bad[sof + 2:sof + 4] = struct.pack('>H', 8 + 3 * 4)
    bad[sof + 9] = 4
    bad[sof + 19:sof + 19] = bytes([4, 0x11, 0])
    with pytest.raises(jpegdec.Unsupported, match='4 components'):
        jpegsamp.parse(bytes(bad))
    dqt = g.index(b'\xff\xdb')
    bad = bytearray(g); bad[dqt + 4] |= 0x10
    with pytest.raises(jpegdec.Unsupported, match='16-bit'):
        jpegsamp.parse(bytes(bad))
    with pytest.raises(jpegdec.Unsupported, match='Adobe'):
        jpegsamp.parse(good[:2] + b'\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00' + good[2:])
    with pytest.raises(jpegdec.Unsupported, match='DNL'):
        jpegsamp.parse(good[:-2] + b'\xff\xdc\x00\x04\x00\x11\xff\xd9')
    with pytest.raises(jpegdec.Unsupported, match='several scans'):
        jpegsamp.parse(good[:-2] + good[good.index(b'\xff\xda'):])
    bad = bytearray(g); bad[sof + 1] = 0xC9
    with pytest.raises(jpegdec.Unsupported, match='arithmetic'):
        jpegsamp.parse(bytes(bad))
    with pytest.raises(jpegdec.Unsupported, match='incomplete progression'):
        jpegsamp.parse(prog[:prog.rindex(b'\xff\xda')] + b'\xff\xd9')
    p = bytearray(prog); p[p.index(b'\xff\xc2') + 4] = 12
    with pytest.raises(jpegdec.Unsupported, match='12-bit'):
        jpegsamp.parse(bytes(p))
    for junk in (b'', b'\x89PNG\r\n\x1a\n' + bytes(40), good[:40], prog[:60]):
        with pytest.raises(jpegdec.Unsupported):
            jpegsamp.parse(junk)
    assert {jpegsamp.L422, jpegsamp.L440, jpegsamp.L411}.isdisjoint({jpegdec.L420, jpegdec.L444, jpegdec.GREY})
    assert jpegsamp.LUMA == {jpegsamp.L422: (2, 1), jpegsamp.L440: (1, 2), jpegsamp.L411: (4, 1)}


# ---- the public functions --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch(monkeypatch):
    pytest.importorskip('PIL')
    from maggie_amd import hip
    monkeypatch.setattr(hip, 'call', lambda *a, **k: pytest.fail('a launch'))
    data = S.stream('422_17x23_flat_pillow_qua90')
    for f in (jpegsamp.decode, jpegsamp.load):
        for bad in (None, 'file.jpg', 5, np.zeros(4, np.uint8)):
            with pytest.raises(TypeError):
                f(bad)
    for f in (jpegsamp.decode_clip, jpegsamp.load_clip, jpegsamp.decode_stats):
        with pytest.raises(TypeError):
            f(data)
        with pytest.raises(TypeError):
            f([data, None])
        with pytest.raises(ValueError):
            f([])
        with pytest.raises(TypeError):
            f([data], std=None)
    for s in (jpegdec.MIN_SUB - 1, jpegdec.MAX_SUB + 1):
        with pytest.raises(ValueError):
            jpegsamp.decode_stats([data], sub_bytes=s)
    x = R.image(17, 23, 'smooth', 1, 2)
    for f in (jpegsamp.decode, jpegsamp.load):
        with pytest.raises(jpegdec.Unsupported):
            f(_resample(_save(x, quality=80, subsampling=1), 0x42))
    with pytest.raises(jpegdec.Unsupported, match='use jpegdec'):
        jpegsamp.decode(_save(x, quality=80))
    with pytest.raises(jpegdec.Unsupported, match='only SOF0 baseline'):           # no parser takes it: the refusal of jpegdec.parse
        jpegsamp.load(_resample(_save(x, quality=80, subsampling=1, progressive=True), 0x42))
    for f in (jpegsamp.decode, jpegsamp.decode_clip, jpegsamp.load_clip):
        assert 'graph' in f.__doc__
    assert 'no CPU fallback' in jpegsamp.__doc__ and 'read-back' in jpegsamp.__doc__


def test_a_clip_shares_one_size_and_one_layout(monkeypatch):
    pytest.importorskip('PIL')
    from maggie_amd import hip
    monkeypatch.setattr(hip, 'call', lambda *a, **k: pytest.fail('a launch'))
    a, b = S.stream('422_17x23_flat_pillow_qua90'), S.stream('422_23x17_binary_pillow_qua100')
    with pytest.raises(ValueError, match='one size'):
        jpegsamp.decode_clip([a, b])
    with pytest.raises(ValueError, match='one size'):
        jpegsamp.decode_clip([a, S.stream('440_17x23_flat_base_qua90')])            # same size, another layout
    with pytest.raises(ValueError, match='all baseline or all progressive'):
        jpegsamp.decode_clip([a, S.stream('422_17x23_uniform_pillow_proT_qua90')])
    with pytest.raises(ValueError, match='one size'):
        jpegsamp.load_clip([a, b])


def test_no_gpu_raises_maggie_hip_error():
    import torch
    from maggie_amd.hip import MaggieHipError
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(MaggieHipError):
        jpegsamp.decode(S.stream('422_17x23_flat_pillow_qua90'))


def test_load_dispatches_by_parsing_only(monkeypatch):
    pytest.importorskip('PIL')
    import torch
    x = R.image(37, 53, 'uniform', 5, 0)
    b420, p420 = _save(x, quality=50, subsampling=2), _save(x, quality=50, subsampling=2, progressive=True)
    b422 = [_save(x, quality=q, subsampling=1) for q in (50, 90)]
    p422 = _save(x, quality=50, subsampling=1, progressive=True)
    b440 = S.stream('440_37x53_uniform_base_qua90_ri1')
    seen = []

    def fake_baseline(datas, plans, normalize, mean, std, device, out):
        seen.append(('jpegdec', list(datas), [type(p).__name__ for p in plans]))
        out.fill_(1)

    def fake_clip(datas, normalize, mean, std, device, out=None, plans=None):
        seen.append(('jpegprog', list(datas), [type(p).__name__ for p in plans]))
        out.fill_(2)

    def fake_run(datas, plans, normalize, mean, std, device, sub_bytes, out):
        seen.append(('jpegsamp', list(datas), [(p.kind, p.layout) for p in plans]))
        out.fill_(3 + len([s for s in seen if s[0] == 'jpegsamp']))
    monkeypatch.setattr(jpegprog, '_baseline', fake_baseline)
    monkeypatch.setattr(jpegprog, '_clip', fake_clip)
    monkeypatch.setattr(jpegsamp, '_run', fake_run)
    monkeypatch.setattr(jpegsamp, 'resolve_device', lambda device=None: torch.device('cpu'))
    out = jpegsamp.load_clip([b422[0], b420, p422, b440, b422[1], p420])
    assert out.shape == (6, 37, 53, 3) and out.dtype == torch.uint8 and out[:, 0, 0, 0].tolist() == [4, 1, 5, 6, 4, 2]
    assert seen == [('jpegsamp', b422, [('baseline', jpegsamp.L422)] * 2), ('jpegdec', [b420], ['JpegPlan']),
                    ('jpegsamp', [p422], [('progressive', jpegsamp.L422)]), ('jpegsamp', [b440], [('baseline', jpegsamp.L440)]),
                    ('jpegprog', [p420], ['ProgPlan'])]                          # each (kind, layout) group once
    seen.clear()
    assert jpegsamp.load(p422, normalize=True).shape == (3, 37, 53) and [s[0] for s in seen] == ['jpegsamp']


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------------------
def test_pitched_layouts_reject_bad_arguments_before_any_launch():
    from maggie_amd import hip
    I, L = ctypes.c_int, ctypes.c_long
    lib = hip.lib()
    for fn in (lib.mg_jpegdec_sync, lib.mg_jpegdec_coef, lib.mg_jpegdec_dcsum, lib.mg_jpegdec_idct, lib.mg_jpeg_rgb_hv, lib.mg_jpegprog_chains):
        fn.restype = ctypes.c_int
    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    a, b, c = (ctypes.c_void_p(4096 * k) for k in (1, 2, 3))
    odd = ctypes.c_void_p(4100)
    L422, L440, L411 = jpegsamp.L422, jpegsamp.L440, jpegsamp.L411
    assert (L422, L440, L411) == (3, 4, 5)
    # 16 x 16 at 4:2:2: one MCU column, two MCU rows, 4 blocks each; planes 16 x 16 + 2 x 16 x 8
    E, PB = 8 * 64, 512

    def sync(n=1, nsub=4, s=8, layout=L422, launch=0, words=8, data=a, nbytes=64):
        return lib.mg_jpegdec_sync(data, L(nbytes), b, c, c, c, c, c, I(words), L(n), I(nsub), I(s), I(layout), I(launch), None)

    def coef(n=1, nsub=4, s=8, h=16, w=16, layout=L422, elems=E, data=a):
        return lib.mg_jpegdec_coef(data, L(64), b, c, c, c, c, L(elems), c, L(n), I(nsub), I(s), I(h), I(w), I(layout), None)

    def dcsum(n=1, h=16, w=16, layout=L422, elems=E, p=a):
        return lib.mg_jpegdec_dcsum(p, L(elems), b, L(n), I(h), I(w), I(layout), None)

    def idct(n=1, h=16, w=16, layout=L422, elems=E, pb=PB, planes=c, p=a):
        return lib.mg_jpegdec_idct(p, L(elems), b, planes, L(pb), L(n), I(h), I(w), I(layout), None)

    def rgb(n=1, h=16, w=16, luma=(2, 1), pb=PB, e=0, mean=three, planes=a, out=b):
        return lib.mg_jpeg_rgb_hv(planes, L(pb), out, L(n), I(h), I(w), I(luma[0]), I(luma[1]), I(e), mean, mean, None)

    def chains(n=1, h=16, w=16, layout=L422, elems=E, data=a, nbytes=64, nscans=1, nchains=1):
        return lib.mg_jpegprog_chains(data, L(nbytes), b, L(nscans), c, L(nchains), c, L(elems), c, L(n), I(h), I(w), I(layout), None)
    every = (sync, coef, dcsum, idct, rgb, chains)
    layouts = (sync, coef, dcsum, idct, chains)
    assert sync(n=0) == coef(n=0, elems=0) == dcsum(n=0, elems=0) == idct(n=0, elems=0, pb=0) == rgb(n=0, pb=0) == chains(n=0, elems=0) == 0
    assert sync(data=None) == coef(data=None) == dcsum(p=None) == idct(p=None) == rgb(planes=None) == chains(data=None) == -2
    for luma in ((2, 2), (1, 1), (3, 1), (0, 1), (1, 4), (2, 0), (4, 2), (-2, 1)):
        assert rgb(luma=luma) == -2, luma
    for layout in (6, 7, -1, 1 << 20):                                     # and the sizes of another layout's buffers do not fit this one's
        assert [f(layout=layout) for f in layouts] == [-2] * 5, layout
    for layout in (jpegdec.L420, jpegdec.L444, jpegdec.GREY, L411):
        assert [f(layout=layout) for f in (coef, dcsum, idct, chains)] == [-2] * 4, layout
    assert [f(n=-1) for f in every] == [-2] * 6
    for bad in (dict(nsub=0), dict(s=jpegdec.MIN_SUB - 1), dict(s=jpegdec.MAX_SUB + 1), dict(nsub=1 << 20, s=4096)):
        assert sync(**bad) == coef(**bad) == -2, bad
    assert sync(launch=-1) == sync(launch=3, words=8) == sync(words=3) == sync(nbytes=-1) == -2
    for bad in (dict(h=0), dict(w=0), dict(h=32768), dict(w=32768), dict(elems=E - 1), dict(elems=E + 64), dict(elems=12 * 64)):
        assert coef(**bad) == dcsum(**bad) == idct(**bad) == chains(**bad) == -2, bad
    assert chains(nbytes=-1) == chains(nscans=-1) == chains(nchains=-1) == chains(nbytes=(1 << 28) + 1) == -2
    assert idct(pb=PB - 1) == idct(pb=PB + 16) == idct(planes=odd) == idct(planes=None) == -2
    assert rgb(pb=PB - 1) == rgb(e=2) == rgb(e=-1) == rgb(mean=None) == rgb(out=a) == rgb(out=None) == rgb(planes=odd) == rgb(h=0) == rgb(w=32768) == -2
    # the pitched planes: 4:4:0 at w = 8 has luma and chroma rows of 16 bytes, 4:1:1 at w = 8 luma rows of 32 and chroma rows of 8
    assert idct(layout=L440, h=16, w=8, elems=4 * 64, pb=16 * 16 + 2 * 8 * 8) == rgb(luma=(1, 2), h=16, w=8, pb=16 * 16 + 2 * 8 * 8) == -2
    assert idct(layout=L411, h=8, w=8, elems=6 * 64, pb=8 * 8 * 3) == rgb(luma=(4, 1), h=8, w=8, pb=8 * 8 * 3) == -2
    assert jpegdec.geometry(16, 8, L440) == (4, 16 * 16 + 2 * 8 * 16, 16, 16, 8, 16) and jpegdec.geometry(8, 8, L411) == (6, 8 * 32 + 2 * 8 * 8, 8, 32, 8, 8)
    assert jpegdec.geometry(16, 16, L422)[:2] == (E // 64, PB)
    header = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    for name in ('mg_jpegdec_sync', 'mg_jpegdec_coef', 'mg_jpegdec_dcsum', 'mg_jpegdec_idct', 'mg_jpeg_rgb_hv', 'mg_jpegprog_chains'):
        assert 'int %s(' % name in header


# ---- the kernel sources on the host, under the sanitizers ----------------------------------------------------------------------------------------
def _case_bytes(datas, sub_bytes=8, recs=None):
    plans = [jpegsamp.parse(d) for d in datas]
    h, w, layout = plans[0].geometry
    T = len(datas)
    if plans[0].kind == 'baseline':
        offs = np.concatenate([[0], np.cumsum([len(d) for d in datas])])
        if recs is None:
            recs = np.stack([jpegdec.record(p, int(o)) for p, o in zip(plans, offs)])
        blob, scans, chains = b''.join(datas), np.zeros((0, 480), np.int32), np.zeros((0, 4), np.int32)
    else:
        blob, scans, chains, qt = jpegprog.pack(plans, datas)
        recs = np.zeros((T, jpegdec.TAB_WORDS), np.int32)
        recs[:, 928:1120] = qt.reshape(T, 192)
    head = struct.pack('<10i', plans[0].kind == 'progressive', h, w, layout, 0, sub_bytes, T, len(scans), len(chains), len(blob))
    return head + recs.astype('<i4').tobytes() + scans.astype('<i4').tobytes() + chains.astype('<i4').tobytes() + blob


def _run_host(exe, tmp_path, cases, tag):
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'jpegsamp_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, raw, p = [], open(dst, 'rb').read(), 0
    for _ in cases:
        rc, status, nc, npl, nrgb = struct.unpack_from('<5i', raw, p)
        p += 20
        coef = np.frombuffer(raw, '<i2', nc, p); p += 2 * nc
        planes = np.frombuffer(raw, np.uint8, npl, p); p += npl
        rgb = np.frombuffer(raw, np.uint8, nrgb, p); p += nrgb
        norm = np.frombuffer(raw, '<f4', nrgb, p); p += 4 * nrgb
        out.append(dict(rc=rc, status=status, coef=coef, planes=planes, rgb=rgb, norm=norm))
    assert p == len(raw)
    return out


@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('jpegsamp_host') / 'jpegsamp_host')
    # the flags of test_jpegdec_cpu.py's host_exe (-fwrapv: a hostile stream can make the 32-bit inverse passes wrap, as libjpeg's do)
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fwrapv',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'jpegsamp_host.cpp')])
    return exe


def _check(datas, r, where):
    samp = [k for k, v in LAYOUT.items() if v == jpegsamp.parse(datas[0]).layout][0]
    hs, vs = S.SAMPLINGS[samp]
    assert r['rc'] == 0 and r['status'] == 0, (where, r['rc'], r['status'])
    coefs = [S.coefficients(d) for d in datas]
    assert np.array_equal(r['coef'], np.concatenate([c.reshape(-1) for c in coefs])), where
    hdr = S.header(datas[0])
    h, w, T = hdr['h'], hdr['w'], len(datas)
    want = [S.planes_of(d, c) for d, c in zip(datas, coefs)]
    for k, got in enumerate(S.device_planes(r['planes'], T, h, w, hs, vs)):
        assert np.array_equal(got, np.stack([p[k] for p in want])), (where, 'plane %d' % k)
    px = np.stack([S.pixels(d, c) for d, c in zip(datas, coefs)])
    assert np.array_equal(r['rgb'].reshape(T, h, w, 3), px), where
    norm = ((px.astype(np.float32) / np.float32(255) - MEAN) / STD).transpose(0, 3, 1, 2)
    assert np.array_equal(r['norm'].reshape(T, 3, h, w).view(np.uint32), np.ascontiguousarray(norm).view(np.uint32)), where


def test_host_build_of_the_kernels_reproduces_the_restatement(host_exe, tmp_path):
    """The whole chain -- entropy, inverse transform, colour at both epilogues -- baseline and progressive, on every case; the restart, optimised-
    table and extreme-table cases at every sub_bytes; clips of three files with tables, restart intervals and scripts per file."""
    pytest.importorskip('PIL')
    special = [n for n in NAMES if any(k in n for k in ('_ri', 'rs', 'opt', 'qta')) and 'pro' not in n]
    jobs = [([S.stream(n)], s) for i, n in enumerate(NAMES) for s in (R.SUB_BYTES if n in special else R.SUB_BYTES[i % 3:i % 3 + 1])]
    for samp in S.SAMPLINGS:
        clip = [n for n in NAMES if n.startswith(samp + '_37x53') and 'pro' not in n][:3]
        jobs.append(([S.stream(n) for n in clip], 29))
    jobs.append(([S.stream(n) for n in ('422_37x53_binary_pillow_proT_qua90', '422_37x53_uniform_pillow_proT_qua90_rsb1', '422_37x53_flat_pillow_proT_qua50')], 8))
    res = _run_host(host_exe, tmp_path, [_case_bytes(d, s) for d, s in jobs], 'list')
    for k, ((datas, s), r) in enumerate(zip(jobs, res)):
        _check(datas, r, (NAMES[k] if k < len(NAMES) else 'clip %d' % k, s))


def test_host_build_stays_clean_on_hostile_streams(host_exe, tmp_path):
    """Exactly sized buffers under ASan / UBSan: segments cut at 1/4, 1/2 and 3/4, every single-byte flip of a short baseline and of a short
    progressive stream, a DRI that lies. Every run ends with a status word; nothing is read or written out of bounds."""
    pytest.importorskip('PIL')
    cases, kinds = [], []
    for name in ('422_64x48_smooth_pillow_qua50_rsb1', '440_37x53_uniform_base_qua90_ri3', '411_64x48_smooth_base_qua50_ri1'):
        data = S.stream(name)
        plan = jpegsamp.parse(data)
        for frac in (1, 2, 3):
            cut = data[:plan.offset + plan.length * frac // 4] + b'\xff\xd9'
            for s in R.SUB_BYTES:
                cases.append(_case_bytes([cut], s)); kinds.append('cut')
    data = S.stream('422_37x53_uniform_pillow_proT_qua90_rsb1')
    plan = jpegsamp.parse(data)
    for k in (0, 1, len(plan.scans) - 1):                                   # a scan of a progressive file cut in the middle: the record says so
        _, scans, chains, qt = jpegprog.pack([plan], [data])
        at = [i for i in range(len(scans)) if scans[i, 456] == plan.scans[k].offset][0]
        scans[at, 457] //= 2
        recs = np.zeros((1, jpegdec.TAB_WORDS), np.int32)
        recs[:, 928:1120] = qt.reshape(1, 192)
        cases.append(struct.pack('<10i', 1, 37, 53, jpegsamp.L422, 0, 8, 1, len(scans), len(chains), len(data)) + recs.tobytes() + scans.astype('<i4').tobytes() +
                     chains.astype('<i4').tobytes() + data)
        kinds.append('cut')
    for start, end in (('440_8x8_', 'qua100'), ('411_9x4_', 'prog_qua90'), ('422_4x4_', 'proT_qua50')):
        short = S.stream([n for n in NAMES if n.startswith(start) and n.endswith(end)][0])
        for i in range(len(short)):
            flipped = short[:i] + bytes([short[i] ^ 0xFF]) + short[i + 1:]
            try:
                plan = jpegsamp.parse(flipped)
                if plan.width * plan.height > 1 << 12:
                    continue
                cases.append(_case_bytes([flipped], jpegdec.MIN_SUB)); kinds.append('flip')
            except jpegdec.Unsupported:
                continue
    for name, ri in (('422_64x48_smooth_pillow_qua50_rsb1', 2), ('440_37x53_uniform_base_qua90_ri3', 4), ('411_37x53_uniform_base_qua90_ri1', 0)):
        data = S.stream(name)
        rec = jpegdec.record(jpegsamp.parse(data), 0)
        assert rec[920] != ri
        rec[920] = ri
        cases.append(_case_bytes([data], 29, rec[None])); kinds.append('dri')
    assert kinds.count('flip') > 300
    res = _run_host(host_exe, tmp_path, cases, 'hostile')
    for kind, r in zip(kinds, res):
        assert r['rc'] == 0
        if kind in ('cut', 'dri'):
            assert r['status'] != 0, kind
    assert sum(1 for k, r in zip(kinds, res) if k == 'flip' and r['status']) > 30
