"""PNG frames and planes without a GPU: the restatement (tests/pngcolor_restatement.py) against live Pillow and the pinned fixture;
`pngcolor.parse` against the pass formula and on what it has to refuse; the routing of `load_planes` and `load_frames`; the header's
constants and the -2 returns of the entry points; and the kernel source itself, compiled for the host with the address and
undefined-behaviour sanitizers (tests/csrc/pngcolor_host.cpp), on the case list, on hostile records and on hostile streams."""
import ctypes
import os
import re
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pngcolor_restatement as R                            # noqa: E402
from maggie_amd.utils import jpegsamp, pngcolor, pngdec     # noqa: E402

P = R.P
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pngcolor_pinned.npz')
ST_SIZE, ST_FILTER, ST_INDEX, ST_RECORD = 2, 256, 512, 1024


@pytest.fixture(scope='module')
def cases():
    pytest.importorskip('PIL')
    c = R.small_cases()
    c.update(R.clip_cases())
    return c


@pytest.fixture(scope='module')
def restated(cases):
    """name -> (defiltered bytes, RGB, L): computed once, shared, never changed."""
    return {n: R.decode(d) for n, d in cases.items()}


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_live_pillow(cases, restated):
    for name, d in cases.items():
        rgb, l = R.pillow(d)
        assert np.array_equal(restated[name][1], rgb), (name, 'RGB')
        assert np.array_equal(restated[name][2], l), (name, 'L')


def test_the_list_holds_what_it_claims(cases, restated):
    heads = {n: P.walk(d)[0] for n, d in cases.items()}
    assert {(h[3], h[2], h[6]) for h in heads.values()} == {(ct, dp, i) for ct, dp in R.PAIRS for i in (0, 1)}
    sizes = {(h[0], h[1]) for h in heads.values()}
    assert sizes >= {(1, 1), (1, 5), (5, 1), (2, 2), (3, 2), (4, 4), (5, 5), (8, 8), (9, 9), (17, 13), (11, 6), (15, 3), (16, 3), (17, 3), (33, 3),
                     (9, 131), (480, 270)}
    assert {h[1] for h in heads.values()} >= {64, 65, 129}
    assert {P.rowbytes(h[3], h[2], h[0]) for h in heads.values() if not h[6]} >= {63, 64, 65}

    def filters(name):
        w, h, depth, ct, _, _, lace = heads[name]
        raw, got = restated[name][0], []
        for pw, ph, rb, off in R.pass_table(w, h, ct, depth, lace)[0]:
            if pw and ph:
                got.append([raw[off + y * (1 + rb)] for y in range(ph)])
        return got
    for bpp in (1, 2, 3, 4, 6, 8):
        for ft in range(5):
            per_pass = filters('ft%d_bpp%d_i1_9x9' % (ft, bpp))
            assert len(per_pass) == 7 and all(set(rows) == {ft} for rows in per_pass)      # the first row of every pass included
            assert filters('ft%d_bpp%d_i0_5x5' % (ft, bpp)) == [[ft] * 5]
    assert len(filters('band_c2_d8_i1_9x131')[6]) == 65       # pass 7 exceeds one band
    assert R.pass_table(4, 4, 2, 8, 1)[0][1][0] == 0 and R.pass_table(1, 5, 2, 8, 1)[0][1][:2] == (0, 1)      # empty passes
    edges = R.decode_samples(cases['grey16_edges_i0_4x2'])[1]
    assert {0, 255, 256, 65535} <= set(edges.reshape(-1).tolist())
    assert restated['grey16_edges_i0_4x2'][2].reshape(-1).tolist() == [0, 255, 255, 255, 1, 254, 255, 255]     # saturation, not the high byte
    assert len(P.walk(cases['short_palette_d4_i0_13x7'])[1]) == 33 and b'tRNS' in cases['trns_rgb_i1_13x7']


def test_fixture_equals_restatement_and_live_pillow():
    pytest.importorskip('PIL')
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith('file_'))
    assert len(names) >= 19
    live = R.small_cases()
    for name in names:
        d = z['file_' + name].tobytes()
        assert d == live[name], name                           # the writer is deterministic
        _, rgb, l = R.decode(d)
        assert np.array_equal(z['rgb_' + name], rgb) and np.array_equal(z['l_' + name], l), name
        prgb, pl = R.pillow(d)
        assert np.array_equal(z['rgb_' + name], prgb) and np.array_equal(z['l_' + name], pl), name


# ---- parse -------------------------------------------------------------------------------------------------------------------------------------
def test_parse_pass_table_is_the_formula(cases, restated):
    for name, d in cases.items():
        plan = pngcolor.parse(d)
        w, h, depth, ct, _, _, lace = P.walk(d)[0]
        table, total = R.pass_table(w, h, ct, depth, lace)
        assert [tuple(t) for t in plan.passes] == table and plan.raw_size == total == len(restated[name][0]), name
        assert plan.interlace == lace and len(plan.passes) == (7 if lace else 1) and plan.size == (h, w), name
        assert plan.stream == P.walk(d)[2], name
        if ct == 3:
            assert plan.palette.tobytes() == P.walk(d)[1] and plan.entries == len(plan.palette), name
        rec = pngcolor.record(plan, 12)
        assert rec.shape == (pngcolor.REC_WORDS,) and rec[0] == 12 and rec[6] == total and rec[5] == lace, name
    # for x0, y0, dx, dy in ADAM7: ceil((w - x0) / dx) x ceil((h - y0) / dy), empty passes included
    for w, h in ((1, 1), (1, 5), (5, 1), (4, 4), (3, 2), (8, 8), (9, 9), (33, 3), (1920, 1080)):
        table = pngcolor.passes(w, h, 6, 16, 1)[0]
        for (pw, ph, rb, off), (x0, y0, dx, dy) in zip(table, pngcolor.ADAM7):
            assert pw == max(0, -(-(w - x0) // dx)) and ph == max(0, -(-(h - y0) // dy)) and rb == pw * 8
        assert sum(pw * ph for pw, ph, _, _ in table) == w * h
    assert [t[:2] for t in pngcolor.passes(1, 1, 0, 8, 1)[0]] == [(1, 1), (0, 1), (1, 0), (0, 1), (1, 0), (0, 1), (1, 0)]
    assert pngcolor.ADAM7 == R.ADAM7


def test_parse_refuses_by_name():
    assert pngcolor.Unsupported is pngdec.Unsupported
    good = P.png(4, 1, 8, 0, bytes(5))
    assert pngcolor.parse(good).size == (1, 4)
    assert pngcolor.parse(P.png(4, 1, 8, 0, bytes(10), interlace=1)).interlace == 1           # passes 1 and 2: 1 + 1 and 1 + 1 ... accepted
    assert pngcolor.parse(P.png(4, 1, 16, 0, bytes(9))).depth == 16
    with pytest.raises(pngcolor.Unsupported, match='critical chunk'):
        pngcolor.parse(good[:33] + P.chunk(b'FOOb', b'') + good[33:])
    with pytest.raises(pngcolor.Unsupported, match='sides up to'):
        pngcolor.parse(P.png(40000, 1, 8, 0, bytes(5)))
    wide = pngcolor.MAX_ROWBYTES // 8
    assert pngcolor.parse(P.png(3840, 1, 16, 6, bytes(1 + 30720))).rowbytes == 30720              # UHD width of the widest pixel
    assert pngcolor.parse(P.png(wide, 1, 16, 6, bytes(1 + 8 * wide))).rowbytes == pngcolor.MAX_ROWBYTES
    with pytest.raises(pngcolor.Unsupported, match='bytes a row'):
        pngcolor.parse(P.png(wide + 1, 1, 16, 6, bytes(5)))
    with pytest.raises(pngcolor.Unsupported, match='inflated bytes'):
        pngcolor.parse(P.png(16384, 32767, 16, 0, bytes(5)))          # 32767 x (1 + 32768) = 2^30 - 1
    with pytest.raises(pngcolor.Unsupported, match='zlib stream of'):
        old = pngdec.MAX_BYTES
        pngdec.MAX_BYTES = 8
        try:
            pngcolor.parse(good)
        finally:
            pngdec.MAX_BYTES = old

    def plain(exc):
        assert not isinstance(exc.value, pngcolor.Unsupported)
    with pytest.raises(ValueError, match='signature') as e:
        pngcolor.parse(b'\x89PNX' + good[4:])
    plain(e)
    bad = bytearray(good)
    bad[good.index(b'IDAT') + 5] ^= 1
    with pytest.raises(ValueError, match='CRC in the IDAT') as e:
        pngcolor.parse(bytes(bad))
    plain(e)
    with pytest.raises(ValueError, match='ends') as e:
        pngcolor.parse(good[:-1])
    plain(e)
    with pytest.raises(ValueError, match='malformed IHDR'):
        pngcolor.parse(P.png(4, 1, 16, 3, bytes(9)))             # a 16-bit palette is not a PNG
    with pytest.raises(ValueError, match='malformed IHDR'):
        pngcolor.parse(P.png(4, 1, 4, 2, bytes(9)))
    with pytest.raises(ValueError, match='without PLTE'):
        pngcolor.parse(P.png(4, 1, 8, 3, bytes(5), interlace=1))
    with pytest.raises(ValueError, match='zlib header'):
        pngcolor.parse(P.png(4, 1, 8, 0, zstream=b'\x78\x9d' + zlib.compress(bytes(5))[2:]))
    with pytest.raises(TypeError):
        pngcolor.parse('a.png')
    # what pngdec refuses stays refused there
    with pytest.raises(pngdec.Unsupported, match='Adam7'):
        pngdec.parse(P.png(4, 1, 8, 0, bytes(10), interlace=1))
    with pytest.raises(pngdec.Unsupported, match='16-bit'):
        pngdec.parse(P.png(4, 1, 16, 0, bytes(9)))


def test_calls_refuse_before_any_launch():
    a, b = P.png(4, 1, 8, 0, bytes(5)), P.png(4, 2, 8, 0, bytes(10))
    for fn in (pngcolor.decode_frames, pngcolor.decode_planes, pngcolor.decode_stats, pngcolor.load_planes, pngcolor.load_frames):
        with pytest.raises(TypeError):
            fn(a)
        with pytest.raises(ValueError, match='at least one'):
            fn([])
    for fn in (pngcolor.decode_frames, pngcolor.decode_planes, pngcolor.load_planes, pngcolor.load_frames):
        with pytest.raises(ValueError, match='share one size'):
            fn([a, b])
    with pytest.raises(TypeError):
        pngcolor.decode_frame(12)
    with pytest.raises(TypeError):
        pngcolor.decode(12)
    with pytest.raises(ValueError, match='neither a JPEG nor a PNG'):
        pngcolor.load_frames([a, b'GIF89a' + bytes(20)])
    with pytest.raises(pngdec.Unsupported, match='sides up to %d and rows' % pngdec.MAX_SIDE):      # neither takes it: pngdec's refusal
        pngcolor.load_planes([P.png(40000, 1, 8, 0, bytes(5))])


def test_load_planes_and_load_frames_route(monkeypatch):
    """Which decoder gets which file, and that the result comes back in the order of `datas`: the launches are replaced by markers."""
    cpu = torch.device('cpu')
    monkeypatch.setattr(pngcolor, 'resolve_device', lambda *a, **k: cpu)
    seen = {}

    def fake_pngdec(datas, *, device=None, out=None):
        seen['pngdec'] = list(datas)
        out.fill_(1)
        return out

    def fake_run(plans, mode, mean, std, device, out):
        seen['pngcolor'] = [(p.interlace, p.depth) for p in plans]
        seen['mode'] = mode
        if out is None:
            out = torch.empty((len(plans),) + plans[0].size + (3,), dtype=torch.uint8)
        out.fill_(2)
        r = pngcolor.Decoded()
        r.out = out
        return r

    def fake_jpeg(datas, *, normalize=False, mean=None, std=None, device=None):
        seen['jpeg'] = list(datas)
        return torch.full((len(datas), 1, 4, 3), 3, dtype=torch.uint8)
    monkeypatch.setattr(pngdec, 'decode_planes', fake_pngdec)
    monkeypatch.setattr(pngcolor, 'run_plans', fake_run)
    monkeypatch.setattr(jpegsamp, 'load_clip', fake_jpeg)
    plain, laced, deep = P.png(4, 1, 8, 0, bytes(5)), P.png(4, 1, 8, 0, bytes(10), interlace=1), P.png(4, 1, 16, 0, bytes(9))
    got = pngcolor.load_planes([laced, plain, deep, plain])
    assert seen['pngdec'] == [plain, plain] and seen['pngcolor'] == [(1, 8), (0, 16)] and seen['mode'] == pngcolor.OUT_L
    assert got.shape == (4, 1, 4) and got[:, 0, 0].tolist() == [2, 1, 2, 1]
    seen.clear()
    assert pngcolor.load_planes([plain])[0, 0, 0] == 1 and 'pngcolor' not in seen
    jpg = b'\xff\xd8' + bytes(30)
    got = pngcolor.load_frames([jpg, plain, jpg + b'x', laced])
    assert seen['jpeg'] == [jpg, jpg + b'x'] and seen['pngcolor'] == [(0, 8), (1, 8)] and seen['mode'] == pngcolor.OUT_RGB
    assert got.shape == (4, 1, 4, 3) and got[:, 0, 0, 0].tolist() == [3, 2, 3, 2]
    seen.clear()
    assert pngcolor.load_frames([plain])[0, 0, 0, 0] == 2 and 'jpeg' not in seen
    seen.clear()
    assert pngcolor.load_frames([jpg])[0, 0, 0, 0] == 3 and 'pngcolor' not in seen


# ---- the header and the entry points -----------------------------------------------------------------------------------------------------------
def test_header_constants_equal_the_module_s():
    text = open(os.path.join(ROOT, 'include', 'maggie_hip.h')).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (MG_PNGCOLOR_\w+) (\d+)\b', text)}
    assert defs == {'MG_PNGCOLOR_REC_WORDS': pngcolor.REC_WORDS, 'MG_PNGCOLOR_REC_PASSES': pngcolor.REC_PASSES,
                    'MG_PNGCOLOR_REC_LTABLE': pngcolor.REC_LTABLE, 'MG_PNGCOLOR_REC_PALETTE': pngcolor.REC_PALETTE,
                    'MG_PNGCOLOR_MAX_ROWBYTES': pngcolor.MAX_ROWBYTES, 'MG_PNGCOLOR_GROUP': pngcolor.GROUP, 'MG_PNGCOLOR_OUT_RGB': pngcolor.OUT_RGB,
                    'MG_PNGCOLOR_OUT_L': pngcolor.OUT_L, 'MG_PNGCOLOR_OUT_NORM': pngcolor.OUT_NORM}
    assert pngcolor.MAX_ROWBYTES == 32768 and 3840 * 8 <= pngcolor.MAX_ROWBYTES


def test_entry_points_return_minus_two():
    from maggie_amd import hip
    lib = hip.lib()
    vals = [ctypes.c_int(0) for _ in range(6)]
    assert lib.mg_pngcolor_limits(*[ctypes.byref(v) for v in vals]) == 0
    assert [v.value for v in vals] == [pngcolor.THREADS, pngcolor.MAX_SIDE, pngcolor.MAX_ROWBYTES, pngcolor.REC_WORDS, pngcolor.INFO_WORDS,
                                       pngcolor.GROUP]
    assert lib.mg_pngcolor_limits(None, *[ctypes.byref(v) for v in vals[1:]]) == -2
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p = ctypes.c_void_p
    L, I = ctypes.c_long, ctypes.c_int
    f3 = (ctypes.c_float * 3)(1, 1, 1)

    def inflate(data=base, nbytes=64, recs=base + 256, raw=base + 2048, stride=16, info=base + 1536, files=1, h=1, w=1):
        return lib.mg_pngcolor_inflate(p(data), L(nbytes), p(recs), p(raw), L(stride), p(info), L(files), I(h), I(w), None)

    def unfilter(raw=base + 2048, stride=16, recs=base + 256, info=base + 1536, files=1, h=1, w=1):
        return lib.mg_pngcolor_unfilter(p(raw), L(stride), p(recs), p(info), L(files), I(h), I(w), None)

    def convert(raw=base + 2048, stride=16, recs=base + 256, out=base + 4096, info=base + 1536, files=1, h=1, w=1, mode=0, mean=f3, std=f3):
        return lib.mg_pngcolor_convert(p(raw), L(stride), p(recs), p(out), p(info), L(files), I(h), I(w), I(mode), mean, std, None)
    for kw in (dict(data=None), dict(recs=None), dict(raw=None), dict(info=None), dict(data=base + 1), dict(raw=base + 2052), dict(recs=base + 258),
               dict(nbytes=-1), dict(nbytes=pngdec.MAX_BYTES + 1), dict(stride=0), dict(stride=24), dict(stride=pngdec.MAX_RAW + 16), dict(files=0),
               dict(h=0), dict(w=0), dict(h=pngdec.MAX_SIDE + 1), dict(w=pngdec.MAX_SIDE + 1)):
        assert inflate(**kw) == -2, kw
    for kw in (dict(raw=None), dict(recs=None), dict(info=None), dict(info=base + 1538), dict(recs=base + 258), dict(stride=8), dict(stride=40),
               dict(files=-1), dict(h=0), dict(w=-3), dict(h=pngdec.MAX_SIDE + 1)):
        assert unfilter(**kw) == -2, kw
    for kw in (dict(raw=None), dict(recs=None), dict(out=None), dict(info=None), dict(info=base + 1538), dict(stride=8), dict(files=0), dict(h=0),
               dict(w=pngdec.MAX_SIDE + 1), dict(mode=3), dict(mode=-1), dict(out=base + 2048), dict(out=base + 2063), dict(out=base + 2046),
               dict(mode=2, out=base + 4097), dict(mode=2, mean=None), dict(mode=2, std=None)):
        assert convert(**kw) == -2, kw
    assert inflate(files=1 << 31) == -3 and unfilter(files=1 << 16, stride=16) == -3 and convert(files=1 << 16, out=base + 64) == -3


# ---- the kernel source on the host, under the sanitizers ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('pngcolor_host') / 'pngcolor_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'pngcolor_host.cpp')])
    return exe


PER = {pngcolor.OUT_RGB: 3, pngcolor.OUT_L: 1, pngcolor.OUT_NORM: 12}


def _case(plans, mode, front=0, recs=None):
    """One launch of the host program: the streams of `plans` concatenated behind `front` bytes, so that offsets are odd. `raw` gets the
    stride the TRUE geometry asks for, whatever the (possibly hostile) records say."""
    h, w = plans[0].size
    blob, made = b'\x5a' * front, []
    for pl in plans:
        made.append(pngcolor.record(pl, len(blob)))
        blob += pl.stream
    true = [pngcolor.passes(pl.width, pl.height, pl.color_type, pl.depth, pl.interlace)[1] for pl in plans]
    stride = -(-max(true) // 16) * 16
    recs = np.stack(made) if recs is None else recs(np.stack(made))
    return struct.pack('<6i', h, w, len(plans), len(blob), mode, stride) + recs.astype(np.int32).tobytes() + blob, (len(plans), h, w, mode, stride)


def _run_host(exe, tmp_path, cases, tag):
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(cases)) + b''.join(c for c, _ in cases))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'pngcolor_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, buf, p = [], open(dst, 'rb').read(), 0
    for _, (F, h, w, mode, stride) in cases:
        rc = struct.unpack_from('<4i', buf, p)
        p += 16
        info = np.frombuffer(buf, np.int32, F * pngcolor.INFO_WORDS, p).reshape(F, -1)
        p += 4 * F * pngcolor.INFO_WORDS
        raw = np.frombuffer(buf, np.uint8, F * stride, p).reshape(F, stride)
        p += F * stride
        assert rc[3] == F * h * w * PER[mode]
        img = np.frombuffer(buf, np.uint8, rc[3], p)
        p += rc[3]
        img = img.view(np.float32).reshape(F, 3, h, w) if mode == pngcolor.OUT_NORM else img.reshape((F, h, w, 3) if mode == pngcolor.OUT_RGB else (F, h, w))
        out.append((rc[:3], info, raw, img))
    assert p == len(buf)
    return out


def _norm(rgb):
    """ToTensor + Normalize of uint8 (h, w, 3) in float32, IEEE operations: (v / 255 - mean) / std."""
    x = rgb.astype(np.float32).transpose(2, 0, 1) / np.float32(255.0)
    m = np.array(pngcolor.IMAGENET_MEAN, np.float32)[:, None, None]
    s = np.array(pngcolor.IMAGENET_STD, np.float32)[:, None, None]
    return (x - m) / s


def test_host_build_reproduces_the_restatement(host_exe, tmp_path, cases, restated):
    names = [n for n in cases if not n.startswith('clip') or n.startswith('clip0')]        # one frame of the 270 x 480 clip: the host wave is slow
    plans = {n: pngcolor.parse(cases[n]) for n in names}
    # every file alone as RGB and as L (at offset 1, 2, 3, 0, ...), the files of one size together -- type, depth and interlace mixed in one
    # launch -- and the normalised form on one group
    runs = [([n], mode) for n in names if not n.startswith('clip') for mode in (pngcolor.OUT_RGB, pngcolor.OUT_L)] + [(['clip0_c2_d8_i0_480x270'], 0)]
    by_size = {}
    for n in names:
        by_size.setdefault(plans[n].size, []).append(n)
    groups = [g for g in by_size.values() if len(g) > 1]
    assert any(len({(plans[n].color_type, plans[n].depth, plans[n].interlace) for n in g}) == 30 for g in groups)
    runs += [(g, k % 2) for k, g in enumerate(groups)] + [(max(groups, key=len), pngcolor.OUT_NORM)]
    made = [_case([plans[n] for n in g], mode, front=(k + 1) % 4) for k, (g, mode) in enumerate(runs)]
    for (g, mode), (rc, info, raw, img) in zip(runs, _run_host(host_exe, tmp_path, made, 'list')):
        assert tuple(rc) == (0, 0, 0), g
        for k, n in enumerate(g):
            want_raw, rgb, l = restated[n]
            assert info[k, 0] == 0, (n, info[k])
            assert raw[k, :len(want_raw)].tobytes() == want_raw, (n, 'defiltered bytes')
            assert (raw[k, len(want_raw):] == 0xA5).all(), n    # nothing written behind the file's bytes
            if mode == pngcolor.OUT_NORM:
                assert np.array_equal(img[k].view(np.int32), _norm(rgb).view(np.int32)), (n, 'normalised')
            else:
                assert np.array_equal(img[k], rgb if mode == pngcolor.OUT_RGB else l), (n, 'pixels')


def _with_stream(plan, stream):
    q = pngdec.PngPlan(**plan.__dict__)
    q.stream = stream
    return q


def _with_raw(plan, raw):
    return _with_stream(plan, zlib.compress(bytes(raw)))


def test_host_build_stays_clean_on_hostile_records_and_streams(host_exe, tmp_path, cases, restated):
    name = 'pair_c3_d2_i1_17x13'
    plan = pngcolor.parse(cases[name])
    raw = zlib.decompress(plan.stream)
    last = plan.passes[6]
    made, expect = [], []

    def add(pl, status, recs=None, mode=pngcolor.OUT_RGB, front=1):
        made.append(_case([pl], mode, front=front + len(made) % 4, recs=recs))
        expect.append(status)
    add(_with_raw(plan, raw[:last[3] + 3]), ST_SIZE)                                   # a truncated pass
    add(_with_raw(plan, raw[:plan.passes[3][3]]), ST_SIZE)                             # the stream ends with pass 3
    add(_with_raw(plan, raw + b'\0'), ST_SIZE)                                         # one byte more
    add(_with_raw(plan, raw[:-1]), ST_SIZE)                                            # one byte fewer
    five = bytearray(raw)
    five[plan.passes[4][3] + (1 + plan.passes[4][2])] = 5                              # filter type 5 on the second row of pass 5
    add(_with_raw(plan, five), ST_FILTER)
    short = pngdec.PngPlan(**plan.__dict__)                                            # a palette index past PLTE
    short.entries = int(R.decode_samples(cases[name])[1].max())
    add(short, ST_INDEX)
    add(short, ST_INDEX, mode=pngcolor.OUT_L)

    def lie(word, value):
        def change(recs):
            recs = recs.copy()
            recs[0, word] = value
            return recs
        return change
    first_record = len(made)
    for word, value in ((pngcolor.REC_PASSES + 4 * 6 + 3, 1 << 20), (pngcolor.REC_PASSES + 4 * 6 + 3, -4), (pngcolor.REC_PASSES + 3, 16),     # pass offsets outside `raw`
                        (6, plan.raw_size + 64), (6, 1 << 30), (6, 0), (pngcolor.REC_PASSES + 4 * 2 + 1, 1 << 14), (pngcolor.REC_PASSES + 2, 1 << 15),
                        (3, 16), (3, 3), (2, 5), (5, 2), (5, 0), (4, 257), (4, -1), (0, -8), (1, 1 << 27), (0, 1 << 27)):
        add(plan, ST_RECORD, recs=lie(word, value))
    first_stream = len(made)
    streams = [plan.stream[:len(plan.stream) * k // 4] for k in (1, 2, 3)]
    for i in range(2, len(plan.stream)):
        s = bytearray(plan.stream)
        s[i] ^= (1, 0x80, 0xff)[i % 3]
        streams.append(bytes(s))
    for s in streams:
        add(_with_stream(plan, s), None)
    res = _run_host(host_exe, tmp_path, made, 'hostile')
    want_raw, rgb, l = restated[name]
    for k, (status, (rc, info, rawbuf, img)) in enumerate(zip(expect, res)):
        assert tuple(rc) == (0, 0, 0), k
        got = int(info[0, 0])
        if status is None:                                     # a changed stream: refused, or (a change of unused bits) decoded right
            assert got != 0 or (rawbuf[0, :len(want_raw)].tobytes() == want_raw and np.array_equal(img[0], rgb)), k
            continue
        assert got & status, (k, got, status)
        if status == ST_RECORD:
            assert got == ST_RECORD and (rawbuf == 0xA5).all(), k                     # nothing of the file is touched
        if status != ST_INDEX:
            assert (img == 0xA5).all(), k                      # the convert launch skips a file whose status is not 0
    assert first_record < first_stream and any(int(r[1][0, 0]) & 128 for r in res[first_stream:]) and any(int(r[1][0, 0]) & 1 for r in res[first_stream:])
    # filter type 5 decodes as type 0
    rb = plan.passes[4][2]
    at = plan.passes[4][3] + (1 + rb)
    line = res[4][2][0, at:at + 1 + rb]
    assert line[0] == 5 and line[1:].tobytes() == bytes(five[at + 1:at + 1 + rb])
