"""PNG decoding without a GPU: the restatement (tests/pngdec_restatement.py) against zlib, live Pillow and the pinned fixture; `pngdec.parse`
against what Pillow reports and on what it has to refuse; the -2 returns of the entry points; and the kernel source itself, compiled for the
host with the address and undefined-behaviour sanitizers (tests/csrc/pngdec_host.cpp), on the case list and on hostile streams."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pngdec_restatement as R                              # noqa: E402
from maggie_amd.utils import jpegdec, pngdec                # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'pngdec_pinned.npz')


@pytest.fixture(scope='module')
def cases():
    pytest.importorskip('PIL')
    return R.all_cases()


@pytest.fixture(scope='module')
def restated(cases):
    """name -> (inflated bytes, L plane, rounds) by the restatement's round algorithm: computed once, shared, never changed."""
    return {name: R.decode_raw(d, rounds=True) for name, d in cases.items()}


# ---- the restatement --------------------------------------------------------------------------------------------------------------------------
def test_restatement_inflate_equals_zlib(cases, restated):
    seen, longest = set(), 0
    for name, d in cases.items():
        (w, h, depth, ct, _, _, _), _, z, _ = R.walk(d)
        stats = {}
        raw = R.inflate(z, h * (1 + R.rowbytes(ct, depth, w)), stats)
        assert raw == zlib.decompress(z), name
        assert restated[name][0] == raw, name                  # the round algorithm on the ring gives the same bytes
        seen |= stats['types']
        longest = max(longest, stats['maxlen'])
        if name == 'z_fibonacci':
            assert stats['maxlen'] == 15
    assert seen == {0, 1, 2} and longest == 15


def test_restatement_equals_live_pillow(cases, restated):
    for name, d in cases.items():
        assert np.array_equal(restated[name][1], R.pillow(d)), name


def test_the_list_holds_what_it_claims(cases, restated):
    def stat(name):
        (w, h, depth, ct, _, _, _), _, z, n = R.walk(cases[name])
        st = {}
        R.inflate(z, None, st)
        raw = restated[name][0]
        return st['types'], n, set(raw[::1 + R.rowbytes(ct, depth, w)]), len(raw)
    assert stat('l_stored')[0] == {0} and stat('l_1x1')[0] == {1} and stat('z_fixed')[0] == {1}
    types, chunks, _, size = stat('large')
    assert chunks >= 4 and size > 16 * R.RING and len([e for e in R.tokens(R.walk(cases['large'])[2]) if e[0] == 'block']) > 4
    assert stat('z_flushes')[0] == {0, 2} and stat('z_flushes')[1] == 4
    assert set().union(*(stat(n)[2] for n in ('l_smooth', 'l_noise', 'l_flat'))) >= {0, 1, 2, 4}
    assert 3 in stat('l_smooth_opt')[2] and 3 not in stat('l_smooth')[2]      # Pillow picks the average filter only with optimize=True
    assert stat('grey2')[2] == {0, 1, 2, 3, 4} and stat('wrap')[3] > R.RING
    ev = [e[:3] for e in R.tokens(R.walk(cases['far_match'])[2])]
    assert ('match', 258, 32768) in ev and ('match', 258, 1) in ev and ('match', 10, 3) in ev and ('lit', 255) in ev
    ev = [e[:3] for e in R.tokens(R.walk(cases['far_after'])[2])]
    k = ev.index(('match', 3, 32758))                        # literals behind a far match in one round, and a match whose bytes alias its sources
    assert all(e[0] == 'lit' for e in ev[k + 1:k + 21]) and ev[k + 21] == ('match', 40, 32763) and (k + 20) // 64 == (k - 1) // 64      # ev[0] is the block event: token t is ev[t + 1]
    for ft in range(5):
        for ct in (0, 4, 2, 6):
            assert stat('f%d_c%d_130x67' % (ft, ct))[2] == {ft} and stat('f%d_c%d_1x1' % (ft, ct))[2] == {ft}
    assert {R.walk(d)[0][:2] for n, d in cases.items() if n[0] == 'f' and n[1].isdigit()} == {(1, 1), (70, 1), (3, 65), (64, 64), (67, 130)}


def test_fixture_equals_restatement_and_live_pillow():
    pytest.importorskip('PIL')
    z = np.load(GOLDEN)
    names = sorted(k[5:] for k in z.files if k.startswith('file_'))
    assert len(names) >= 12
    for name in names:
        d = z['file_' + name].tobytes()
        assert np.array_equal(z['l_' + name], R.decode(d)), name
        assert np.array_equal(z['l_' + name], R.pillow(d)), name


def test_fixture_is_what_pillow_writes_today():
    pytest.importorskip('PIL')
    z = np.load(GOLDEN)
    live = R.pillow_cases()
    for k in z.files:
        if k.startswith('file_'):
            assert np.array_equal(R.pillow(live[k[5:]]), z['l_' + k[5:]]), k


# ---- parse -------------------------------------------------------------------------------------------------------------------------------------
def test_parse_returns_what_pillow_reports(cases):
    from PIL import Image
    modes = {(0, 1): '1', (0, 8): 'L', (3, 1): 'P', (3, 2): 'P', (3, 4): 'P', (3, 8): 'P', (2, 8): 'RGB', (6, 8): 'RGBA', (4, 8): 'LA',
             (0, 2): 'L', (0, 4): 'L'}
    for name, d in cases.items():
        plan, im = pngdec.parse(d), Image.open(io.BytesIO(d))
        assert (plan.width, plan.height) == im.size, name
        assert modes[(plan.color_type, plan.depth)] == im.mode, name
        ihdr, plte, z, n = R.walk(d)
        assert plan.stream == z and plan.idat_chunks == n and plan.raw_size == len(zlib.decompress(z)), name
        if plan.color_type == 3:
            assert plan.palette.tobytes() == plte and im.getpalette() == list(plte), name
            assert np.array_equal(plan.ltable[:plan.entries], np.asarray(Image.fromarray(plan.palette[None]).convert('L'))[0]), name
    assert pngdec.parse(cases['large']).idat_chunks >= 4 and pngdec.parse(cases['z_flushes']).idat_chunks == 4


def test_parse_refuses_by_name():
    assert pngdec.Unsupported is jpegdec.Unsupported and issubclass(pngdec.Unsupported, ValueError)
    raw = bytes(5)
    good = R.png(4, 1, 8, 0, raw)
    assert pngdec.parse(good).size == (1, 4)
    with pytest.raises(pngdec.Unsupported, match='Adam7'):
        pngdec.parse(R.png(4, 1, 8, 0, raw, interlace=1))
    with pytest.raises(pngdec.Unsupported, match='16-bit'):
        pngdec.parse(R.png(4, 1, 16, 0, bytes(9)))
    with pytest.raises(pngdec.Unsupported, match='sides up to'):
        pngdec.parse(R.png(40000, 1, 8, 0, raw))
    with pytest.raises(pngdec.Unsupported, match='bytes a row'):
        pngdec.parse(R.png(pngdec.MAX_ROWBYTES // 4 + 1, 1, 8, 6, raw))

    def plain(exc):
        assert not isinstance(exc.value, pngdec.Unsupported)
    with pytest.raises(ValueError, match='signature') as e:
        pngdec.parse(b'\x89PNX' + good[4:])
    plain(e)
    bad = bytearray(good)
    bad[good.index(b'IDAT') + 5] ^= 1
    with pytest.raises(ValueError, match='CRC in the IDAT') as e:
        pngdec.parse(bytes(bad))
    plain(e)
    bad = bytearray(good)
    bad[good.index(b'IHDR') + 4 + 13] ^= 1
    with pytest.raises(ValueError, match='CRC in the IHDR'):
        pngdec.parse(bytes(bad))
    for cut in (len(good) - 1, len(good) - 12, good.index(b'IDAT') + 6, good.index(b'IDAT') - 2, 20):
        with pytest.raises(ValueError, match='ends') as e:
            pngdec.parse(good[:cut])
        plain(e)
    with pytest.raises(ValueError, match='no IDAT'):
        pngdec.parse(R.SIGNATURE + R.chunk(b'IHDR', struct.pack('>IIBBBBB', 4, 1, 8, 0, 0, 0, 0)) + R.chunk(b'IEND', b''))
    with pytest.raises(ValueError, match='IHDR'):
        pngdec.parse(R.SIGNATURE + R.chunk(b'IDAT', zlib.compress(raw)) + R.chunk(b'IEND', b''))
    with pytest.raises(ValueError, match='without PLTE'):
        pngdec.parse(R.png(4, 1, 8, 3, raw))
    for hdr in (b'\x79\x9c', b'\x88\x1c', b'\x78\xbb', b'\x78\x9d'):           # CM 9; window 64 KiB; preset dictionary; FCHECK
        with pytest.raises(ValueError, match='zlib header'):
            pngdec.parse(R.png(4, 1, 8, 0, zstream=hdr + zlib.compress(raw)[2:]))
    # an ancillary chunk is skipped, its CRC unread; tRNS is skipped
    anc = R.png(4, 1, 8, 0, raw, extra=b'\0\0\0\1tEXtA\0\0\0\0', trns=b'\0\1')
    assert pngdec.parse(anc).stream == pngdec.parse(good).stream
    with pytest.raises(TypeError):
        pngdec.parse('a.png')
    # several IDAT chunks are one stream
    assert pngdec.parse(R.png(4, 1, 8, 0, raw, split=3)).stream == zlib.compress(raw)


def test_decode_planes_refuses_before_any_launch():
    a, b = R.png(4, 1, 8, 0, bytes(5)), R.png(4, 2, 8, 0, bytes(10))
    with pytest.raises(ValueError, match='share one size'):
        pngdec.decode_planes([a, b])
    with pytest.raises(TypeError):
        pngdec.decode_planes(a)
    with pytest.raises(ValueError, match='at least one'):
        pngdec.decode_planes([])
    with pytest.raises(TypeError):
        pngdec.decode(12)
    with pytest.raises(pngdec.Unsupported):
        pngdec.decode_planes([a, R.png(4, 1, 8, 0, bytes(5), interlace=1)])


# ---- the entry points' argument checks ---------------------------------------------------------------------------------------------------------
def test_entry_points_return_minus_two():
    from maggie_amd import hip
    lib = hip.lib()
    vals = [ctypes.c_int(0) for _ in range(7)]
    assert lib.mg_pngdec_limits(*[ctypes.byref(v) for v in vals]) == 0
    assert [v.value for v in vals] == [pngdec.THREADS, pngdec.MAX_SIDE, pngdec.MAX_ROWBYTES, pngdec.REC_WORDS, pngdec.INFO_WORDS, pngdec.ROUND_TOKENS,
                                       pngdec.FLUSH_BYTES]
    assert lib.mg_pngdec_limits(None, *[ctypes.byref(v) for v in vals[1:]]) == -2
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p = ctypes.c_void_p
    L, I = ctypes.c_long, ctypes.c_int

    def inflate(data=base, nbytes=64, recs=base + 256, raw=base + 1024, stride=16, info=base + 512, planes=1, h=1, w=1):
        return lib.mg_pngdec_inflate(p(data), L(nbytes), p(recs), p(raw), L(stride), p(info), L(planes), I(h), I(w), None)

    def unfilter(raw=base + 1024, stride=16, recs=base + 256, out=base + 2048, info=base + 512, planes=1, h=1, w=1):
        return lib.mg_pngdec_unfilter(p(raw), L(stride), p(recs), p(out), p(info), L(planes), I(h), I(w), None)
    for kw in (dict(data=None), dict(recs=None), dict(raw=None), dict(info=None), dict(data=base + 1), dict(raw=base + 1028), dict(recs=base + 258),
               dict(nbytes=-1), dict(nbytes=pngdec.MAX_BYTES + 1), dict(stride=0), dict(stride=24), dict(stride=pngdec.MAX_RAW + 16), dict(planes=0),
               dict(h=0), dict(w=0), dict(h=pngdec.MAX_SIDE + 1), dict(w=pngdec.MAX_SIDE + 1)):
        assert inflate(**kw) == -2, kw
    for kw in (dict(raw=None), dict(recs=None), dict(out=None), dict(info=None), dict(out=base + 1024), dict(info=base + 514), dict(stride=8),
               dict(stride=40), dict(planes=-1), dict(h=0), dict(w=-3), dict(h=pngdec.MAX_SIDE + 1)):
        assert unfilter(**kw) == -2, kw
    assert inflate(planes=1 << 31) == -3 and unfilter(planes=1 << 31) == -3


# ---- the kernel source on the host, under the sanitizers ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def host_exe(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path_factory.mktemp('pngdec_host') / 'pngdec_host')
    subprocess.check_call(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                           '-fno-strict-aliasing', '-pthread', '-o', exe, os.path.join(ROOT, 'tests', 'csrc', 'pngdec_host.cpp')])
    return exe


def _case(plans, front=0):
    """One launch of the host program: the streams of `plans` concatenated behind `front` bytes, so that offsets are odd."""
    h, w = plans[0].size
    blob, recs = b'\x5a' * front, []
    for pl in plans:
        recs.append(pngdec.record(pl, len(blob)))
        blob += pl.stream
    return struct.pack('<4i', h, w, len(plans), len(blob)) + np.stack(recs).tobytes() + blob


def _run_host(exe, tmp_path, cases, shapes, tag):
    src, dst = str(tmp_path / (tag + '.in')), str(tmp_path / (tag + '.out'))
    with open(src, 'wb') as f:
        f.write(struct.pack('<i', len(cases)) + b''.join(cases))
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'pngdec_host: ok' in r.stdout and not r.stderr.strip(), (r.stdout + r.stderr)[-3000:]
    out, buf, p = [], open(dst, 'rb').read(), 0
    for (P, h, w) in shapes:
        rc1, rc2, stride, nout = struct.unpack_from('<4i', buf, p)
        p += 16
        info = np.frombuffer(buf, np.int32, P * pngdec.INFO_WORDS, p).reshape(P, -1)
        p += 4 * P * pngdec.INFO_WORDS
        raw = np.frombuffer(buf, np.uint8, P * stride, p).reshape(P, stride)
        p += P * stride
        assert nout == P * h * w
        img = np.frombuffer(buf, np.uint8, nout, p).reshape(P, h, w)
        p += nout
        out.append((rc1, rc2, info, raw, img))
    assert p == len(buf)
    return out


def test_host_build_reproduces_the_restatement(host_exe, tmp_path, cases, restated):
    names = list(cases)
    plans = {n: pngdec.parse(cases[n]) for n in names}
    # every file alone (at offset 1, 2, 3, 0, ...), and the files of one size together: colour types mixed in one launch
    groups = [[n] for n in names]
    by_size = {}
    for n in names:
        by_size.setdefault(plans[n].size, []).append(n)
    groups += [g for g in by_size.values() if len(g) > 1]
    res = _run_host(host_exe, tmp_path, [_case([plans[n] for n in g], front=(k + 1) % 4) for k, g in enumerate(groups)],
                    [(len(g),) + plans[g[0]].size for g in groups], 'list')
    assert any(len({plans[n].color_type for n in g}) > 1 for g in groups)
    for g, (rc1, rc2, info, raw, img) in zip(groups, res):
        assert rc1 == 0 and rc2 == 0, g
        for k, n in enumerate(g):
            want_raw, want_img, rounds = restated[n]
            assert info[k, 0] == 0, (n, info[k])
            assert raw[k, :len(want_raw)].tobytes() == want_raw, n
            assert (raw[k, len(want_raw):] == 0xA5).all(), n    # nothing written behind the file's bytes
            assert np.array_equal(img[k], want_img), n
            assert info[k, 1] == rounds, (n, info[k, 1], rounds)
            assert info[k, 4] == info[k, 5] and (int(info[k, 4]) & 0xffffffff) == zlib.adler32(want_raw), n


def test_host_build_on_a_stored_block_behind_a_huffman_block_at_a_refill(host_exe, tmp_path):
    """The stage of the compressed bytes (4 096 of them) is refilled in front of a block header when fewer than 648 are left in it; a stored
    block then hands the whole bytes in the bit reader back. Swept so that the refill falls on the stored header at every bit phase, at every
    count of bytes held and at stream offsets 0..3; an empty stored block (what Z_SYNC_FLUSH writes) in between for half of them."""
    files, fronts = [], []
    for li, literals in enumerate(range(130, 400, 13)):        # 3 328 + literals bytes consumed: 3 458 .. 3 727, around the refill point 3 448
        for nine in range(8):
            for empty in (0, 1):
                files.append(R.huffman_then_stored(3328, literals, nine, empty))
                fronts.append((li + nine) % 4)                 # 13 is 1 mod 4: every (byte phase, offset) pair occurs
    plans = [pngdec.parse(d) for d in files]
    res = _run_host(host_exe, tmp_path, [_case([pl], front=f) for pl, f in zip(plans, fronts)], [(1,) + pl.size for pl in plans], 'refill')
    for k, (pl, (rc1, rc2, info, raw, img)) in enumerate(zip(plans, res)):
        want = zlib.decompress(pl.stream)
        assert rc1 == 0 and rc2 == 0 and info[0, 0] == 0, (k, info[0])
        assert raw[0, :len(want)].tobytes() == want and info[0, 2] == 3 + (k % 2), k
    d = files[5]
    assert np.array_equal(R.decode(d), R.pillow(d))


def _hostile(plan, stream):
    q = pngdec.PngPlan(**plan.__dict__)
    q.stream = stream
    return q


def _lying_headers():
    """Dynamic block headers that zlib refuses: HLIT 287+, HDIST 31+, an over-subscribed and an incomplete code length code, a repeat with
    nothing before it, a repeat past the last length, no end-of-block code, an over-subscribed and an incomplete literal/length set."""
    out = []

    def start(hlit=0, hdist=0, clens=None):
        bw = R.BitWriter()
        bw.bits(0x78, 8); bw.bits(0x01, 8); bw.bits(1, 1); bw.bits(2, 2)
        bw.bits(hlit, 5); bw.bits(hdist, 5); bw.bits(15, 4)
        for s in R.CL_ORDER:
            bw.bits((4 if s < 16 else 0) if clens is None else clens[s], 3)
        return bw

    def finish(bw):
        bw.bits(0, 64)
        return bytes(bw.out) + b'\0\0\0\1'
    out.append(finish(start(hlit=30)))                         # HLIT = 287
    out.append(finish(start(hdist=30)))                        # HDIST = 31
    out.append(finish(start(clens=[1, 1, 1] + [0] * 16)))      # over-subscribed code length code
    out.append(finish(start(clens=[2, 2, 2] + [0] * 16)))      # incomplete code length code
    bw = start(clens=[3, 3, 3, 3, 3, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0])    # eight 3-bit codes: lengths 0..6 and repeat-previous
    bw.code(7, 3)                                              # the repeat code first: nothing before it
    out.append(finish(bw))
    bw = start(clens=[3, 3, 3, 3, 3, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3])    # lengths 0..6 and the long zero run
    for _ in range(3):
        bw.code(7, 3); bw.bits(127, 7)                         # 3 x 138 zeros > 258 lengths
    out.append(finish(bw))
    bw = start()
    for _ in range(258):
        bw.code(8 if _ < 256 else 0, 4)                        # 256 literals of 8 bits, no end-of-block code
    out.append(finish(bw))
    bw = start()
    for _ in range(258):
        bw.code(7 if _ < 257 else 1, 4)                        # 257 codes of 7 bits: over-subscribed
    out.append(finish(bw))
    bw = start()
    for _ in range(258):
        bw.code(9 if _ < 257 else 1, 4)                        # 257 codes of 9 bits: incomplete
    out.append(finish(bw))
    return out


def test_host_build_stays_clean_on_hostile_streams(host_exe, tmp_path, cases, restated):
    streams = []                                               # (plan, stream)
    for name in ('l_smooth', 'wrap', 'far_match', 'l_stored'):
        pl = pngdec.parse(cases[name])
        for q in (4, 2):
            for k in (1, 3) if q == 4 else (1,):
                streams.append((pl, pl.stream[:len(pl.stream) * k // q]))
    short = pngdec.parse(cases['p_bits2'])                     # a dynamic block in a short stream: every single-byte flip
    assert ('block', 2, 1) in list(R.tokens(short.stream)) and len(short.stream) < 400
    for i in range(2, len(short.stream)):
        for bit in (1, 0x80, 0xff):
            s = bytearray(short.stream)
            s[i] ^= bit
            streams.append((short, bytes(s)))
    fixed = pngdec.parse(cases['l_flat'])
    for i in range(2, len(fixed.stream)):
        s = bytearray(fixed.stream)
        s[i] ^= 0x55
        streams.append((fixed, bytes(s)))
    one = pngdec.parse(R.png(16, 16, 8, 0, bytes(16 * 17)))
    streams += [(one, s) for s in _lying_headers()]
    first = len(streams)
    streams.append((one, R.fixed_stream([('lit', 1), ('match', 200, 2), ('lit', 0), ('match', 70, 1)], b'')))      # a distance beyond the start
    streams.append((one, R.fixed_stream([('lit', 0)] * 16 * 17 + [('lit', 0)], bytes(16 * 17 + 1))))               # one byte more
    streams.append((one, R.fixed_stream([('lit', 0)] * (16 * 17 - 1), bytes(16 * 17 - 1))))                        # one byte fewer
    streams.append((one, b'\x78\x01\x07' + bytes(8)))                                                              # the reserved block type
    streams.append((one, b'\x78\x01\x01\x10\x01\x10\x01' + bytes(300)))                                            # LEN == NLEN
    res = _run_host(host_exe, tmp_path, [_case([_hostile(pl, s)], front=k % 4) for k, (pl, s) in enumerate(streams)],
                    [(1,) + pl.size for pl, _ in streams], 'hostile')
    differ = []
    for k, ((pl, s), (rc1, rc2, info, raw, img)) in enumerate(zip(streams, res)):
        assert rc1 == 0 and rc2 == 0
        status = int(info[0, 0])
        try:
            want = R.inflate(s, pl.raw_size)
            rows = R.unfilter(want, pl.height, pl.rowbytes, max(1, R.CHANNELS[pl.color_type] * pl.depth // 8))
            want_img = R.to_l(rows, pl.width, pl.color_type, pl.depth, None if pl.palette is None else pl.palette.tobytes())
        except R.Corrupt as e:
            assert status != 0, (len(s), e)
            if not status & e.status:
                differ.append((k, len(s), status, e.status, str(e)))
            continue
        # a flip that zlib and the restatement accept: an output of the right shape, and the right one
        assert status == 0 and raw[0, :len(want)].tobytes() == want and np.array_equal(img[0], want_img)
    tail = [int(r[2][0, 0]) for r in res[first:]]
    assert tail[0] & R.DISTANCE and tail[1] & R.SIZE and tail[2] & R.SIZE and tail[3] & R.BLOCK_TYPE and tail[4] & R.STORED_LEN, tail
    assert all(int(r[2][0, 0]) & R.CODE_SET for r in res[first - 9:first]), [int(r[2][0, 0]) for r in res[first - 9:first]]
    assert any(int(r[2][0, 0]) & R.ADLER for r in res) and any(int(r[2][0, 0]) & R.PAST_END for r in res)
    assert not differ, differ
