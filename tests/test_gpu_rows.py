"""The device-row-count kernels of the sparse head against float64, one kernel at a time.

Every kernel that takes `rows=` re-derives its loop bounds, its rows per block and (BatchNorm) its sample count from an int32 device word. Each
test here runs one such kernel through kernels.py on a (cap, C) buffer whose rows from `live` on are NaN, whose rows 0 and live - 1 carry
16 x outliers, and whose `out=` buffers carry sentinel guard rows, for the row-count words -3, 0, 1, 5, 257, cap - 1, cap, cap + 1000 and
for rows=None -- ONE device word rewritten in place between the calls, as a graph replay does. The references, the case construction and the
element-wise comparison |got - ref| <= u_out |ref| + u32 k S live in tests/rows_reference.py; tests/test_rows_reference_cpu.py proves on the
host that this comparison rejects a dropped last row, an added dead row, a divisor taken from the capacity, a shifted row and a two-unit error.
Pure sums run on exact-integer inputs and are compared bit for bit.

Capacities: 777 (ragged, fewer rows than row blocks), 20 000 x 64 (wraps the 512 x 32-row grid of the LayerNorm backward), 2 500 x 512 in
16-bit (64 lanes per row), 70 001 x 64 (wraps the 2048-block LayerNorm forward grid and the column-statistics row blocks), 140 000 x 64
(wraps the 4096-block grid of the element-wise kernels; the gather's own grid has 8192 blocks: 270 000 x 64 wraps that one).

Measured err / (u32 S) on the MI355X (largest over all cases of this file; the 16-bit outputs are absorbed by u_out and read 0) and the k in use
(rows_reference.K_*; sum(n) = ceil(log2 n) + 8):

    kernel / output                      measured   k
    rows_sigmoid_mul, bwd da                1.22    K_SIGMUL 8
    rows_sigmoid_mul_bwd dg                 0.61    K_SIGMUL_BWD 12
    rows_add (also in place)                0.50    K_ADD 1
    rows_dropout                            0.67    K_DROPOUT 2
    affine_act (also yoff)                  1.11    K_AFFINE 5
    gather_rows with mul                    0.50    K_GATHER 1 (without mul: a copy, compared with equality)
    layernorm y / mean / rstd               0.52 / 0.82 / 0.41    K_LN_Y 44 / K_LN_MEAN 16 / K_LN_RSTD 40
    layernorm dz                            1.03    K_LN_DZ 32
    layernorm dgamma                        1.21    sum(n) + K_XHAT 3            (12 .. 28)
    layernorm dbeta                         1.01    sum(n)                       (9 .. 25)
    bn_train_fwd mean, running_mean         3.48, 2.58    sum(n) + K_BN_MEAN 8   (17 .. 33)
    bn_train_fwd shift                      1.86    sum(n) + K_BN_SHIFT 24       (33 .. 49)
    bn_train_fwd invstd, scale              5.76, 5.88 (one-pass form; two-pass 1.66, 1.74)    sum(n) + K_BN_VAR 48 (57 .. 73)
    bn_train_fwd running_var                12.39 (one-pass form; two-pass 2.43)               sum(n) + K_BN_VAR 48
    bn_train_fwd y                          1.02    sum(n) + K_BN_SHIFT + K_BN_Y (37 .. 53)
    colstats centred squares                5.53    sum(n) + K_CENSQ 16          (25 .. 41)
    bn sum g (train_bwd, reduce_only)       2.15    sum(n) + 1                   (10 .. 26)
    bn sum g * xhat                         5.08    sum(n) + K_SUM_GX 12         (21 .. 37)
    bn_train_bwd dx                         1.70    sum(n) + K_BN_DX 12
    bn_backward apply dx, linked dx         1.82, 1.42    K_BN_DX 12 (+ 1)
    bn dres                                 0.60    1
    bias_act_bwd db                         1.12    sum(n)                       (9 .. 25)

The k of the element-wise outputs (the first block, LayerNorm's y / mean / rstd / dz included) are operation counts of the longest path and were NOT
fitted to the measurements: K_LN_Y and K_LN_RSTD stand 85 and 98 times above what was observed, because the count follows the whole chain x + r ->
mean -> variance -> rsqrtf while S already carries the condition of v - mean. For a 16-bit output u_out |ref| dominates either way.

The k of every column sum of rounded products (dgamma, dbeta, centred squares, sum g, sum g * xhat, db, the BatchNorm statistics) lies between 4 x
and 64 x the ratio measured for it. The one-pass figures belong to deterministic mode with 16-bit storage and to rows=None, where the variance is
E[x^2] - E[x]^2 in fp32; S of the variance is then <x^2> + mean^2. The exact-integer sums (LayerNorm dbeta, bias db, BatchNorm sum g, the column
sum and sum of squares of the statistics scratch, the gather's ddense and dmul) have no k: they are compared with equality.

Run time on the MI355X: the 170 cases take 63 s together; the slowest are bn_backward at 70 001 x 64 (4.0 s), sigmoid-multiply at 140 000 x 64 (3.6 s)
and the gather at 270 000 x 64 (2.9 s), every other case stays below 3 s. Most of that is the float64 reference on the host, built once per distinct
live count of a case (_memo) and shared by the count words and summation modes that use it.

affine_act with yoff was checked on the device: rows live .. cap - 1 of its `out=` buffer and the columns next to the slice keep their bits, like
those of rows_add and gather_rows, so the assertion stands for all three.
"""
import contextlib

import numpy as np
import pytest
import torch

import rows_reference as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
EPS, MOM, SLOPE = 1e-5, 0.1, 0.2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


def _id(g):
    return '%dx%d-%s' % (g[0], g[1], str(g[2]).replace('torch.', ''))


def _geoms(*extra):
    gs = [(777, 8, BF16), (777, 8, F16)]                    # C = 8 in 16-bit only: fp32 needs C % 4 == 0 and two lanes per row are enough
    gs += [(777, C, dt) for C in (32, 64) for dt in (BF16, F16, F32)]
    return gs + list(extra)


ELEMENTWISE = _geoms((140000, 64, F16))
LAYERNORM = _geoms((20000, 64, BF16), (20000, 64, F16), (20000, 64, F32), (2500, 512, BF16), (2500, 512, F16), (70001, 64, BF16))
COLUMNS = _geoms((20000, 64, F32), (70001, 64, BF16))
GATHER = ELEMENTWISE + [(270000, 64, BF16)]              # 262 144 rows x 8 chunks fill the gather's 8192 blocks: this one wraps them


@contextlib.contextmanager
def _mode(det):
    from maggie_amd import hip
    was = hip.DETERMINISTIC
    hip.set_deterministic(det)
    try:
        yield
    finally:
        hip.set_deterministic(was)


def _words(cap):
    """(word value or None, live rows) for every count of a case."""
    return [(v, R.clamp_live(v, cap)) for v in R.live_counts(cap) + [None]]


def _set(rows, v):
    if v is None:
        return None
    rows.fill_(v)
    return rows


def _f32(C, seed, lo=0.5, hi=1.5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(C, generator=g) * (hi - lo) + lo).float()


def _memo(build):
    """build(live) with the last result kept: the words cap, cap + 1000 and None share one set of operands and references."""
    last = {}

    def get(*key):
        if key not in last:
            last.clear()
            last[key] = build(*key)
        return last[key]
    return get


def _same_as_cap(store, key, v, *tensors):
    """rows=None must give the bits of rows=cap (same inputs: live == cap for both)."""
    if v is not None and v == store.get('cap'):
        store[key] = [t.detach().cpu().clone() for t in tensors]
    if v is None:
        for a, b in zip(store[key], tensors):
            assert torch.equal(R.bits_of(a), R.bits_of(b)), key


# ------------------------------------------------------------------------------------------------------------------
# rows.hip: sigmoid-multiply, add, dropout
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('geom', ELEMENTWISE, ids=_id)
def test_sigmoid_mul_rows(geom):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    a0, g0, d0 = R.base_rows(cap, 2 * C, 1), R.base_rows(cap, C, 2), R.base_rows(cap, C, 3)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    store = {'cap': cap}

    @_memo
    def case(live):
        wide = R.rows_input(a0, live, dtype)
        g, d = R.rows_input(g0, live, dtype), R.rows_input(d0, live, dtype)
        return wide, g, d, R.sigmoid_mul(wide[:live, :C], g[:live]), R.sigmoid_mul_bwd(d[:live], wide[:live, :C], g[:live])

    for v, live in _words(cap):
        rw = _set(rows, v)
        wide, g, d, ref_fwd, ((rda, sda), (rdg, sdg)) = case(live)
        a = wide.to(dev)[:, :C]                                       # a channel slice: lda = 2C
        gd, dd = g.to(dev), d.to(dev)
        out = K.rows_sigmoid_mul(a, gd, rows=rw)
        R.check(out[:live], *ref_fwd, R.K_SIGMUL, dtype, 'rows_sigmoid_mul')
        da, dg = K.rows_sigmoid_mul_bwd(dd, a, gd, rows=rw)
        R.check(da[:live], rda, sda, R.K_SIGMUL, dtype, 'rows_sigmoid_mul_bwd da')
        R.check(dg[:live], rdg, sdg, R.K_SIGMUL_BWD, dtype, 'rows_sigmoid_mul_bwd dg')
        _same_as_cap(store, 'sig', v, out, da, dg)


@pytest.mark.parametrize('geom', ELEMENTWISE, ids=_id)
def test_rows_add_rows(geom):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    a0, b0 = R.base_rows(cap, 2 * C, 1), R.base_rows(cap, C, 4)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    store = {'cap': cap}

    @_memo
    def case(live):
        wide, b = R.rows_input(a0, live, dtype), R.rows_input(b0, live, dtype)
        return wide, b, R.add(wide[:live, :C], b[:live]), R.add(wide[:live, C:], b[:live])

    for v, live in _words(cap):
        rw = _set(rows, v)
        wide, b, ref_add, ref_add2 = case(live)
        a = wide.to(dev)[:, :C]                                       # a channel slice: lda = 2C
        bd = b.to(dev)
        # a + b into a guarded buffer
        before = R.guarded(cap, C, dtype)
        buf = before.to(dev)
        K.rows_add(a, bd, out=buf[:cap], rows=rw)
        R.check(buf[:live], *ref_add, R.K_ADD, dtype, 'rows_add')
        assert R.untouched(buf, before, live), ('rows_add wrote outside the live rows', v)
        # in place on a channel slice of a wider guarded buffer (out = a), the way the head accumulates a gradient with two consumers
        before2 = R.guarded(cap, 2 * C, dtype)
        before2[:live] = wide[:live]                                # the dead rows keep the sentinel: NaN + NaN would hide a write there
        buf2 = before2.to(dev)
        K.rows_add(buf2[:cap, C:], bd, out=buf2[:cap, C:], rows=rw)
        R.check(buf2[:live, C:], *ref_add2, R.K_ADD, dtype, 'rows_add in place')
        assert R.untouched(buf2, before2, live, cols=(C, 2 * C)), ('rows_add (in place) wrote outside its slice', v)
        _same_as_cap(store, 'add', v, buf, buf2)


@pytest.mark.parametrize('geom', ELEMENTWISE, ids=_id)
def test_dropout_mask_does_not_depend_on_the_count(geom):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    p = 0.25
    x0 = R.base_rows(cap, C, 5, std=0.5, offset=3.0)               # no zeros: a zero in the output is a dropped element
    state = torch.tensor([20240229, 17], dtype=torch.int64, device=dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    full = R.rows_input(x0, cap, dtype)
    keep_all = R.dropout_keep(K.rows_dropout(full.to(dev), p, state, 3, rows=None))
    assert 0.70 < float(keep_all.double().mean()) < 0.80 or cap * C < 10000
    for v, live in _words(cap):
        rw = _set(rows, v)
        x = R.rows_input(x0, live, dtype)
        y = K.rows_dropout(x.to(dev), p, state, 3, rows=rw)
        keep = R.dropout_keep(y[:live])
        assert torch.equal(keep, keep_all[:live]), v               # the hash index is the element's, whatever the count
        ref = torch.where(keep, x[:live].double() / (1 - p), torch.zeros((), dtype=torch.float64))
        R.check(y[:live], ref, ref.abs(), R.K_DROPOUT, dtype, 'rows_dropout')


# ------------------------------------------------------------------------------------------------------------------
# rows.hip: residual + LayerNorm
# ------------------------------------------------------------------------------------------------------------------
LN_CASES = [(g, False) for g in LAYERNORM] + [(g, True) for g in LAYERNORM if g[:2] == (777, 64)]


@pytest.mark.parametrize('geom,offset', LN_CASES, ids=[_id(g) + ('-offset100' if o else '') for g, o in LN_CASES])
def test_add_layernorm_forward_backward(geom, offset):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    if offset:                                                      # x + r near 100, spread near 1: the variance must be the two-pass form
        x0, r0 = R.base_rows(cap, C, 6, std=0.7, offset=60.0), R.base_rows(cap, C, 7, std=0.7, offset=40.0)
    else:
        x0, r0 = R.base_rows(cap, C, 6), R.base_rows(cap, C, 7)
    dy0, dyi0 = R.base_rows(cap, C, 8), R.base_int_rows(cap, C, 9)
    gamma, beta = _f32(C, 10), _f32(C, 11, -1.0, 1.0)
    gd, bd = gamma.to(dev), beta.to(dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    store = {'cap': cap}

    @_memo
    def case(live):
        x, r, dy = (R.rows_input(t, live, dtype) for t in (x0, r0, dy0))
        dyi = R.rows_input(dyi0, live, dtype, outlier=8)
        fwd = R.layernorm(x[:live], r[:live], gamma, beta, EPS)
        # the backward takes the reference's statistics as fp32 operands, dead rows of rstat poisoned
        st = torch.full((cap, 2), float('nan'))
        st[:live, 0], st[:live, 1] = fwd[1][0].float(), fwd[2][0].float()
        return x, r, dy, dyi, fwd, st, R.layernorm_bwd(dy[:live], x[:live], r[:live], gamma, st[:live, 0], st[:live, 1])

    for v, live in _words(cap):
        rw = _set(rows, v)
        x, r, dy, dyi, ((ry, sy), (rmean, smean), (rrstd, srstd)), st, ((rdz, sdz), (rdg, sdg), (rdb, sdb)) = case(live)
        xd, rd = x.to(dev), r.to(dev)
        y, rstat = K.rows_add_layernorm(xd, rd, gd, bd, EPS, rows=rw)
        R.check(y[:live], ry, sy, R.K_LN_Y, dtype, 'layernorm y')
        R.check(rstat[:live, 0], rmean, smean, R.K_LN_MEAN, F32, 'layernorm mean')
        R.check(rstat[:live, 1], rrstd, srstd, R.K_LN_RSTD, F32, 'layernorm rstd')
        isum = dyi[:live].double().sum(0)
        R.assert_exact_conditions(dyi[:live], partial_bound=float(dyi[:live].double().abs().sum(0).max()) if live else 0.0)
        for det in (True, False):
            with _mode(det):
                dz, dgm, dbt = K.rows_add_layernorm_bwd(dy.to(dev), xd, rd, gd, st.to(dev), rows=rw)
                dbi = K.rows_add_layernorm_bwd(dyi.to(dev), xd, rd, gd, st.to(dev), rows=rw)[2].clone()
            R.check(dz[:live], rdz, sdz, R.K_LN_DZ, dtype, 'layernorm dz')
            if live == 0:
                assert not dgm.any() and not dbt.any() and not dbi.any()           # exact zeros
            else:
                R.check(dgm, rdg, sdg, R.sum_k(live) + R.K_XHAT, F32, 'layernorm dgamma')
                R.check(dbt, rdb, sdb, R.sum_k(live), F32, 'layernorm dbeta')
            R.exact(dbi, isum, 'layernorm dbeta (integers)')
            if det:
                _same_as_cap(store, 'ln', v, y, rstat, dz, dgm, dbt)


# ------------------------------------------------------------------------------------------------------------------
# norm_act.hip: affine + activation, BatchNorm, bias backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY])
@pytest.mark.parametrize('geom', ELEMENTWISE, ids=_id)
def test_affine_act_rows(geom, act):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    x0, r10, r20 = R.base_rows(cap, C, 12), R.base_rows(cap, 2 * C, 13), R.base_rows(cap, C, 14)
    scale, shift = _f32(C, 15), _f32(C, 16, -1.0, 1.0)
    sd, hd = scale.to(dev), shift.to(dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    store = {'cap': cap}

    @_memo
    def case(live):
        x, r1w, r2 = (R.rows_input(t, live, dtype) for t in (x0, r10, r20))
        r1 = r1w[:, C:]
        return (x, r1w, r2, R.affine_act(x[:live], scale, shift, r1[:live], None, act, SLOPE),
                R.affine_act(x[:live], scale, shift, r1[:live], r2[:live], act, SLOPE))

    for v, live in _words(cap):
        rw = _set(rows, v)
        x, r1w, r2, ref1, ref2 = case(live)
        xd, r1d, r2d = x.to(dev), r1w.to(dev)[:, C:], r2.to(dev)   # res is a channel slice (ldr = 2C)
        # res, into a guarded buffer of its own
        before = R.guarded(cap, C, dtype)
        buf = before.to(dev)
        K.affine_act(xd, sd, hd, res=r1d, act=act, slope=SLOPE, out=buf[:cap], rows=rw)
        R.check(buf[:live], *ref1, R.K_AFFINE, dtype, 'affine_act')
        assert R.untouched(buf, before, live), ('affine_act wrote outside the live rows', v)
        # res and res2, into the upper channel slice of a wider guarded buffer (yoff = C)
        before2 = R.guarded(cap, 2 * C, dtype)
        buf2 = before2.to(dev)
        K.affine_act(xd, sd, hd, res=r1d, res2=r2d, act=act, slope=SLOPE, out=buf2[:cap], yoff=C, rows=rw)
        R.check(buf2[:live, C:], *ref2, R.K_AFFINE, dtype, 'affine_act yoff')
        assert R.untouched(buf2, before2, live, cols=(C, 2 * C)), ('affine_act (yoff) wrote outside its slice', v)
        _same_as_cap(store, 'aff', v, buf, buf2)


def _bn_operands(cap, C):
    g = torch.Generator().manual_seed(21)
    return (_f32(C, 17), _f32(C, 18, -1.0, 1.0), torch.randn(C, generator=g).float(), (torch.rand(C, generator=g) + 0.5).float())


@pytest.mark.parametrize('apply', [True, False], ids=['apply', 'stats'])
@pytest.mark.parametrize('count_mult', [1, 3])
@pytest.mark.parametrize('geom', COLUMNS, ids=_id)
def test_bn_train_fwd_rows(geom, count_mult, apply):
    """scale | shift | mean | invstd, the running statistics (unbiased over live * count_mult samples) and y against float64 batch_norm over
    x[:live]. The statistics scratch handed in as `stats_ws` is read back: with a device row count it holds [sum | centred squares] (two-pass
    form), in deterministic mode with 16-bit storage one [sum | sum of squares] row per row block (one-pass form) -- on integer inputs the plain
    sums are exact.
    The unbiased factor of the running variance is that of live * count_mult samples in every mode."""
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    x0, res0, xi0 = R.base_rows(cap, C, 19, std=2.0, offset=1.0), R.base_rows(cap, C, 20), R.base_int_rows(cap, C, 22)
    gamma, beta, rm0, rv0 = _bn_operands(cap, C)
    gd, bd = gamma.to(dev), beta.to(dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    act = R.ACT_LEAKY

    @_memo
    def case(live):
        return R.rows_input(x0, live, dtype), R.rows_input(res0, live, dtype), R.rows_input(xi0, live, dtype, outlier=8)

    @_memo
    def reference(live, one_pass):
        x, res, _ = case(live)
        return R.batchnorm(x[:live], gamma, beta, rm0, rv0, MOM, EPS, count_mult, res[:live] if apply else None, act, SLOPE, one_pass=one_pass)

    for v, live in _words(cap):
        rw = _set(rows, v)
        x, res, xi = case(live)
        xs = xi[:live].double()
        R.assert_exact_conditions(xi[:live], partial_bound=float((xs * xs).sum(0).max()) if live else 0.0)
        for det in (True, False):
            one_pass = v is None or (det and dtype != F32)
            with _mode(det):
                n_ws = max(K.stats_ws_floats(C, True), K.stats_ws_floats(C, False))
                ws = torch.zeros(n_ws, device=dev)
                rm, rv = rm0.to(dev), rv0.to(dev)
                y, outs = K.bn_train_fwd(x.to(dev), gd, bd, rm, rv, MOM, EPS, act, SLOPE, res=res.to(dev) if apply else None, stats_ws=ws,
                                         rows=rw, count_mult=count_mult, apply=apply)
                wsi = torch.zeros(n_ws, device=dev)
                if v is not None:
                    K.bn_train_fwd(xi.to(dev), gd, bd, rm0.to(dev), rv0.to(dev), MOM, EPS, act, SLOPE, stats_ws=wsi, rows=rw, apply=False)
            outs = outs.cpu().reshape(4, C)
            if live == 0:                                              # no live row: identity statistics, running statistics untouched
                assert torch.equal(outs[0], gamma) and torch.equal(outs[1], beta) and not outs[2].any() and torch.equal(outs[3], torch.ones(C))
                assert torch.equal(R.bits_of(rm), R.bits_of(rm0)) and torch.equal(R.bits_of(rv), R.bits_of(rv0))
                assert not wsi.any()
                continue
            ref = reference(live, one_pass)
            kk = R.sum_k(live)
            tag = ' (one pass)' if one_pass else ''
            for i, (name, extra) in enumerate((('scale', R.K_BN_VAR), ('shift', R.K_BN_SHIFT), ('mean', R.K_BN_MEAN), ('invstd', R.K_BN_VAR))):
                R.check(outs[i], *ref[name], kk + extra, F32, 'bn_train_fwd ' + name + tag)
            R.check(rm, *ref['running_mean'], kk + R.K_BN_MEAN, F32, 'bn_train_fwd running_mean' + tag)
            R.check(rv, *ref['running_var'], kk + R.K_BN_VAR, F32, 'bn_train_fwd running_var' + tag)
            if live == 1:                                              # one sample: the variance is exactly 0
                want = torch.full((C,), EPS, dtype=torch.float64).rsqrt()
                R.check(outs[3], want, want, 8, F32, 'bn_train_fwd invstd of one row')
            if apply:
                R.check(y[:live], *ref['y'], kk + R.K_BN_SHIFT + R.K_BN_Y, dtype, 'bn_train_fwd y' + tag)
            else:
                assert y is None
            if v is None:
                continue
            if det and dtype != F32:                                   # one row [sum | sum of squares] per row block
                tot = wsi.cpu().double().reshape(-1, 2 * C).sum(0)
                R.exact(tot[:C].float(), xs.sum(0), 'colstats sum (integers)')
                R.exact(tot[C:].float(), (xs * xs).sum(0), 'colstats sum of squares (integers)')
            else:                                                      # [sum | centred squares]
                R.exact(wsi[:C], xs.sum(0), 'colstats sum (integers, two-pass)')
                iref = R.batchnorm(xs, gamma, beta, rm0, rv0, MOM, EPS)
                R.check(wsi[C:2 * C], *iref['censq'], R.sum_k(live) + R.K_CENSQ, F32, 'colstats centred squares')


@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_LEAKY])
@pytest.mark.parametrize('geom', COLUMNS, ids=_id)
def test_bn_backward_rows(geom, act):
    """bn_train_bwd (one call) and bn_backward as reduce_only + apply_only (the synchronised form of the head, with and without a global count)
    against float64 over the live rows. The divisor is the live count -- bn_train_bwd's wrapper passes count = M, bn_backward's callers pass
    count = 1.0, and the kernels must ignore both when a row-count word is given."""
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    x0, y0, dy0, dyi0 = R.base_rows(cap, C, 23, std=2.0, offset=1.0), R.base_rows(cap, C, 24), R.base_rows(cap, C, 25), R.base_int_rows(cap, C, 26)
    gamma, beta, rm0, rv0 = _bn_operands(cap, C)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)

    @_memo
    def case(live):
        x, y, dy = (R.rows_input(t, live, dtype) for t in (x0, y0, dy0))
        dyi = R.rows_input(dyi0, live, dtype, outlier=8)
        R.assert_exact_conditions(dyi[:live], partial_bound=float(dyi[:live].double().abs().sum(0).max()) if live else 0.0)
        if live:
            f = R.batchnorm(x[:live], gamma, beta, rm0, rv0, MOM, EPS)
            pack = torch.stack([f[n][0].float() for n in ('scale', 'shift', 'mean', 'invstd')])
        else:
            pack = torch.stack([gamma, beta, torch.zeros(C), torch.ones(C)])
        scale, _, mean, invstd = pack
        ref = R.batchnorm_bwd(dy[:live], y[:live], x[:live], scale, mean, invstd, act, SLOPE, n=max(live, 1))
        # sums that are NOT the local ones (a synchronised layer applies the global sums), with and without a global count
        glob = torch.cat([ref['sum_g'][0] * 2 + 1, ref['sum_gx'][0] * 2 - 1]).float()
        ref2 = {n_glob: R.batchnorm_bwd(dy[:live], y[:live], x[:live], scale, mean, invstd, act, SLOPE, n=n_glob or max(live, 1), sums=(glob[:C], glob[C:]))
                for n_glob in (None, float(2 * live + 3))}
        # the linked form: g arrives masked, the sums as replicas
        ref3 = R.batchnorm_bwd(dy[:live], None, x[:live], scale, mean, invstd, n=max(live, 1), sums=(glob[:C], glob[C:]))
        return x, y, dy, dyi, pack, ref, glob, ref2, ref3

    for v, live in _words(cap):
        rw = _set(rows, v)
        x, y, dy, dyi, pack, ref, glob, ref2s, ref3 = case(live)
        pd = pack.reshape(-1).to(dev)
        xd, yd, dyd = x.to(dev), y.to(dev), dy.to(dev)
        kk = R.sum_k(live)
        for det in (True, False):
            with _mode(det):
                dx, dres, sums = K.bn_train_bwd(dyd, yd, xd, pd, act, SLOPE, want_dres=True, rows=rw)
                sums_i = K.bn_train_bwd(dyi.to(dev), yd, xd, pd, R.ACT_NONE, SLOPE, rows=rw)[2].clone()
                _, _, local = K.bn_backward(dyd, yd, xd, pd[:C], pd[2 * C:3 * C], pd[3 * C:], 1.0, act=act, slope=SLOPE, reduce_only=True, rows=rw)
            R.check(dx[:live], *ref['dx'], kk + R.K_BN_DX, dtype, 'bn_train_bwd dx')
            R.check(dres[:live], *ref['dres'], 1, dtype, 'bn_train_bwd dres')
            for s, what in ((sums, 'bn_train_bwd'), (local, 'bn_backward reduce')):
                if live == 0:
                    assert not s.any(), what
                else:
                    R.check(s[:C], *ref['sum_g'], kk + 1, F32, what + ' sum g')
                    R.check(s[C:], *ref['sum_gx'], kk + R.K_SUM_GX, F32, what + ' sum g xhat')
            R.exact(sums_i[:C], dyi[:live].double().sum(0), 'bn_train_bwd sum g (integers)')
        count = 1.0 if v is not None else float(cap)                # with a row-count word the host value is a dummy, as in the head
        for n_glob in (None, float(2 * live + 3)):
            cnt = None if n_glob is None else torch.tensor([n_glob], device=dev)
            dx2, dres2, _ = K.bn_backward(dyd, yd, xd, pd[:C], pd[2 * C:3 * C], pd[3 * C:], count, act=act, slope=SLOPE, sums=glob.to(dev), apply_only=True,
                                          want_dres=True, count_ptr=cnt, rows=rw)
            R.check(dx2[:live], *ref2s[n_glob]['dx'], R.K_BN_DX, dtype, 'bn_backward apply dx')
            R.check(dres2[:live], *ref2s[n_glob]['dres'], 1, dtype, 'bn_backward apply dres')
        # the linked apply pass: two replicas of the sums (halves: their sum is exact), the divisor again the live count and not `count`
        rep = torch.stack([glob / 2, glob / 2]).to(dev)
        dx3, sums3 = K.bn_bwd_apply_linked(dyd, xd, pd, rep, float(cap), rows=rw)
        R.check(dx3[:live], *ref3['dx'], R.K_BN_DX + 1, dtype, 'bn_bwd_apply_linked dx')
        assert torch.equal(sums3.cpu(), glob)


@pytest.mark.parametrize('geom', COLUMNS, ids=_id)
def test_bias_act_bwd_rows(geom):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    dy0, y0, dyi0 = R.base_rows(cap, C, 27), R.base_rows(cap, C, 28), R.base_int_rows(cap, C, 29)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    for v, live in _words(cap):
        rw = _set(rows, v)
        dy, y = R.rows_input(dy0, live, dtype), R.rows_input(y0, live, dtype)
        dyi = R.rows_input(dyi0, live, dtype, outlier=8)
        R.assert_exact_conditions(dyi[:live], partial_bound=float(dyi[:live].double().abs().sum(0).max()) if live else 0.0)
        for det in (True, False):
            for use_y in (True, False):
                yy = y if use_y else None
                g_ref, (db_ref, s_db) = R.bias_act_bwd(dy[:live], None if yy is None else yy[:live])
                gi_ref, (dbi_ref, _) = R.bias_act_bwd(dyi[:live], None if yy is None else yy[:live])
                with _mode(det):
                    dyd = dy.to(dev)
                    g, db = K.bias_act_bwd(dyd, None if yy is None else yy.to(dev), True, rows=rw)
                    gi, dbi = K.bias_act_bwd(dyi.to(dev), None if yy is None else yy.to(dev), True, rows=rw)
                    g0, db0 = K.bias_act_bwd(dyd, None if yy is None else yy.to(dev), False, rows=rw)
                assert db0 is None
                if not use_y:
                    assert g.data_ptr() == dyd.data_ptr()             # in place: g IS dy
                for gg in (g, g0):
                    assert torch.equal(gg[:live].cpu().double(), g_ref), (v, det, use_y)
                if live == 0:
                    assert not db.any() and not dbi.any()
                else:
                    R.check(db, db_ref, s_db, R.sum_k(live), F32, 'bias_act_bwd db')
                R.exact(dbi, dbi_ref, 'bias_act_bwd db (integers)')
                assert torch.equal(gi[:live].cpu().double(), gi_ref)


# ------------------------------------------------------------------------------------------------------------------
# sparse.hip: dense <-> rows, alpha planes; region.hip: gather tables; rows.hip: the empty-region patch
# ------------------------------------------------------------------------------------------------------------------
N_F, N_I = 2, 3


def _dense(shape, seed, dtype, poison_pixel, integer=False):
    N, H, W, C = shape
    base = (R.base_int_rows(N * H * W, C, seed, lim=4) if integer else R.base_rows(N * H * W, C, seed)).reshape(shape).to(dtype)
    base[poison_pixel[0] // N_I, poison_pixel[1], poison_pixel[2]] = float('nan')
    return base


@pytest.mark.parametrize('geom', GATHER, ids=_id)
def test_gather_rows_rows(geom):
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    coords0, (P, H, W), poison = R.site_coords(cap, N_F, N_I, 30)
    dense = _dense((N_F, H, W, C), 31, dtype, poison)
    mul = R.base_rows(N_F * (N_I + 1), C, 32).float().reshape(N_F, N_I + 1, C)
    dd, md = dense.to(dev), mul.to(dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    store = {'cap': cap}
    for v, live in _words(cap):
        rw = _set(rows, v)
        coords = R.coords_input(coords0, live, poison)
        cd = coords.to(dev)
        before = R.guarded(cap, C, dtype)
        buf = before.to(dev)
        K.gather_rows(dd, cd, N_I, out=buf[:cap], rows=rw)
        ref, _ = R.gather_rows(dense, coords[:live], N_I)
        assert torch.equal(buf[:live].cpu().double(), ref), ('gather_rows is a copy', v)
        assert R.untouched(buf, before, live), ('gather_rows wrote outside the live rows', v)
        before2 = R.guarded(cap, 2 * C, dtype)
        buf2 = before2.to(dev)
        K.gather_rows(dd, cd, N_I, mul=md, out=buf2[:cap], yoff=C, rows=rw)
        R.check(buf2[:live, C:], *R.gather_rows(dense, coords[:live], N_I, mul), R.K_GATHER, dtype, 'gather_rows mul')
        assert R.untouched(buf2, before2, live, cols=(C, 2 * C)), ('gather_rows (yoff) wrote outside its slice', v)
        _same_as_cap(store, 'gather', v, buf, buf2)


@pytest.mark.parametrize('geom', ELEMENTWISE, ids=_id)
def test_gather_rows_bwd_rows_exact(geom):
    """Integer operands: ddense and dmul are exact whatever the order of the atomics (rows of several instance planes share a pixel), in both modes
    (deterministic: dmul through the ordered per-plane form)."""
    from maggie_amd import kernels as K
    dev = _dev()
    cap, C, dtype = geom
    coords0, (P, H, W), poison = R.site_coords(cap, N_F, N_I, 33)
    shape = (N_F, H, W, C)
    dense = _dense(shape, 34, dtype, poison, integer=True)
    mul = R.base_int_rows(N_F * (N_I + 1), C, 35, lim=4).float().reshape(N_F, N_I + 1, C)
    dout0 = R.base_int_rows(cap, 2 * C, 36)
    dd, md = dense.to(dev), mul.to(dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    for v, live in _words(cap):
        rw = _set(rows, v)
        coords = R.coords_input(coords0, live, poison)
        cd = coords.to(dev)
        dout_w = R.rows_input(dout0, live, dtype, outlier=8)
        dout = dout_w[:, C:]                                          # a channel slice read with yoff = C
        dod = dout_w.to(dev)
        (rdd, sdd), (rdm, sdm) = R.gather_rows_bwd(dout[:live], coords[:live], N_I, torch.nan_to_num(dense.double()), mul)
        (rdd0, sdd0), _ = R.gather_rows_bwd(dout[:live], coords[:live], N_I, torch.nan_to_num(dense.double()), None)
        R.assert_exact_conditions(dout[:live], mul, dense, partial_bound=max(float(sdd.max()), float(sdm.max()), float(sdd0.max())))
        for det in (True, False):
            with _mode(det):
                a, none = K.gather_rows_bwd(dod, cd, N_I, shape, yoff=C, rows=rw)
                b, bm = K.gather_rows_bwd(dod, cd, N_I, shape, mul=md, dense=dd, yoff=C, want_ddense=True, want_dmul=True, rows=rw)
                _, cm = K.gather_rows_bwd(dod, cd, N_I, shape, mul=md, dense=dd, yoff=C, want_ddense=False, want_dmul=True, rows=rw)
            assert none is None
            R.exact(a, rdd0, 'gather_rows_bwd ddense')
            R.exact(b, rdd, 'gather_rows_bwd ddense (mul)')
            R.exact(bm, rdm, 'gather_rows_bwd dmul (with ddense)')
            R.exact(cm, rdm, 'gather_rows_bwd dmul')


@pytest.mark.parametrize('dtype', [BF16, F16, F32])
@pytest.mark.parametrize('cap', [777, 20000])
def test_scatter_and_gather_plane_rows(cap, dtype):
    from maggie_amd import kernels as K
    dev = _dev()
    coords0, (P, H, W), poison = R.site_coords(cap, N_F, N_I, 37)
    vals0 = R.base_rows(cap, 8, 38)
    plane = R.base_rows(P * H, W, 39).float().reshape(P, H, W)
    plane[poison] = float('nan')
    pd = plane.to(dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    for v, live in _words(cap):
        rw = _set(rows, v)
        coords = R.coords_input(coords0, live, poison)
        cd = coords.to(dev)
        vals = R.rows_input(vals0, live, dtype)
        got = K.scatter_plane(vals.to(dev), 5, cd, P, H, W, fill=-99.0, rows=rw)
        ref = R.scatter_plane(vals[:live], 5, coords[:live], P, H, W, -99.0)
        assert torch.equal(got.cpu().double(), ref), ('scatter_plane', v)           # sites not hit keep the fill, the poison site included
        for width in (1, 8):
            out = K.gather_plane(pd, cd, dtype, width=width, rows=rw)
            assert torch.equal(out[:live].cpu().double(), R.gather_plane(plane, coords[:live], dtype, width)), ('gather_plane', v, width)
        back = K.gather_plane(got, cd, dtype, width=1, rows=rw)                       # round trip over the live rows
        assert torch.equal(R.bits_of(back[:live, 0]), R.bits_of(vals[:live, 5])), ('round trip', v)


def test_gather_table_rows():
    from maggie_amd import kernels as K
    from oracle import region
    dev = _dev()
    rs = np.random.RandomState(40)
    roi = (rs.uniform(size=(3, 40, 72)) > 0.6).astype(np.uint8)
    roi[1, :, :20] = 0
    pyr = region.active_pyramid(roi)
    levels = [(K.bits_pack(torch.from_numpy(roi).to(dev), mode=1), 40, 72)]
    levels.append(K.bits_downsample(levels[0][0], 72))
    ranks = [K.bits_rank(b, w)[1] for b, h, w in levels]
    co = [torch.from_numpy(region.coords_of(a)) for a in pyr[:2]]
    refs = {(0, 0): region.subm_neighbors(pyr[0]), (1, 0): region.inverse_neighbors(pyr[0], pyr[1]), (2, 1): R.strided_neighbors(pyr[1], pyr[0])}
    src = {0: 0, 1: 1, 2: 0}                                          # kind -> level of the source bit planes
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    for (kind, lv), ref in refs.items():
        cap = co[lv].shape[0]
        assert cap > 257 and ref.shape[0] == cap
        sb, hs, ws = levels[src[kind]]
        for v, live in _words(cap):
            rw = _set(rows, v)
            coords = co[lv].clone()
            coords[live:] = coords[0] if live else torch.zeros(3, dtype=torch.int32)     # dead rows: a valid site, never read
            nbr = K.gather_table(coords.to(dev), 3, kind, sb, ranks[src[kind]], hs, ws, rows=rw)
            assert np.array_equal(nbr[:live].cpu().numpy(), ref[:live]), (kind, v)


@pytest.mark.parametrize('W,box', [(100, (3, 9, 60, 70)), (128, (0, 12, 0, 128)), (200, (5, 6, 63, 65))], ids=['ragged', 'full', 'straddle'])
def test_bits_patch_if_empty(W, box):
    from maggie_amd import kernels as K
    dev = _dev()
    P, H = 3, 12
    y0, y1, x0, x1 = box
    g = torch.Generator().manual_seed(41)
    bits = torch.randint(-2 ** 62, 2 ** 62, (P, H, (W + 63) // 64), generator=g, dtype=torch.int64)
    bits &= torch.randint(-2 ** 62, 2 ** 62, bits.shape, generator=g, dtype=torch.int64)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    for c in (7, 1, 0):
        count.fill_(c)
        got = K.bits_patch_if_empty_(bits.to(dev), count, H, W, y0, y1, x0, x1)
        assert torch.equal(got.cpu(), R.patch_bits(bits, c, H, W, y0, y1, x0, x1)), c
    assert not torch.equal(R.patch_bits(bits, 0, H, W, y0, y1, x0, x1), bits)
