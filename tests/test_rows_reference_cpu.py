"""Host-side proof for tests/test_gpu_rows.py: the float64 references of tests/rows_reference.py equal torch.autograd in float64, and the
element-wise comparison rejects every way a device-row-count kernel can be subtly wrong (a dropped last row, an added dead row, a divisor taken
from the capacity, a shifted row, a two-unit error, a write past the capacity) while it accepts the correctly rounded result. No GPU needed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rows_reference as R

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
CAPS = [777, 140000]                      # both ends of the capacity range of test_gpu_rows.py
TIGHT = 1e-12


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------
# the references are right
# ------------------------------------------------------------------------------------------------------------------
def test_layernorm_reference_equals_autograd():
    g = torch.Generator().manual_seed(0)
    M, C = 37, 32
    x = torch.randn((M, C), generator=g, dtype=torch.float64, requires_grad=True)
    r = (torch.randn((M, C), generator=g, dtype=torch.float64) + 5).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((M, C), generator=g, dtype=torch.float64)
    y = F.layer_norm(x + r, (C,), gamma, beta, 1e-5)
    y.backward(dy)
    (yr, _), (mean, _), (rstd, _) = R.layernorm(x.detach(), r.detach(), gamma.detach(), beta.detach(), 1e-5)
    assert _rel(yr, y.detach()) < TIGHT
    (dz, _), (dgm, _), (dbt, _) = R.layernorm_bwd(dy, x.detach(), r.detach(), gamma.detach(), mean, rstd)
    assert _rel(dz, x.grad) < TIGHT and _rel(dz, r.grad) < TIGHT
    assert _rel(dgm, gamma.grad) < TIGHT and _rel(dbt, beta.grad) < TIGHT


def test_sigmoid_mul_reference_equals_autograd():
    g = torch.Generator().manual_seed(1)
    a = torch.randn((29, 16), generator=g, dtype=torch.float64, requires_grad=True)
    gt = (torch.randn((29, 16), generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    d = torch.randn((29, 16), generator=g, dtype=torch.float64)
    out = a * torch.sigmoid(gt)
    out.backward(d)
    assert _rel(R.sigmoid_mul(a.detach(), gt.detach())[0], out.detach()) < TIGHT
    (da, _), (dg, _) = R.sigmoid_mul_bwd(d, a.detach(), gt.detach())
    assert _rel(da, a.grad) < TIGHT and _rel(dg, gt.grad) < TIGHT


@pytest.mark.parametrize('act', [R.ACT_NONE, R.ACT_RELU, R.ACT_LEAKY])
@pytest.mark.parametrize('count_mult', [1, 3])
def test_batchnorm_reference_equals_autograd(act, count_mult):
    g = torch.Generator().manual_seed(2)
    M, C, eps, mom = 53, 16, 1e-5, 0.1
    x = (torch.randn((M, C), generator=g, dtype=torch.float64) * 2 + 1).requires_grad_(True)
    res = torch.randn((M, C), generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    rm0, rv0 = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dy = torch.randn((M, C), generator=g, dtype=torch.float64)
    rm, rv = rm0.clone(), rv0.clone()
    # every row stands for count_mult samples: the same batch statistics, the unbiased factor of M * count_mult samples
    pre = F.batch_norm(x.repeat(count_mult, 1), rm, rv, gamma, beta, True, mom, eps)[:M] + res
    y = [lambda t: t, F.relu, lambda t: F.leaky_relu(t, 0.2)][act](pre)
    y.backward(dy)
    ref = R.batchnorm(x.detach(), gamma.detach(), beta.detach(), rm0, rv0, mom, eps, count_mult, res.detach(), act, 0.2)
    assert _rel(ref['y'][0], y.detach()) < TIGHT
    assert _rel(ref['running_mean'][0], rm) < TIGHT and _rel(ref['running_var'][0], rv) < TIGHT
    assert _rel(ref['sum'][0], x.detach().sum(0)) < TIGHT and _rel(ref['censq'][0], ((x - x.mean(0)) ** 2).detach().sum(0)) < TIGHT
    b = R.batchnorm_bwd(dy, y.detach(), x.detach(), ref['scale'][0], ref['mean'][0], ref['invstd'][0], act, 0.2)
    assert _rel(b['dx'][0], x.grad) < TIGHT
    assert _rel(b['dres'][0], res.grad) < TIGHT
    assert _rel(b['sum_g'][0], beta.grad) < TIGHT and _rel(b['sum_gx'][0], gamma.grad) < TIGHT


def test_batchnorm_backward_reference_equals_autograd_plain():
    """count_mult = 1, no repetition: dx itself."""
    g = torch.Generator().manual_seed(3)
    M, C, eps = 41, 8, 1e-5
    x = (torch.randn((M, C), generator=g, dtype=torch.float64) * 2 + 1).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn((M, C), generator=g, dtype=torch.float64)
    y = F.leaky_relu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps), 0.2)
    y.backward(dy)
    ref = R.batchnorm(x.detach(), gamma.detach(), beta.detach(), torch.zeros(C), torch.ones(C), 0.1, eps, act=R.ACT_LEAKY)
    b = R.batchnorm_bwd(dy, y.detach(), x.detach(), ref['scale'][0], ref['mean'][0], ref['invstd'][0], R.ACT_LEAKY, 0.2)
    assert _rel(b['dx'][0], x.grad) < TIGHT
    assert _rel(b['sum_g'][0], beta.grad) < TIGHT and _rel(b['sum_gx'][0], gamma.grad) < TIGHT


def test_gather_reference_equals_autograd():
    n_f, n_i, C, cap = 2, 3, 8, 300
    coords, (P, H, W), _ = R.site_coords(cap, n_f, n_i, 5)
    g = torch.Generator().manual_seed(4)
    dense = torch.randn((n_f, H, W, C), generator=g, dtype=torch.float64, requires_grad=True)
    mul = torch.randn((n_f, n_i + 1, C), generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn((cap, C), generator=g, dtype=torch.float64)
    c = coords.long()
    frame, inst = c[:, 0] // n_i, c[:, 0] % n_i
    out = dense[frame, c[:, 1], c[:, 2]] * mul[frame, inst]
    out.backward(dout)
    assert _rel(R.gather_rows(dense.detach(), coords, n_i, mul.detach())[0], out.detach()) < TIGHT
    (dd, _), (dm, _) = R.gather_rows_bwd(dout, coords, n_i, dense.detach(), mul.detach())
    assert _rel(dd, dense.grad) < TIGHT and _rel(dm, mul.grad) < TIGHT
    # rows of several instance planes share pixels (the atomics of the device kernel collide there)
    pix = (frame * H + c[:, 1]) * W + c[:, 2]
    assert pix.unique().numel() < cap


def test_strided_table_is_the_transpose_of_the_inverse_table():
    from oracle import region
    rs = np.random.RandomState(7)
    roi = rs.uniform(size=(3, 20, 36)) > 0.7
    pyr = region.active_pyramid(roi.astype(np.uint8))
    inv = region.inverse_neighbors(pyr[0], pyr[1])
    down = R.strided_neighbors(pyr[1], pyr[0])
    chk = np.full_like(down, -1)
    rr, kk = np.nonzero(inv >= 0)
    chk[inv[rr, kk], kk] = rr
    assert np.array_equal(down, chk)


def test_patch_bits_reference():
    bits = torch.zeros((2, 5, 2), dtype=torch.int64)
    assert torch.equal(R.patch_bits(bits, 3, 5, 100, 1, 4, 60, 70), bits)
    out = R.patch_bits(bits, 0, 5, 100, 1, 4, 60, 70).numpy().view(np.uint64)
    dense = ((out[:, :, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(2, 5, 128)[:, :, :100]
    want = np.zeros((2, 5, 100), np.uint64)
    want[:, 1:4, 60:70] = 1
    assert np.array_equal(dense, want)


# ------------------------------------------------------------------------------------------------------------------
# the comparison has teeth
# ------------------------------------------------------------------------------------------------------------------
C = 64
_CASES = {}


def _case(cap, dtype):
    """One case per (capacity, dtype) with live = cap - 1 (one dead row exists, the divisors cap / live / live - 1 are as close as they get):
    the operands of an element-wise kernel, of column sums of values and of rounded products, and of the BatchNorm statistics, with their
    float64 references. `shadow` holds what the dead rows held before they were poisoned (a kernel that reads one row too many in a
    buffer that was not poisoned adds a FINITE row)."""
    key = (cap, dtype)
    if key in _CASES:
        return _CASES[key]
    live = cap - 1
    a0, b0 = R.base_rows(cap, C, 11), R.base_rows(cap, C, 12)
    x0 = R.base_rows(cap, C, 13, std=1.0, offset=3.0)             # BatchNorm input: the mean carries weight
    xi0 = R.base_int_rows(cap, C, 14)
    a, b, x, xi = (R.rows_input(t, live, dtype) for t in (a0, b0, x0, xi0))
    k = type('Case', (), {})()
    k.cap, k.live, k.dtype = cap, live, dtype
    k.a, k.b, k.x, k.xi = a, b, x, xi
    k.shadow = {'a': a0.to(dtype), 'b': b0.to(dtype), 'x': x0.to(dtype), 'xi': xi0.to(dtype)}
    k.add = R.add(a[:live], b[:live])
    k.colsum = (a[:live].double().sum(0), a[:live].double().abs().sum(0))
    k.prod = ((a[:live].double() * b[:live].double()).sum(0), (a[:live].double() * b[:live].double()).abs().sum(0))
    k.isum = xi[:live].double().sum(0)
    gamma, beta = torch.ones(C), torch.zeros(C)
    k.bn = R.batchnorm(x[:live], gamma, beta, torch.zeros(C), torch.ones(C), 0.1, 1e-5)
    _CASES[key] = k
    return k


def _kmax(live):
    """The largest k a column sum is compared under in test_gpu_rows.py."""
    return R.sum_k(live) + max(R.K_XHAT, R.K_SUM_GX, R.K_CENSQ, R.K_BN_VAR, R.K_BN_SHIFT, R.K_BN_MEAN)


def _round(ref, dtype):
    return ref.to(dtype)


@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_correctly_rounded_results_pass(cap, dtype):
    k = _case(cap, dtype)
    assert R.close(_round(k.add[0], dtype), *k.add, R.K_ADD, dtype)
    assert R.close(k.colsum[0].float(), *k.colsum, R.sum_k(k.live), torch.float32)
    assert R.close(k.prod[0].float(), *k.prod, R.sum_k(k.live), torch.float32)
    for name, kk in (('mean', R.K_BN_MEAN), ('running_mean', R.K_BN_MEAN), ('shift', R.K_BN_SHIFT), ('invstd', R.K_BN_VAR), ('scale', R.K_BN_VAR),
                     ('running_var', R.K_BN_VAR)):
        assert R.close(k.bn[name][0].float(), *k.bn[name], R.sum_k(k.live) + kk, torch.float32), name
    R.exact(k.isum.float(), k.isum, 'integer column sum')


@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_last_live_row_missing_is_rejected(cap, dtype):
    k = _case(cap, dtype)
    last = k.live - 1
    assert not R.close((k.colsum[0] - k.a[last].double()).float(), *k.colsum, R.sum_k(k.live), torch.float32)
    assert not R.close((k.prod[0] - k.a[last].double() * k.b[last].double()).float(), *k.prod, R.sum_k(k.live), torch.float32)
    mean = (k.x[:k.live].double().sum(0) - k.x[last].double()) / k.live
    assert not R.close(mean.float(), *k.bn['mean'], R.sum_k(k.live) + R.K_BN_MEAN, torch.float32)
    with pytest.raises(AssertionError):
        R.exact((k.isum - k.xi[last].double()).float(), k.isum, 'integer column sum')
    # ... and the first live row
    assert not R.close((k.colsum[0] - k.a[0].double()).float(), *k.colsum, R.sum_k(k.live), torch.float32)
    # the same under the LARGEST k any column sum of the device tests runs with (dgamma: + K_XHAT, sum g * xhat: + K_SUM_GX, the centred
    # squares: + K_CENSQ, the variance family: + K_BN_VAR)
    assert not R.close((k.colsum[0] - k.a[last].double()).float(), *k.colsum, _kmax(k.live), torch.float32)
    assert not R.close((k.prod[0] - k.a[last].double() * k.b[last].double()).float(), *k.prod, _kmax(k.live), torch.float32)
    d = k.x[:k.live].double() - k.bn['mean'][0]
    assert R.close(k.bn['censq'][0].float(), *k.bn['censq'], R.sum_k(k.live) + R.K_CENSQ, torch.float32)
    assert not R.close((k.bn['censq'][0] - d[last] ** 2).float(), *k.bn['censq'], _kmax(k.live), torch.float32)
    # ... and the variance a kernel forms from the short sum, against invstd and running_var under their own k
    var = (k.bn['censq'][0] - d[last] ** 2) / k.live
    assert not R.close(torch.rsqrt(var + 1e-5).float(), *k.bn['invstd'], R.sum_k(k.live) + R.K_BN_VAR, torch.float32)
    assert not R.close((0.9 + 0.1 * var * k.live / (k.live - 1)).float(), *k.bn['running_var'], R.sum_k(k.live) + R.K_BN_VAR, torch.float32)


@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_first_dead_row_included_is_rejected(cap, dtype):
    k = _case(cap, dtype)
    dead = k.live
    assert torch.isnan(k.a[dead]).all() and torch.isnan(k.x[dead]).all()
    for extra_a, extra_x, extra_i in ((k.shadow['a'][dead], k.shadow['x'][dead], k.shadow['xi'][dead]), (k.a[dead], k.x[dead], k.xi[dead])):
        assert not R.close((k.colsum[0] + extra_a.double()).float(), *k.colsum, R.sum_k(k.live), torch.float32)
        mean = (k.x[:k.live].double().sum(0) + extra_x.double()) / k.live
        assert not R.close(mean.float(), *k.bn['mean'], R.sum_k(k.live) + R.K_BN_MEAN, torch.float32)
        with pytest.raises(AssertionError):
            R.exact((k.isum + extra_i.double()).float(), k.isum, 'integer column sum')
        # under the largest k in use: the sum of values and of rounded products. The centred squares under their own k; under the largest one
        # (that of invstd / running_var) a FINITE row of typical size among 140 000 stays inside the tolerance (ratio 54 against k = 74: S of a
        # variance counts 2 |d| (|x| + |mean|) per term) -- at that size the variance family sees an added dead row because it is NaN
        assert not R.close((k.colsum[0] + extra_a.double()).float(), *k.colsum, _kmax(k.live), torch.float32)
        extra_p = extra_a.double() * k.shadow['b'][dead].double() if torch.isfinite(extra_a).all() else extra_a.double()
        assert not R.close((k.prod[0] + extra_p).float(), *k.prod, _kmax(k.live), torch.float32)
        extra_d = (extra_x.double() - k.bn['mean'][0]) ** 2
        assert not R.close((k.bn['censq'][0] + extra_d).float(), *k.bn['censq'], R.sum_k(k.live) + R.K_CENSQ, torch.float32)
        if cap < 1000 or not torch.isfinite(extra_x).all():
            assert not R.close((k.bn['censq'][0] + extra_d).float(), *k.bn['censq'], _kmax(k.live), torch.float32)
            var = (k.bn['censq'][0] + extra_d) / k.live
            assert not R.close(torch.rsqrt(var + 1e-5).float(), *k.bn['invstd'], R.sum_k(k.live) + R.K_BN_VAR, torch.float32)


@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('divisor', ['cap', 'live-1'])
def test_wrong_divisor_is_rejected(cap, dtype, divisor):
    k = _case(cap, dtype)
    n = k.cap if divisor == 'cap' else k.live - 1
    x = k.x[:k.live].double()
    mean = x.sum(0) / n
    kk = R.sum_k(k.live) + R.K_BN_MEAN
    assert not R.close(mean.float(), *k.bn['mean'], kk, torch.float32)
    small = 5                                                       # the same buffers with five live rows: any divisor but 5 is far off
    xs = k.x[:small].double()
    ref = R.batchnorm(xs, torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C), 0.1, 1e-5)
    g = k.a[:small].double()
    b = R.batchnorm_bwd(g, None, xs, ref['scale'][0], ref['mean'][0], ref['invstd'][0])
    xh = (xs - ref['mean'][0]) * ref['invstd'][0]
    for wrong in (k.cap, small - 1):
        assert not R.close((xs.sum(0) / wrong).float(), *ref['mean'], R.sum_k(small) + R.K_BN_MEAN, torch.float32)
        # a BatchNorm backward that divides its two sums by the wrong count (the capacity M is what the host passes)
        dx = ref['scale'][0] * (g - b['sum_g'][0] / wrong - xh * b['sum_gx'][0] / wrong)
        assert not R.close(dx.to(dtype), *b['dx'], R.sum_k(small) + R.K_BN_DX, dtype)
    dx = ref['scale'][0] * (g - b['sum_g'][0] / small - xh * b['sum_gx'][0] / small)
    assert R.close(dx.to(dtype), *b['dx'], R.sum_k(small) + R.K_BN_DX, dtype)


@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_shifted_row_and_two_unit_error_are_rejected(cap, dtype):
    k = _case(cap, dtype)
    ref, S = k.add
    good = _round(ref, dtype)
    for m in (0, k.live // 2, k.live - 2):
        bad = good.clone()
        bad[m] = good[m + 1]
        assert not R.close(bad, ref, S, R.K_ADD, dtype)
    # two units of the output dtype on the best-conditioned element (for an fp32 output a unit is u32 and k units are allowed by construction:
    # the addition has k = 1)
    unit = R.U_OUT[dtype] if dtype != torch.float32 else R.U32
    flat = int((ref.abs() / S.clamp_min(1e-300)).reshape(-1).argmax())
    bad = good.double().reshape(-1).clone()
    bad[flat] = ref.reshape(-1)[flat] * (1 + 2 * unit)
    assert not R.close(bad.reshape(ref.shape), ref, S, R.K_ADD, dtype)
    ok = good.double().reshape(-1).clone()
    ok[flat] = ref.reshape(-1)[flat] * (1 + 0.5 * unit)
    assert R.close(ok.reshape(ref.shape), ref, S, R.K_ADD, dtype)
    if dtype != torch.float32:                                      # 16-bit outputs: two units miss under every k in use (k u32 S << u_out |ref|)
        kmax = R.sum_k(140000) + R.K_BN_VAR + R.K_LN_Y
        assert not R.close(bad.reshape(ref.shape), ref, S, kmax, dtype)


@pytest.mark.parametrize('cap', CAPS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_overwritten_guard_or_dead_row_is_rejected(cap, dtype):
    live = cap - 1
    before = R.guarded(cap, C, dtype)
    buf = before.clone()
    buf[:live] = 1.0
    assert R.untouched(buf, before, live)
    for row in (live, cap, cap + R.GUARD - 1):                      # the dead row, the first and the last guard row
        bad = buf.clone()
        bad[row, 3] = 1.0
        assert not R.untouched(bad, before, live)
    wide = R.guarded(cap, 2 * C, dtype)                             # a channel slice: the columns next to it count too
    w = wide.clone()
    w[:live, C:] = 2.0
    assert R.untouched(w, wide, live, cols=(C, 2 * C))
    w[1, C - 1] = 2.0
    assert not R.untouched(w, wide, live, cols=(C, 2 * C))
    # the sentinel survives a copy through the dtype bit for bit and is not a value a kernel would produce by accident
    assert torch.isfinite(before.float()).all() and torch.equal(R.bits_of(before.clone()), R.bits_of(before))


# ------------------------------------------------------------------------------------------------------------------
# the exact-integer cases
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', [777, 20000, 70001, 140000])
def test_exact_integer_conditions(cap):
    xi = R.rows_input(R.base_int_rows(cap, C, 14), cap, torch.float32, outlier=8)
    yi = R.rows_input(R.base_int_rows(cap, C, 15), cap, torch.float32, outlier=8)
    assert float(xi.abs().max()) <= 64 and float(xi[1:cap - 1].abs().max()) <= 8
    # column sums, sums of squares and sums of products of two such operands: the sum of absolute values bounds every partial sum
    bound = max(float(xi.abs().sum(0).max()), float((xi * xi).sum(0).max()), float((xi * yi).abs().sum(0).max()))
    R.assert_exact_conditions(xi, yi, partial_bound=bound)
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(xi.to(dt).float(), xi)
    with pytest.raises(AssertionError):
        R.assert_exact_conditions(xi * 0.5 + 0.25, partial_bound=1.0)
    with pytest.raises(AssertionError):
        R.assert_exact_conditions(xi * 1024 + 1, partial_bound=1.0)              # 8193: not a bf16 / f16 integer
    with pytest.raises(AssertionError):
        R.assert_exact_conditions(xi, partial_bound=2.0 ** 24)


def test_live_counts_and_clamp():
    assert R.live_counts(777) == [-3, 0, 1, 5, 257, 776, 777, 1777]
    assert [R.clamp_live(v, 777) for v in R.live_counts(777) + [None]] == [0, 0, 1, 5, 257, 776, 777, 777, 777]
