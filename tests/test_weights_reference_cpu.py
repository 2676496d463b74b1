"""Host-side proof for tests/test_gpu_weights.py: the float64 references of tests/weights_reference.py equal torch in float64 (the statements of
SpectralNorm.normalized_weight and autograd through W / sigma), the element-wise comparison accepts a plain fp32 numpy evaluation of the same
formulas for every case of the device file, and it rejects every seeded way the spectral-norm kernels can be subtly wrong: a dropped last row
or last 32-column block of W^T u, a dropped row of W t, swapped kh / kw, swapped A / B in the transposed layout, a non-zero padding element, a
tile's partial missing from <G, W>, the vectors from before the power iteration, a flipped rank-one term, a twin-layout gradient read in the
ordinary order. No GPU needed."""
import numpy as np
import pytest
import torch

import weights_reference as R

F = np.float32
DTYPES = [R.BF16, R.F16, R.F32]
GEOMS = R.all_geoms()
_id = str


# ------------------------------------------------------------------------------------------------------------------
# the references are right
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', [R.G_(7, 3, 3), R.G_(20, 32, 4, transposed=1), R.G_(30, 7, 1, 3)], ids=_id)
def test_reference_equals_torch_float64(g):
    """power_iteration / krsc / twin / dW against the module's own statements and autograd, both in float64."""
    from maggie_amd.network.module.spectral_norm import l2normalize
    W, u, v0 = R.make_w(g).double(), R.make_u(g).double(), R.make_v(g).double()
    wm = W.reshape(g.A, -1)
    nv = l2normalize(torch.mv(wm.t(), u))
    nu = l2normalize(torch.mv(wm, nv))
    sigma = nu.dot(wm.mv(nv))
    ref = R.forward_reference(W, u, g.transposed, g.pad_in)
    tight = lambda a, b: float(np.abs(a - b.numpy()).max()) <= 1e-13 * max(float(b.abs().max()), 1.0)    # noqa: E731
    assert tight(ref['v'].value, nv) and tight(ref['u'].value, nu) and tight(ref['sigma'].value, sigma.reshape(1))
    wb = W.clone().requires_grad_(True)
    wn = wb / nu.dot(wb.reshape(g.A, -1).mv(nv))                              # u', v' held fixed, as the kernels do
    k = wn.permute(1, 2, 3, 0) if g.transposed else wn.permute(0, 2, 3, 1)     # (Cout, kh, kw, Cin)
    k = torch.nn.functional.pad(k.reshape(g.cout, g.taps, g.cin), (0, g.pad_in - g.cin))
    assert tight(ref['out'].value, k.detach()) and tight(ref['twin'].value, k.detach().permute(2, 1, 0))
    G = R.make_g(g, torch.float64, pad=0.0)
    (want,) = torch.autograd.grad(k, wb, G)
    got = R.dW(G, W, nu, nv, float(sigma), g.transposed)
    assert tight(got.value, want.reshape(g.A, g.B, g.taps))
    Gt = R.make_g(g, torch.float64).permute(2, 1, 0).contiguous()              # the twin's order, NaN in the padded rows: never read
    assert np.array_equal(R.dW(Gt, W, nu, nv, float(sigma), g.transposed, twin_layout=True).value, got.value)


def test_inputs_carry_their_outliers_and_poison():
    g = R.G_(20, 32, 4, transposed=1)
    W, G = R.make_w(g).reshape(g.A, g.B, g.taps), R.make_g(g, R.BF16)
    assert float(W[-1].abs().mean()) > 8 * float(W[:-1, :-1, :-1].abs().mean())
    assert float(W[:, -1].abs().mean()) > 8 * float(W[:-1, :-1, :-1].abs().mean())
    assert float(W[:, :, -1].abs().mean()) > 8 * float(W[:-1, :-1, :-1].abs().mean())
    assert G.shape == (32, 16, 24) and torch.isnan(G[:, :, 20:]).all() and torch.isfinite(G[:, :, :20]).all()
    assert abs(float(R.make_u(g).double().norm()) - 1) < 1e-6
    assert torch.equal(R.rounded(G, R.BF16)[:, :, :20], G.float()[:, :, :20])


# ------------------------------------------------------------------------------------------------------------------
# a plain fp32 numpy evaluation of the same formulas, with seeded mutations
# ------------------------------------------------------------------------------------------------------------------
def _krsc32(g, Wn, mut):
    """(A, B, kh, kw) fp32 -> (Cout, taps, pad_in)."""
    A, B, kh, kw = g.A, g.B, g.kh, g.kw
    if mut == 'swap_khkw':
        Wn = Wn.transpose(0, 1, 3, 2)                                         # tap = kx * kh + ky
    if mut == 'swap_ab' and g.transposed:
        Wn = Wn.reshape(-1).reshape(B, A, kh, kw).transpose(1, 0, 2, 3)        # the parameter read as [Cout][Cin]
    Wn = np.ascontiguousarray(Wn).reshape(A, B, g.taps)
    o = Wn.transpose(1, 2, 0) if g.transposed else Wn.transpose(0, 2, 1)
    out = np.zeros((g.cout, g.taps, g.pad_in), F)
    out[:, :, :g.cin] = o
    if mut == 'pad_nonzero' and g.pad_in > g.cin:
        out[g.cout - 1, g.taps - 1, g.pad_in - 1] = F(2.0 ** -20)
    return out


def forward32(g, W, u, mut=None):
    """The kernels' statements in fp32 numpy: t = W^T u, s' = W t, the two norms, sv / su / sigma as sn_finish_kernel forms them."""
    Wm = W.numpy().reshape(g.A, -1)
    u = u.numpy()
    eps = F(1e-12)
    if mut == 'drop_last_row':
        t = Wm[:-1].T @ u[:-1]
    else:
        t = Wm.T @ u
    if mut == 'drop_last_colblock':
        t = t.copy()
        t[(g.Wd - 1) // 32 * 32:] = 0
    s = Wm @ t
    if mut == 'drop_row_of_four':
        s = s.copy()
        s[3::4] = 0
    nt = np.sqrt(np.sum(t * t, dtype=F))
    sv = F(1) / (nt + eps)
    ns = np.sqrt(np.sum(s * s, dtype=F)) * sv
    su = sv / (ns + eps)
    sigma = ns * ns / (ns + eps)
    out = _krsc32(g, W.numpy() * (F(1) / sigma), mut)
    assert t.dtype == F and out.dtype == F and np.asarray(sigma).dtype == F
    return {'v': t * sv, 'u': s * su, 'sigma': np.array([sigma], F), 'out': out, 'twin': np.ascontiguousarray(out.transpose(2, 1, 0))}


def backward32(g, G, W, u, v, sigma, mut=None, twin_layout=False):
    """dW in fp32 numpy from a gradient in the (Cout, taps, pad_in) order (or the twin's)."""
    G = G.float().numpy()
    if mut == 'twin_as_krsc':
        G = G.reshape(-1).reshape(g.cout, g.taps, g.pad_in)                    # the twin's memory read in the ordinary order
        twin_layout = False
    if twin_layout:
        G = G.transpose(2, 1, 0)
    G = G[:, :, :g.cin]
    Gp = np.ascontiguousarray(G.transpose(2, 0, 1) if g.transposed else G.transpose(0, 2, 1))
    Wp = W.numpy().reshape(g.A, g.B, g.taps)
    prod = Gp * Wp
    dot = np.sum(prod, dtype=F)
    if mut == 'drop_tile':                                                     # the last (16 x 32) tile's partial
        a0, b0 = (g.A - 1) // 16 * 16, (g.B - 1) // 32 * 32
        dot = dot - np.sum(prod[a0:, b0:], dtype=F)
    inv = F(1) / F(sigma)
    coef = dot * inv * inv
    if mut == 'flip_sign':
        coef = -coef
    out = Gp * inv - coef * u.reshape(g.A, 1, 1) * v.reshape(1, g.B, g.taps)
    assert out.dtype == F
    return out


_memo = {}


def _case(g):
    if g not in _memo:
        W, u = R.make_w(g), R.make_u(g)
        _memo[g] = (W, u, R.forward_reference(W, u, g.transposed, g.pad_in))
    return _memo[g]


def _store(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _forward_ok(g, dtype, mut=None):
    """(vectors ok, weight ok, twin ok, padding ok) of the fp32 evaluation under `mut`."""
    W, u, ref = _case(g)
    got = forward32(g, W, u, mut)
    vec = (R.close(got['v'], ref['v'], R.k_v(g.Wd), R.F32) and R.close(got['u'], ref['u'], R.k_u(g.A), R.F32)
           and R.close(got['sigma'], ref['sigma'], R.k_sigma(g.A), R.F32))
    out, tw = _store(got['out'], dtype), _store(got['twin'], dtype)
    return (vec, R.close(out, ref['out'], R.K_OUT, dtype), R.close(tw, ref['twin'], R.K_OUT, dtype),
            R.padding_is_zero(out, g.cin) and R.twin_padding_is_zero(tw, g.cin))


def _backward_ok(g, dtype, mut=None, twin_layout=False, stale=False):
    W, u, ref = _case(g)
    G = R.make_g(g, dtype)
    want = R.backward_reference(G, W, ref, g.transposed)
    fed = G.permute(2, 1, 0).contiguous() if twin_layout else G
    f = forward32(g, W, u)
    uu, vv = (u.numpy(), R.make_v(g).numpy()) if stale else (f['u'], f['v'])
    got = backward32(g, fed, W, uu, vv, f['sigma'][0], mut, twin_layout)
    return R.close(got, want, R.K_DW, R.F32)


@pytest.mark.parametrize('dtype', DTYPES, ids=lambda d: str(d).replace('torch.', ''))
@pytest.mark.parametrize('g', GEOMS, ids=_id)
def test_comparator_accepts_fp32_evaluation(g, dtype):
    """Every case of the device file, evaluated in fp32 numpy and stored in `dtype`, stays within the bounds."""
    assert _forward_ok(g, dtype) == (True, True, True, True)
    assert _backward_ok(g, dtype)
    if g.transposed:
        assert _backward_ok(g, dtype, twin_layout=True)


def test_comparator_accepts_second_iteration_from_rounded_vectors():
    """The second call starts from the fp32 u the first one wrote: a fresh reference from that vector has no inherited budget to lean on."""
    g = R.G_(57, 34, 3)
    W, u, _ = _case(g)
    first = forward32(g, W, u)
    u1 = torch.from_numpy(first['u'])
    ref = R.forward_reference(W, u1, 0, g.pad_in)
    got = forward32(g, W, u1)
    assert R.close(got['v'], ref['v'], R.k_v(g.Wd), R.F32) and R.close(got['u'], ref['u'], R.k_u(g.A), R.F32)
    assert R.close(got['sigma'], ref['sigma'], R.k_sigma(g.A), R.F32) and R.close(got['out'], ref['out'], R.K_OUT, R.F32)


FORWARD_MUTATIONS = {
    # name: (applies to g, index of the verdict in _forward_ok that must turn False)
    'drop_last_row': (lambda g: g.A > 1, 0),
    'drop_last_colblock': (lambda g: g.Wd > 32, 0),
    'drop_row_of_four': (lambda g: g.A >= 4, 0),
    'swap_khkw': (lambda g: g.kh > 1 and g.kw > 1, 1),
    'swap_ab': (lambda g: g.transposed and g.A != g.B, 1),
    'pad_nonzero': (lambda g: g.pad_in > g.cin, 3),
}


@pytest.mark.parametrize('mut', sorted(FORWARD_MUTATIONS))
def test_comparator_rejects_forward_mutation(mut):
    applies, idx = FORWARD_MUTATIONS[mut]
    hit = [g for g in GEOMS if applies(g) and g.numel <= 600000]
    assert len(hit) >= 2
    for g in hit:
        for dtype in DTYPES:
            ok = _forward_ok(g, dtype, mut)
            assert not ok[idx], (mut, str(g), dtype)
            if mut in ('swap_khkw', 'swap_ab'):
                assert not ok[2], (mut, str(g), dtype)                        # the twin is wrong with it


BACKWARD_MUTATIONS = {
    'drop_tile': lambda g: g.numel > 1,
    'flip_sign': lambda g: g.numel > 1,
    'twin_as_krsc': lambda g: g.transposed,
}


@pytest.mark.parametrize('mut', sorted(BACKWARD_MUTATIONS))
def test_comparator_rejects_backward_mutation(mut):
    hit = [g for g in GEOMS if BACKWARD_MUTATIONS[mut](g) and g.numel <= 600000]
    assert len(hit) >= 2
    for g in hit:
        for dtype in DTYPES:
            assert not _backward_ok(g, dtype, mut, twin_layout=(mut == 'twin_as_krsc')), (mut, str(g), dtype)


def test_comparator_rejects_vectors_from_before_the_power_iteration():
    for g in GEOMS:
        if g.numel > 1 and g.numel <= 600000:
            for dtype in DTYPES:
                assert not _backward_ok(g, dtype, stale=True), (str(g), dtype)


def test_comparator_rejects_a_negative_zero_in_the_padding():
    out = torch.zeros((4, 9, 8), dtype=R.BF16)
    assert R.padding_is_zero(out, 3) and R.twin_padding_is_zero(out.permute(2, 1, 0).contiguous(), 3)
    out[3, 8, 7] = -0.0
    assert not R.padding_is_zero(out, 3) and not R.twin_padding_is_zero(out.permute(2, 1, 0).contiguous(), 3)
    out[3, 8, 7] = float('nan')
    assert not R.padding_is_zero(out, 3)


def test_comparator_rejects_nan_and_shape_mismatch():
    g = R.G_(7, 3, 3)
    W, u, ref = _case(g)
    got = forward32(g, W, u)
    bad = got['out'].copy()
    bad[0, 0, 0] = np.nan
    assert not R.close(bad, ref['out'], R.K_OUT, R.F32)
    assert not R.close(got['out'][:, :, :3], ref['out'], R.K_OUT, R.F32)


def test_plan_refuses_more_than_sixteen_taps():
    """A 5x5 kernel (25 taps) does not fit the (16 x 32 x 16 taps) LDS tile of the batched kernels: the plan must say so, not build."""
    from maggie_amd import functional as MF, hip
    from maggie_amd.network.module import ConvWeight, SpectralNorm
    with pytest.raises(hip.MaggieHipError, match='16 taps'):
        MF.SpectralNormPlan([SpectralNorm(ConvWeight(4, 4, 5, 1, 2, 1))], torch.bfloat16)
    with pytest.raises(hip.MaggieHipError, match='16 taps'):
        MF.SpectralNormPlan([ConvWeight(4, 4, 5, 1, 2, 1)], torch.float32)
