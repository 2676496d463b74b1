"""The spectral-norm weight kernels (csrc/spectral_norm.hip) against float64 at their tile edges: the per-conv mg_spectral_norm /
mg_spectral_norm_bwd and the batched pipeline behind functional.spectral_norm_prepare (SpectralNormPlan, SpectralNormBatch).

The references (one power iteration, W / sigma in the (Cout, taps, pad_in) layout and its twin, dW = G / sigma - <G, W> / sigma^2 u' v'^T), the
case construction (normal W and G from a fixed seed per geometry, last row / last column / last tap scaled by 16, values rounded through the
storage type on the host) and the element-wise comparison |got - ref| <= u_out |ref| + u32 k S live in tests/weights_reference.py;
tests/test_weights_reference_cpu.py proves on the host that this comparison accepts an fp32 numpy evaluation of every case below and rejects a
dropped last row, a dropped last 32-column block, a dropped row of four, swapped kh / kw, swapped A / B, a non-zero padding element, a missing
tile partial, stale vectors, a flipped rank-one term and a twin-layout gradient read in the ordinary order.

A. per-conv, fp32 / bf16 / f16 outputs, geometry (A, B, kh x kw) and the edge it reaches:
    (1,1,1x1)            total = 1: one dot block, its partial parked in a one-element dW
    (7,3,3x3)            A < 8 row lanes, Wd = 27 < 32, Cin = 3 -> pad_in = 8, A % 4 != 0
    (9,5,1x1)            the four-accumulator loop of wt_u_columns does not run; stride-8 tail; pad_in = 8
    (33,20,1x1)          one four-accumulator round, then a one-row tail; pad_in = 24
    (57,34,3x3)          lane 0 takes a second round (32 + 24 < 57); Wd = 306 is no multiple of 32 or 64; pad_in = 40
    (64,40,4x4) T        16 taps, transposed: dW in [Cin][Cout][taps] order
    (20,32,4x4) T        16 taps, transposed, padding along A (20 -> 24)
    (300,70,1x3)         non-square taps; A > 256 and Wd = 210 < 256 in sn_norms
    (256,256,3x3)        589 824 outputs wrap the 2048-block grid of sn_finish_kernel; all 256 dot blocks run
B. one plan over (7,3,3x3), plain (24,8,3x3), (33,20,1x1), (17,34,3x3) [last b tile nb = 2: scalar load and store], (20,32,4x4) T,
   (64,40,4x4) T, plain (3,5,1x1) [numel 15, n_out 24: every offset rounding], (48,64,1x1) [fully vectorised]; bf16 / f16 / fp32.
C. one conv of more than 256 tiles: (512,512,4x4) T (512 tiles) and (512,512,3x3) (512 tiles), bf16: the second round of the stride-256 partial
   sum in snb_bwd_apply_kernel.
D. batched and per-conv at (64,40,3x3) and (32,64,1x1), both against the same float64 reference.
E. a parameter 4 bytes off a 16-byte boundary: the scalar branch of sn_load_param_tile at a vector-friendly shape.
F. plain_krsc with a stale epoch or another dtype: the fresh conversion.

Measured err / (u32 S) on the MI355X (largest over all cases of this file; S includes the inherited budget C / k, see weights_reference.py) and
the k in use:

    output                                   measured                      k
    v' (per-conv, 2nd call, batched, big)    0.43, 0.86, 0.43, 0.17        k_v(Wd) = k_norm(Wd) + 4          (10 .. 16)
    u' (per-conv, 2nd call, batched, big)    0.094, 0.127, 0.094, 0.010    k_u(A) = k_norm(A) + 5            (11 .. 15)
    sigma (per-conv, 2nd call)               0.101, 0.141                  k_sigma(A) = k_norm(A) + 5        (11 .. 13)
    out fp32 (per-conv, 2nd call, batched)   0.038, 0.057, 0.038           K_OUT 3
    twin fp32 (batched)                      0.038                         K_OUT 3
    out / twin bf16, f16 (all)               0.000 (absorbed by u_out)     K_OUT 3
    dW (per-conv, batched, big)              0.118, 0.087, 0.019           K_DW 8
    misaligned parameter: v', u', out, dW    0.160, 0.073, 0.020, 0.051    as above

Every k is an operation count and was not fitted. Those of u', sigma and dW stand 100, 90 and 68 times above what was measured (out: 53, v': 14):
S carries, next to the element's own terms, the budget inherited along t -> v' -> s -> u' -> sigma, and every link hands it on through |W| and
through the norm as a sum of absolute values, as if all rounding errors of the links before it had the same sign; on the device they have random
signs, and u' and sigma do not change at all when v' is merely scaled, which the inherited part counts in full. For v', whose S holds one link
only, the margin is 14. The plain and absent-gradient entries, the twins against their weights, the twin-layout gradients, the GRAD_DEST
destinations, the misaligned parameter against the aligned one and the repeated runs are compared bit for bit and have no k.

The channel padding of every weight and the padded rows of every twin were +0 in blocks that held NaN before the call; the 16-float gaps between
the GRAD_DEST slices stayed NaN. The `out` buffer of a plan has no gaps to check: pad_in is a multiple of 8, so every n_out is one and the
rounding of out_off to 8 never moves an offset (the assertion counts the gap elements and finds 0); work_off and dw_off do get rounded in list B.
An absent gradient reaches SpectralNormBatch.backward as a zero tensor (autograd materialises it), so the kernels' NULL-entry branch is not
reachable through torch.autograd.grad; the zero dW is asserted all the same.

Run time on the MI355X: the 39 cases take 8.6 s together; the slowest are (512,512,4x4) T at 1.8 s and the bf16 mixed list at 1.1 s (first use of
the kernels included), every other case stays below 0.4 s.
"""
import numpy as np
import pytest
import torch

import weights_reference as R

pytestmark = pytest.mark.gpu

BF16, F16, F32 = R.BF16, R.F16, R.F32
DTYPES = [F32, BF16, F16]
_dt = lambda d: str(d).replace('torch.', '')      # noqa: E731


def _dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


_refs = {}


def _ref(g):
    """(W, u0, v0, forward reference) of a geometry: built once, shared by the dtypes and tests that use it, never changed."""
    if g not in _refs:
        W, u = R.make_w(g), R.make_u(g)
        _refs[g] = (W, u, R.make_v(g), R.forward_reference(W, u, g.transposed, g.pad_in))
    return _refs[g]


def _poison(shape, dtype, dev, count=1):
    """Allocate `count` NaN-filled buffers and free them: the caching allocator hands the very same blocks to the next torch.empty calls of that
    size, so an element the kernel fails to write (channel padding, a gap it should not touch) is NaN, not a zero left over from an earlier
    test. Returns the addresses so the caller can check that the blocks did come back."""
    ts = [torch.full(shape, float('nan'), dtype=dtype, device=dev) for _ in range(count)]
    ptrs = [t.data_ptr() for t in ts]
    del ts
    return ptrs


def _same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def _check_forward(g, ref, dtype, out, u, v, sigma, tag):
    R.check(v, ref['v'], R.k_v(g.Wd), F32, tag + ' v')
    R.check(u, ref['u'], R.k_u(g.A), F32, tag + ' u')
    if sigma is not None:
        R.check(sigma, ref['sigma'], R.k_sigma(g.A), F32, tag + ' sigma')
    assert out.dtype == dtype
    R.check(out, ref['out'], R.K_OUT, dtype, tag + ' out')
    assert R.padding_is_zero(out, g.cin), 'channel padding of %s is not +0' % g


# ------------------------------------------------------------------------------------------------------------------
# A. per-conv kernels
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=_dt)
@pytest.mark.parametrize('g', [g for g, _ in R.PER_CONV], ids=str)
def test_per_conv_forward_and_backward(g, dtype):
    from maggie_amd import kernels as K
    dev = _dev()
    W, u0, v0, ref = _ref(g)
    Wd = W.to(dev)

    def forward(u, v):
        # `out` comes from torch.empty inside kernels.spectral_norm: poison the block it will get (see _poison)
        (p,) = _poison((g.cout, g.taps, g.pad_in), dtype, dev)
        out, work = K.spectral_norm(Wd, u, v, g.transposed, dtype, g.pad_in)
        assert out.data_ptr() == p, 'the poisoned block did not come back'
        return out, work

    u, v = u0.to(dev), v0.to(dev)
    out, work = forward(u, v)
    assert out.shape == (g.cout, g.taps, g.pad_in)
    _check_forward(g, ref, dtype, out, u, v, work[-1:], 'per-conv')

    # two runs from the same state give the same bits
    ub, vb = u0.to(dev), v0.to(dev)
    outb, workb = forward(ub, vb)
    n = g.Wd + g.A
    assert _same_bits(out, outb) and _same_bits(u, ub) and _same_bits(v, vb)
    assert _same_bits(work[:n + 2], workb[:n + 2]) and _same_bits(work[-1:], workb[-1:])

    # backward with the vectors after the iteration; the padded channels of G hold NaN and must not be read
    G = R.make_g(g, dtype)
    want = R.backward_reference(G, W, ref, g.transposed)
    Gd = G.float().to(dev)
    dW = K.spectral_norm_bwd(Gd, Wd, u, v, g.transposed, work)
    assert dW.shape == W.shape and dW.dtype == F32                 # the parameter's own order: [Cin][Cout][taps] for a transposed conv
    R.check(dW.reshape(g.A, g.B, g.taps), want, R.K_DW, F32, 'per-conv dW')
    assert _same_bits(dW, K.spectral_norm_bwd(Gd, Wd, u, v, g.transposed, work))

    # a second call from the updated u, v against a second reference iteration from the very fp32 u the first call wrote
    u1 = u.cpu().clone()
    ref2 = R.forward_reference(W, u1, g.transposed, g.pad_in)
    out2, work2 = forward(u, v)
    _check_forward(g, ref2, dtype, out2, u, v, work2[-1:], 'per-conv 2nd')


# ------------------------------------------------------------------------------------------------------------------
# B. the batched pipeline over a mixed list
# ------------------------------------------------------------------------------------------------------------------
def _module(g, plain, dev):
    """A SpectralNorm wrapper (or a plain ConvWeight) holding the case's W, u, v."""
    from maggie_amd.network.module import ConvWeight, SpectralNorm
    assert g.kh == g.kw
    cw = ConvWeight(g.cin, g.cout, g.kh, 1, g.kh // 2, 1, transposed=bool(g.transposed))
    W, u, v, _ = _ref(g) if not plain else (R.make_w(g), None, None, None)
    assert tuple(cw.weight.shape) == tuple(W.shape)
    cw.weight.data.copy_(W)
    if plain:
        return cw.to(dev)
    m = SpectralNorm(cw)
    m.module.weight_u.data.copy_(u)
    m.module.weight_v.data.copy_(v)
    return m.to(dev)


def _param(m):
    return m.module.weight_bar if hasattr(m, 'module') else m.weight


def _flat(t, n):
    """The whole flat buffer a slice `t` of it was cut from (t starts the buffer)."""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), 0, (n,))


def _prepare(mods, dtype, dev, poison=True):
    """functional.spectral_norm_prepare on a plan built beforehand, so that the three torch.empty of SpectralNormBatch.forward (out, out_t, work)
    are the next allocations after the poison. -> (plan, prepared weights)"""
    from maggie_amd import functional as MF
    MF.ARENA.reset(dev)
    cache = {'plan': MF.SpectralNormPlan(mods, dtype)}
    plan = cache['plan']
    if poison:
        ptrs = _poison((plan.total_out,), dtype, dev, count=2)
    MF.spectral_norm_prepare(mods, dtype, cache)
    assert cache['plan'] is plan
    outs = [m.__dict__['_prepared'] for m in mods]
    if poison:
        # out and its twin buffer have the same size: whichever of the two poisoned blocks each one got, both are poisoned
        assert {outs[0].data_ptr(), outs[0]._mg_wt.data_ptr()} == set(ptrs), 'the poisoned blocks did not come back'
    return plan, outs


def _gaps_untouched(flat, plan):
    """-> (elements of the flat buffer that lie between the slices of the plan, whether all of them are still NaN)."""
    keep = torch.ones(flat.numel(), dtype=torch.bool)
    for o, n in plan.out_slices:
        keep[o:o + n] = False
    gaps = flat.detach().cpu().float()[keep]
    return gaps.numel(), bool(torch.isnan(gaps).all())


@pytest.mark.parametrize('dtype', [BF16, F16, F32], ids=_dt)
def test_batched_pipeline_mixed_list(dtype):
    from maggie_amd import functional as MF
    dev = _dev()
    mods = [_module(g, plain, dev) for g, plain in R.BATCH_LIST]
    params = [_param(m) for m in mods]
    state = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    grads = [R.make_g(g, dtype).to(dev) for g, _ in R.BATCH_LIST]        # NaN in the padded channels: never read

    def run(twin_layout, dest=None):
        for m, sd in zip(mods, state):
            m.load_state_dict(sd)
        plan, outs = _prepare(mods, dtype, dev)
        fed = [G.permute(2, 1, 0).contiguous().permute(2, 1, 0) if (twin_layout and g.transposed) else G for (g, _), G in zip(R.BATCH_LIST, grads)]
        live = [i for i in range(len(mods)) if i != R.BATCH_NO_GRAD]
        if dest is not None:
            MF.GRAD_DEST.update({id(p): d for p, d in zip(params, dest)})
        try:
            got = torch.autograd.grad([outs[i] for i in live], params, [fed[i] for i in live], allow_unused=True)
        finally:
            MF.GRAD_DEST.clear()
        return plan, outs, got

    plan, outs, got = run(False)

    # offsets: rounded to 8 (out), 4 (work), 4 (dW) elements between the convs
    o_out = o_dw = 0
    for (g, _), (oo, n), (od, nd) in zip(R.BATCH_LIST, plan.out_slices, plan.dw_slices):
        assert (oo, n, od, nd) == (o_out, g.n_out, o_dw, g.numel)
        o_out += (g.n_out + 7) // 8 * 8
        o_dw += (g.numel + 3) // 4 * 4
    assert plan.total_out == o_out and plan.total_dw == o_dw
    assert plan.total_work == sum((g.Wd + g.A + 4 + 3) // 4 * 4 for g, _ in R.BATCH_LIST)

    # forward: SN entries against float64, plain entries bit-equal to the permuted parameter cast once
    for (g, plain), m, w in zip(R.BATCH_LIST, mods, outs):
        wt = w._mg_wt
        assert w.shape == (g.cout, g.taps, g.pad_in) and wt.shape == (g.pad_in, g.taps, g.cout) and w.dtype == dtype and wt.dtype == dtype
        if plain:
            want = torch.from_numpy(R.plain_krsc(R.make_w(g), g.pad_in)).to(dtype)
            assert _same_bits(w, want), 'plain %s' % g
            assert _same_bits(wt, want.permute(2, 1, 0).contiguous()), 'plain twin %s' % g
            continue
        ref = _ref(g)[3]
        _check_forward(g, ref, dtype, w, m.module.weight_u.data, m.module.weight_v.data, None, 'batched')
        R.check(wt, ref['twin'], R.K_OUT, dtype, 'batched twin')
        assert R.twin_padding_is_zero(wt, g.cin), 'padded rows of the twin of %s are not +0' % g
        assert _same_bits(wt, w.permute(2, 1, 0).contiguous())
    # nothing written between the slices of out and of the twin buffer
    for first in (outs[0], outs[0]._mg_wt):
        n_gap, ok = _gaps_untouched(_flat(first, plan.total_out), plan)
        assert n_gap == plan.total_out - sum(g.n_out for g, _ in R.BATCH_LIST) and ok
    # gradients
    want_dw = {}
    for i, ((g, plain), p, G, d) in enumerate(zip(R.BATCH_LIST, params, grads, got)):
        assert d.dtype == F32 and d.shape == p.shape
        if i == R.BATCH_NO_GRAD:
            assert not bool(d.detach().cpu().ne(0).any()), 'an absent gradient must give dW = 0'
            continue
        if plain:
            want = torch.from_numpy(R.grad_to_param(G.float(), g.A, g.B, g.taps, 0)).float().reshape(p.shape)
            assert _same_bits(d, want), 'plain dW %s' % g
            continue
        want_dw[i] = R.backward_reference(G, _ref(g)[0], _ref(g)[3], g.transposed)
        R.check(d.reshape(g.A, g.B, g.taps), want_dw[i], R.K_DW, F32, 'batched dW')

    # the twin layout for the transposed entries: the same bits; and two runs from the same saved state give the same bits
    _, outs2, got2 = run(True)
    for a, b in zip(got, got2):
        assert _same_bits(a, b)
    for m, sd, a, b in zip(mods, state, outs, outs2):
        assert _same_bits(a, b) and _same_bits(a._mg_wt, b._mg_wt)
    u_after = [m.module.weight_u.data.clone() for m in mods if hasattr(m, 'module')]
    _, outs3, got3 = run(False)
    for a, b in zip(got, got3):
        assert _same_bits(a, b)
    for a, b in zip(outs, outs3):
        assert _same_bits(a, b)
    for a, m in zip(u_after, [m for m in mods if hasattr(m, 'module')]):
        assert _same_bits(a, m.module.weight_u.data)

    # GRAD_DEST: slices of one NaN-filled flat buffer with 16-float gaps
    flat = torch.full((sum(p.numel() + 16 for p in params),), float('nan'), device=dev)
    dest, keep, o = [], torch.ones(flat.numel(), dtype=torch.bool), 0
    for p in params:
        dest.append(flat[o:o + p.numel()].view(p.shape))
        keep[o:o + p.numel()] = False
        o += p.numel() + 16
    _, _, got4 = run(True, dest)
    for a, b, d in zip(got4, got, dest):
        assert a.data_ptr() == d.data_ptr() and _same_bits(a, b) and _same_bits(d, b)
    assert bool(torch.isnan(flat.cpu()[keep]).all()) and int(keep.sum()) == 16 * len(params)


# ------------------------------------------------------------------------------------------------------------------
# C. more than 256 tiles in one conv
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('g', R.BIG, ids=str)
def test_batched_conv_of_more_than_256_tiles(g):
    dev = _dev()
    dtype = BF16
    m = _module(g, 0, dev)
    plan, (w,) = _prepare([m], dtype, dev)
    assert plan.k3.shape[0] == 512 > 256
    W, _, _, ref = _ref(g)
    _check_forward(g, ref, dtype, w, m.module.weight_u.data, m.module.weight_v.data, None, 'big')
    R.check(w._mg_wt, ref['twin'], R.K_OUT, dtype, 'big twin')
    G = R.make_g(g, dtype)
    (d,) = torch.autograd.grad([w], [_param(m)], [G.to(dev)])
    R.check(d.reshape(g.A, g.B, g.taps), R.backward_reference(G, W, ref, g.transposed), R.K_DW, F32, 'big dW')


# ------------------------------------------------------------------------------------------------------------------
# D. batched and per-conv against the same reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=_dt)
def test_batched_and_per_conv_agree_with_float64(dtype):
    """The geometries of test_batched_weight_pipeline_mixes_spectral_norm_and_plain_convs (test_gpu_kernels.py), whose atol = 1e-6 between the
    two implementations stands here next to the stated bound of each against float64."""
    from maggie_amd import kernels as K
    dev = _dev()
    mods = [_module(g, 0, dev) for g in R.AGREE]
    _, outs = _prepare(mods, dtype, dev)
    for g, m, w in zip(R.AGREE, mods, outs):
        W, u0, v0, ref = _ref(g)
        Wd, u, v = W.to(dev), u0.to(dev), v0.to(dev)
        out, work = K.spectral_norm(Wd, u, v, 0, dtype, g.pad_in)
        _check_forward(g, ref, dtype, out, u, v, work[-1:], 'per-conv')
        _check_forward(g, ref, dtype, w, m.module.weight_u.data, m.module.weight_v.data, None, 'batched')
        assert torch.allclose(m.module.weight_u.data, u, atol=1e-6) and torch.allclose(m.module.weight_v.data, v, atol=1e-6)
        G = R.make_g(g, dtype)
        want = R.backward_reference(G, W, ref, 0)
        R.check(K.spectral_norm_bwd(G.float().to(dev), Wd, u, v, 0, work).reshape(g.A, g.B, g.taps), want, R.K_DW, F32, 'per-conv dW')
        (d,) = torch.autograd.grad([w], [_param(m)], [G.to(dev)], retain_graph=True)
        R.check(d.reshape(g.A, g.B, g.taps), want, R.K_DW, F32, 'batched dW')


# ------------------------------------------------------------------------------------------------------------------
# E. alignment fall-back of the parameter load
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES, ids=_dt)
def test_batched_parameter_off_a_16_byte_boundary(dtype):
    dev = _dev()
    g = R.MISALIGNED
    W, _, _, ref = _ref(g)
    aligned, shifted = _module(g, 0, dev), _module(g, 0, dev)
    buf = torch.zeros(g.numel + 8, device=dev)
    view = buf[1:1 + g.numel].view(W.shape)
    view.copy_(W)
    shifted.module.weight_bar.data = view
    assert aligned.module.weight_bar.data_ptr() % 16 == 0 and shifted.module.weight_bar.data_ptr() % 16 == 4
    G = R.make_g(g, dtype)
    res = []
    for m in (aligned, shifted):
        _, (w,) = _prepare([m], dtype, dev)
        (d,) = torch.autograd.grad([w], [_param(m)], [G.to(dev)])
        res.append((w, w._mg_wt, m.module.weight_u.data, m.module.weight_v.data, d))
    for a, b in zip(*res):
        assert _same_bits(a, b)
    w, wt, u, v, d = res[1]
    _check_forward(g, ref, dtype, w, u, v, None, 'shifted')
    R.check(wt, ref['twin'], R.K_OUT, dtype, 'shifted twin')
    R.check(d.reshape(g.A, g.B, g.taps), R.backward_reference(G, W, ref, 0), R.K_DW, F32, 'shifted dW')
    assert float(buf[0]) == 0 and not bool(buf[1 + g.numel:].ne(0).any())


# ------------------------------------------------------------------------------------------------------------------
# F. the prepared-weight cache
# ------------------------------------------------------------------------------------------------------------------
def test_plain_krsc_falls_back_to_a_fresh_conversion():
    from maggie_amd import functional as MF
    dev = _dev()
    g = R.G_(24, 8, 3)
    conv = _module(g, 1, dev)
    _prepare([_module(R.G_(7, 3, 3), 0, dev), conv], BF16, dev, poison=False)
    prepared = conv.__dict__['_prepared']
    assert MF.plain_krsc(conv, BF16, keep=True) is prepared
    # another dtype than the plan's
    other = MF.plain_krsc(conv, F16, keep=True)
    assert other is not prepared and other.dtype == F16
    assert _same_bits(other.detach(), MF.weight_oihw_to_krsc(conv.weight.detach(), F16))
    assert _same_bits(other.detach(), torch.from_numpy(R.plain_krsc(R.make_w(g), g.pad_in)).to(F16))
    # a stale epoch: the parameter has changed since and a new step has begun
    with torch.no_grad():
        conv.weight.mul_(2.0)
    MF.ARENA.reset(dev)
    assert conv.__dict__['_prepared_epoch'] != MF.ARENA.epoch
    fresh = MF.plain_krsc(conv, BF16, keep=True)
    assert fresh is not prepared
    assert _same_bits(fresh.detach(), torch.from_numpy(R.plain_krsc(R.make_w(g) * 2, g.pad_in)).to(BF16))
    assert not _same_bits(fresh.detach(), prepared.detach())
