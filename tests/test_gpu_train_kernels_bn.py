"""GPU: the trainer's BatchNorm kernels of csrc/train.hip (statistics, apply,
stem BN + ReLU + max-pool, backward), each called through its C entry and
compared, element for element, with the same operation in float64 torch on the
same input values (bf16 cases: fp32 data rounded to bf16, both sides get the
rounded values).  Gradients are compared with float64 autograd.

Every bar is an a-priori rounding bound, computed here from the data and the
launch geometry with u = 2^-24 (one fp32 rounding); none is a measured error.
Every test prints its worst error / bar ratio.

Launch geometry (bn_nblocks / bn_reduce_kernel).  A thread owns 8 channels of
one row; a workgroup covers R = 256 / (C / 8) rows per pass (C = 8: 256,
C = 24: 85, C = 64: 32, C = 136: 15, C = 2048: 1) and the grid is
ceil(P / (16 R)) workgroups, at most 1024.  So a thread adds at most 16 rows
below the cap and ceil(P / (1024 R)) rows at it (P = 16389, C = 2048: 17); the
LDS combine then adds R thread sums; the per-workgroup partials are summed in
float64 (no error that counts).

Sum bound.  A kernel sum of fp32 terms t_i is held to K u sum|t_i| with
K = rows_per_thread + R + 8 (the 8 covers the roundings inside a term).

Elementwise bound.  An fp32 elementwise result is held to 8 u (sum of its
operands' magnitudes) plus the propagated bound of what it consumes.  A result
stored as bf16 adds 2^-8 |ref|.

Statistics.  S = sum x, Q = sum x^2, mean = S / P, var = Q / P - mean^2 (float64):
  e_S     = K u sum|x| / P                       (error of S / P)
  e_mean  = e_S + 8 u |mean|
  e_var   = K u sum x^2 / P + 2 |mean| e_S + e_S^2
  e_istd  = max(istd(max(var - e_var, 0)) - istd(var), istd(var) - istd(var + e_var))
            + 8 u istd        (istd = (var + eps)^-1/2 is monotone; var is clamped at 0,
            so with var ~ 0 the upper end is the one that moves)
  e_scale = |gamma| e_istd + 8 u |scale|
  e_shift = (|mean| + e_mean) e_scale + |scale| e_mean + 8 u (|beta| + |mean scale|)
  running mean: momentum e_S + 8 u (|(1-momentum) rm| + |momentum mean|)
  running var:  momentum e_var P/(P-1) + 8 u (|(1-momentum) rv| + |momentum unbiased|)
The running statistics are F.batch_norm's (float64, training, the fp32 value of
momentum 0.1).  F.batch_norm refuses P = 1 (one value per channel); there the
kernel's guard defines the reference: the unbiased variance is the biased one (0).

Apply / max-pool.  y = x scale + shift (+ res | + res rscale + rshift):
8 u (|x scale| + |shift| + |res rscale| + |rshift|); ReLU and max are
1-Lipschitz, so a pooled output is held to the largest bar in its window.

Backward.  With dz = dy [y > 0] (or dpool / hw [y > 0]), xhat = (x - mean) istd:
  e_xhat  = (8 u (|x| + |mean|) + e_mean) (istd + e_istd) + |x - mean| e_istd
            (isolated: stats are the float64 statistics rounded to fp32, so
            e_mean = u |mean|, e_istd = u istd; chained: the statistics bars)
  e_dz    = 0 for a dy tensor, 8 u |dz| for dpool / hw; as re-read from a
            stored dz_out: that bar plus 2^-8 |dz| in bf16
  e_s     = K u sum|dz| + sum e_dz                         -> dbeta  (+ 8 u (|s| + |previous|))
  e_q     = K u sum|dz xhat| + sum(|dz| e_xhat + e_dz (|xhat| + e_xhat))   -> dgamma (same)
  c0 = gamma istd, c1 = s / P, c2 = q / P with e_c0 = |gamma| e_istd + 8 u |c0|,
  e_c1 = e_s / P + 8 u |c1|, e_c2 = e_q / P + 8 u |c2|
  inner = dz - c1 - xhat c2:
  e_inner = e_dz + e_c1 + |xhat| e_c2 + (|c2| + e_c2) e_xhat + 8 u (|dz| + |c1| + |xhat c2|)
  dx = c0 inner:  (|c0| + e_c0) e_inner + e_c0 |inner| + 8 u |dx|
The reference's own forward gives y (and so the mask), so |y| ~ 0 is not
ambiguous.  In the chained case (stats -> apply -> backward, every stage fed
by the kernel before it) the mask comes from the kernel's y: where the
reference |y| is within the forward bar of 0 the mask may differ, and such an
element carries e_dz = |dy| (the count is printed; no element is left out).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
BF = 2.0 ** -8
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))


def _dt(dtype):
    from sad import _lib
    return (_lib.SAD_BF16, torch.bfloat16) if dtype == 'bf16' else (_lib.SAD_F32, torch.float32)


def _stream():
    from sad import _lib
    return _lib.stream_handle(torch.device(DEV))


def _geom(P, C):
    """(R, workgroups, K) of bn_nblocks / bn_reduce_kernel."""
    R = 256 // (C // 8)
    want = -(-P // (R * 16))
    nb = max(1, min(1024, want))
    rows = 16 if want <= 1024 else -(-P // (1024 * R))
    return R, nb, rows + R + 8


def _ws(P, C):
    from sad import _lib
    sz = _lib.SZ()
    _lib.call('sad_bn_workspace_size', P, C, _lib.ctypes.byref(sz))
    assert sz.value == (_geom(P, C)[1] * 2 * C + 3 * C) * 4
    return torch.zeros(sz.value // 4, device=DEV), sz.value


def _report(name, got, ref, bar):
    """Worst err / bar over all elements; asserts err <= bar everywhere."""
    err = (got.double() - ref).abs().flatten()
    bar = bar.double().expand_as(ref).flatten()
    assert err.numel() == bar.numel() and err.numel() > 0
    assert torch.isfinite(err).all(), f'{name}: non-finite error'
    ratio = torch.where(err > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    print(f'{name}: worst err {err[i].item():.3e} vs bar {bar[i].item():.3e} (ratio {ratio[i].item():.3f}, '
          f'max err {err.max().item():.3e})')
    assert (err <= bar).all(), f'{name}: err {err[i].item():.3e} > bar {bar[i].item():.3e}'


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _affine(C, gen):
    gamma = torch.randn(C, generator=gen, device=DEV) * 0.5 + 1.0
    gamma[1::5] *= -1.0                       # negative gamma
    beta = torch.randn(C, generator=gen, device=DEV) * 0.5
    return gamma, beta


def _bn_input(P, C, tdt, gen):
    """Per-channel mean in [-4, 4] std, std in [0.5, 2]; channel C - 3 is constant."""
    m = torch.rand(C, generator=gen, device=DEV) * 8.0 - 4.0
    s = torch.rand(C, generator=gen, device=DEV) * 1.5 + 0.5
    x = (torch.randn(P, C, generator=gen, device=DEV) + m) * s
    x[:, C - 3] = 0.75
    return x.to(tdt)


# ------------------------------------------------------------ statistics --
def _stats_ref(x64, gamma, beta, K):
    """float64 statistics of x64 [P, C] and the bars of the module docstring."""
    P = x64.shape[0]
    g, b = gamma.double(), beta.double()
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    e_S = K * U * x64.abs().sum(0) / P
    e_var = K * U * (x64 * x64).sum(0) / P + 2 * mean.abs() * e_S + e_S * e_S
    istd = (var + EPS).rsqrt()
    e_istd = torch.maximum(((var - e_var).clamp_min(0) + EPS).rsqrt() - istd,
                           istd - (var + e_var + EPS).rsqrt()) + 8 * U * istd
    scale = g * istd
    e_mean = e_S + 8 * U * mean.abs()
    e_scale = g.abs() * e_istd + 8 * U * scale.abs()
    shift = b - mean * scale
    e_shift = (mean.abs() + e_mean) * e_scale + scale.abs() * e_mean + 8 * U * (b.abs() + (mean * scale).abs())
    return dict(mean=mean, var=var, istd=istd, scale=scale, shift=shift, e_S=e_S, e_mean=e_mean, e_var=e_var,
                e_istd=e_istd, e_scale=e_scale, e_shift=e_shift,
                stats=torch.cat([mean, istd, scale, shift]), e_stats=torch.cat([e_mean, e_istd, e_scale, e_shift]))


def _stats_run(x, P, C, code, gamma, beta, rm=None, rv=None):
    from sad import _lib
    stats = torch.full((4 * C,), float('nan'), device=DEV)
    ws, nbytes = _ws(P, C)
    _lib.call('sad_bn_stats_run', _lib.ptr(x), P, C, code, _lib.ptr(gamma), _lib.ptr(beta), EPS, MOM, _lib.ptr(rm),
              _lib.ptr(rv), _lib.ptr(stats), _lib.ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()
    return stats


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('P,C', [(1, 8), (7, 24), (4097, 8), (513, 136), (1000, 64), (16389, 2048)])
def test_bn_stats_vs_float64(P, C, dtype):
    code, tdt = _dt(dtype)
    gen = _gen(P * 7 + C)
    x = _bn_input(P, C, tdt, gen)
    gamma, beta = _affine(C, gen)
    R, nb, K = _geom(P, C)
    x64 = x.double()
    r = _stats_ref(x64, gamma, beta, K)
    rm0 = torch.randn(C, generator=gen, device=DEV)
    rv0 = torch.rand(C, generator=gen, device=DEV) + 0.5
    rm64, rv64 = rm0.double(), rv0.double()
    if P > 1:
        F.batch_norm(x64, rm64, rv64, gamma.double(), beta.double(), True, MOM, EPS)   # updates rm64 / rv64
        unb = r['var'] * P / (P - 1)
        assert torch.allclose(rv64, (1 - MOM) * rv0.double() + MOM * unb, rtol=1e-9, atol=1e-12)
    else:
        with pytest.raises(ValueError):
            F.batch_norm(x64, rm64, rv64, gamma.double(), beta.double(), True, MOM, EPS)
        unb = r['var']                           # the kernel's P == 1 guard
        rm64 = (1 - MOM) * rm0.double() + MOM * r['mean']
        rv64 = (1 - MOM) * rv0.double() + MOM * unb
    tag = f'bn_stats {dtype} P{P} C{C} (R {R}, {nb} wg, K {K})'
    rm, rv = rm0.clone(), rv0.clone()
    stats = _stats_run(x, P, C, code, gamma, beta, rm, rv)
    _report(f'{tag} stats', stats, r['stats'], r['e_stats'])
    _report(f'{tag} running_mean', rm, rm64,
            MOM * r['e_S'] + 8 * U * (((1 - MOM) * rm0.double()).abs() + (MOM * r['mean']).abs()))
    _report(f'{tag} running_var', rv, rv64,
            MOM * r['e_var'] * (P / (P - 1) if P > 1 else 1.0)
            + 8 * U * (((1 - MOM) * rv0.double()).abs() + (MOM * unb).abs()))
    # the constant channel: 0.75 n and 0.5625 n are exact in fp32, so var = 0 exactly
    assert stats[C + C - 3].item() == pytest.approx(EPS ** -0.5, rel=1e-6)
    # running_mean = running_var = NULL
    stats2 = _stats_run(x, P, C, code, gamma, beta)
    _report(f'{tag} stats, no running stats', stats2, r['stats'], r['e_stats'])
    assert torch.equal(stats2, stats)


# ------------------------------------------------------------ apply --
def _rand_stats(C, gen):
    """[mean | invstd | scale | shift] with scale of both signs; apply reads only the last two."""
    st = torch.full((4 * C,), float('nan'), device=DEV)
    sign = torch.ones(C, device=DEV)
    sign[1::2] = -1.0
    st[2 * C:3 * C] = (torch.randn(C, generator=gen, device=DEV).abs() * 1.5 + 0.1) * sign
    st[3 * C:] = torch.randn(C, generator=gen, device=DEV) - 0.25
    return st


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('P,C', [(1, 8), (37, 24), (300, 136)])
def test_bn_apply_vs_float64(P, C, dtype):
    from sad import _lib
    code, tdt = _dt(dtype)
    gen = _gen(P + C)
    x = (torch.randn(P, C, generator=gen, device=DEV) * 3.0).to(tdt)
    res = (torch.randn(P, C, generator=gen, device=DEV) * 2.0).to(tdt)
    st, rst = _rand_stats(C, gen), _rand_stats(C, gen)
    assert (st[2 * C:3 * C] < 0).any() and (st[2 * C:3 * C] > 0).any()
    sc, sh = st[2 * C:3 * C].double(), st[3 * C:].double()
    rsc, rsh = rst[2 * C:3 * C].double(), rst[3 * C:].double()
    for res_mode in ('none', 'res', 'res_stats'):
        pre = x.double() * sc + sh
        mag = (x.double() * sc).abs() + sh.abs()
        if res_mode == 'res':
            pre, mag = pre + res.double(), mag + res.double().abs()
        elif res_mode == 'res_stats':
            pre, mag = pre + res.double() * rsc + rsh, mag + (res.double() * rsc).abs() + rsh.abs()
        for relu in (0, 1):
            ref = pre.clamp_min(0) if relu else pre
            out = torch.full((P, C), float('nan'), dtype=tdt, device=DEV)
            _lib.call('sad_bn_apply_run', _lib.ptr(x), P, C, code, _lib.ptr(st),
                      _lib.ptr(res) if res_mode != 'none' else None,
                      _lib.ptr(rst) if res_mode == 'res_stats' else None, relu, _lib.ptr(out), _stream())
            torch.cuda.synchronize()
            bar = 8 * U * mag + (BF * ref.abs() if dtype == 'bf16' else 0)
            _report(f'bn_apply {dtype} P{P} C{C} {res_mode} relu {relu}', out, ref, bar)
            if relu:
                assert (out >= 0).all()


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_bn_apply_empty_writes_nothing(dtype):
    from sad import _lib
    code, tdt = _dt(dtype)
    x = torch.ones(8, dtype=tdt, device=DEV)
    st = torch.ones(32, device=DEV)
    out = torch.full((64,), 1.5, dtype=tdt, device=DEV)
    _lib.call('sad_bn_apply_run', _lib.ptr(x), 0, 8, code, _lib.ptr(st), None, None, 1, _lib.ptr(out), _stream())
    _lib.call('sad_bn_relu_maxpool_run', _lib.ptr(x), 0, 4, 4, 8, code, _lib.ptr(st), _lib.ptr(out), _stream())
    torch.cuda.synchronize()
    assert (out.float() == 1.5).all()


@pytest.mark.parametrize('C', [4, 12, 2056])
def test_bn_apply_and_maxpool_refuse_unsupported_channels(C):
    from sad import _lib
    x = torch.zeros(4 * C, device=DEV)
    st = torch.zeros(4 * C, device=DEV)
    out = torch.full((4 * C,), 1.5, device=DEV)
    with pytest.raises(RuntimeError, match=r'multiple of 8 in \[8, 2048\]'):
        _lib.call('sad_bn_apply_run', _lib.ptr(x), 1, C, _lib.SAD_F32, _lib.ptr(st), None, None, 0, _lib.ptr(out),
                  _stream())
    with pytest.raises(RuntimeError, match=r'multiple of 8 in \[8, 2048\]'):
        _lib.call('sad_bn_relu_maxpool_run', _lib.ptr(x), 1, 1, 1, C, _lib.SAD_F32, _lib.ptr(st), _lib.ptr(out),
                  _stream())
    torch.cuda.synchronize()
    assert (out == 1.5).all()


# ------------------------------------------------------------ BN + ReLU + max-pool --
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('C', [8, 64])
@pytest.mark.parametrize('H,W', [(1, 1), (2, 3), (5, 7), (8, 8)])
def test_bn_relu_maxpool_vs_float64(H, W, C, dtype):
    from sad import _lib
    code, tdt = _dt(dtype)
    n = 2
    gen = _gen(H * 100 + W * 10 + C)
    x = (torch.randn(n, H, W, C, generator=gen, device=DEV) * 2.0).to(tdt)
    st = _rand_stats(C, gen)
    st[3 * C:] -= 1.0                        # many all-negative windows before the ReLU;
    st[3 * C], st[3 * C + 1] = -100.0, 100.0   # channel 0 always is, channel 1 never
    sc, sh = st[2 * C:3 * C].double(), st[3 * C:].double()
    assert (sc < 0).any() and (sc > 0).any()
    a = (x.double() * sc + sh).permute(0, 3, 1, 2)
    mag = ((x.double() * sc).abs() + sh.abs()).permute(0, 3, 1, 2)
    ref = F.max_pool2d(F.relu(a), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    bar = 8 * U * F.max_pool2d(mag, 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert ref.shape == (n, Ho, Wo, C)
    out = torch.full((n * Ho * Wo * C + 8,), -2.0, dtype=tdt, device=DEV)
    _lib.call('sad_bn_relu_maxpool_run', _lib.ptr(x), n, H, W, C, code, _lib.ptr(st), _lib.ptr(out), _stream())
    torch.cuda.synchronize()
    assert (out[-8:].float() == -2.0).all(), 'wrote past the pooled output'
    got = out[:-8].view(n, Ho, Wo, C)
    zeros = int((ref == 0).sum())
    _report(f'bn_relu_maxpool {dtype} {H}x{W} C{C} ({zeros}/{ref.numel()} windows all-negative)', got, ref,
            bar + (BF * ref.abs() if dtype == 'bf16' else 0))
    assert 0 < zeros < ref.numel()


# ------------------------------------------------------------ backward --
def _bwd_bars(x64, mean, istd, e_mean, e_istd, gamma64, dz, e_dz_sum, e_dz_apply, K, prev_dg, prev_db, bf16):
    """(dx, dgamma, dbeta) by the formula in float64 and their bars (module docstring)."""
    P = x64.shape[0]
    xh = (x64 - mean) * istd
    e_xh = (8 * U * (x64.abs() + mean.abs()) + e_mean) * (istd + e_istd) + (x64 - mean).abs() * e_istd
    s, q = dz.sum(0), (dz * xh).sum(0)
    e_s = K * U * dz.abs().sum(0) + e_dz_sum.sum(0)
    e_q = K * U * (dz * xh).abs().sum(0) + (dz.abs() * e_xh + e_dz_sum * (xh.abs() + e_xh)).sum(0)
    bar_db = e_s + 8 * U * (s.abs() + prev_db.abs())
    bar_dg = e_q + 8 * U * (q.abs() + prev_dg.abs())
    c0, c1, c2 = gamma64 * istd, s / P, q / P
    e_c0 = gamma64.abs() * e_istd + 8 * U * c0.abs()
    e_c1 = e_s / P + 8 * U * c1.abs()
    e_c2 = e_q / P + 8 * U * c2.abs()
    inner = dz - c1 - xh * c2
    e_inner = e_dz_apply + e_c1 + xh.abs() * e_c2 + (c2.abs() + e_c2) * e_xh \
        + 8 * U * (dz.abs() + c1.abs() + (xh * c2).abs())
    dx = c0 * inner
    bar_dx = (c0.abs() + e_c0) * e_inner + e_c0 * inner.abs() + 8 * U * dx.abs()
    if bf16:
        bar_dx = bar_dx + BF * dx.abs()
    return dict(dx=dx, dgamma=q, dbeta=s, bar_dx=bar_dx, bar_dg=bar_dg, bar_db=bar_db)


def _autograd(x64, gamma64, beta64, mode, dy64, dpool64, hw):
    """float64 autograd of avgpool?(relu?(batch_norm(x))): y, dz, dx, dgamma, dbeta."""
    P, C = x64.shape
    xr = x64.clone().requires_grad_()
    g, b = gamma64.clone().requires_grad_(), beta64.clone().requires_grad_()
    out = F.batch_norm(xr, None, None, g, b, True, 0.0, EPS)
    out.retain_grad()
    y = out if mode == 'dy' else F.relu(out)
    if mode == 'dpool':
        y.view(P // hw, hw, C).mean(1).backward(dpool64)
    else:
        y.backward(dy64)
    return y.detach(), out.grad, xr.grad, g.grad, b.grad


def _bwd_run(x, P, C, code, stats, gamma, dy, dpool, hw, y, dgamma, dbeta, accumulate, dz_out, dx):
    from sad import _lib
    ws, nbytes = _ws(P, C)
    _lib.call('sad_bn_backward_run', _lib.ptr(x), P, C, code, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(dy),
              _lib.ptr(dpool), hw, _lib.ptr(y), _lib.ptr(dgamma), _lib.ptr(dbeta), accumulate, _lib.ptr(dz_out),
              _lib.ptr(dx), _lib.ptr(ws), nbytes, _stream())
    torch.cuda.synchronize()


BWD_CASES = [(P, C, mode, 0) for (P, C) in [(7, 24), (513, 136), (1024, 64)] for mode in ('dy', 'dy_y')] + \
            [(7, 24, 'dpool', 1), (513, 136, 'dpool', 1), (1024, 64, 'dpool', 1), (1024, 64, 'dpool', 256),
             (196, 24, 'dpool', 49)]          # P = 4 * 49: the only way 49 divides P


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('P,C,mode,hw', BWD_CASES)
def test_bn_backward_vs_float64_autograd(P, C, mode, hw, dtype):
    code, tdt = _dt(dtype)
    bf16 = dtype == 'bf16'
    gen = _gen(P * 3 + C + hw + len(mode))
    x = _bn_input(P, C, tdt, gen)
    gamma, beta = _affine(C, gen)
    R, nb, K = _geom(P, C)
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    dy = dpool = None
    if mode == 'dpool':
        dpool = torch.randn(P // hw, C, generator=gen, device=DEV) * 0.3
    else:
        dy = (torch.randn(P, C, generator=gen, device=DEV) * 0.3).to(tdt)
    y64, dz, dx_ref, dg_ref, db_ref = _autograd(x64, g64, b64, mode, None if dy is None else dy.double(),
                                                None if dpool is None else dpool.double(), hw)
    y = None if mode == 'dy' else y64.to(tdt)
    if y is not None:
        assert torch.equal(y > 0, y64 > 0)     # rounding y kept the mask
    # stats: the float64 statistics rounded to fp32, so the backward is isolated
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    istd = (var + EPS).rsqrt()
    stats = torch.cat([mean, istd, g64 * istd, b64 - mean * g64 * istd]).float()
    e_mean, e_istd = U * mean.abs(), U * istd
    e_sum = 8 * U * dz.abs() if mode == 'dpool' else torch.zeros_like(dz)
    bar_dz = e_sum + (BF * dz.abs() if bf16 else 0)
    prev_dg = torch.randn(C, generator=gen, device=DEV)
    prev_db = torch.randn(C, generator=gen, device=DEV)
    zero = torch.zeros(C, dtype=torch.float64, device=DEV)
    tag = f'bn_backward {dtype} P{P} C{C} {mode}' + (f' hw{hw}' if hw else '') + f' (K {K})'
    for with_dz, accumulate, with_grads in [(0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 0, 0)]:
        pdg, pdb = (prev_dg.double(), prev_db.double()) if accumulate else (zero, zero)
        r = _bwd_bars(x64, mean, istd, e_mean, e_istd, g64, dz, e_sum, bar_dz if with_dz else e_sum, K, pdg, pdb, bf16)
        scale = dx_ref.abs().max().clamp_min(1e-30)
        assert ((r['dx'] - dx_ref).abs().max() / scale).item() < 1e-9       # the formula is what autograd computes
        dx = torch.full((P, C), float('nan'), dtype=tdt, device=DEV)
        dzo = torch.full((P, C), float('nan'), dtype=tdt, device=DEV) if with_dz else None
        dgm, dbt = (prev_dg.clone(), prev_db.clone()) if with_grads else (None, None)
        _bwd_run(x, P, C, code, stats, gamma, dy, dpool, hw, y, dgm, dbt, accumulate, dzo, dx)
        t = f'{tag} dz_out {with_dz} acc {accumulate} grads {with_grads}'
        _report(f'{t} dx', dx, dx_ref, r['bar_dx'])
        if with_dz:
            _report(f'{t} dz_out', dzo, dz, bar_dz)
        if with_grads:
            _report(f'{t} dgamma', dgm, dg_ref + pdg, r['bar_dg'])
            _report(f'{t} dbeta', dbt, db_ref + pdb, r['bar_db'])


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_bn_chain_stats_apply_backward(dtype):
    """stats -> apply -> backward at (513, 136), each stage fed by the kernel before it."""
    from sad import _lib
    code, tdt = _dt(dtype)
    bf16 = dtype == 'bf16'
    P, C = 513, 136
    gen = _gen(99)
    x = _bn_input(P, C, tdt, gen)
    gamma, beta = _affine(C, gen)
    dy = (torch.randn(P, C, generator=gen, device=DEV) * 0.3).to(tdt)
    R, nb, K = _geom(P, C)
    x64, g64, b64 = x.double(), gamma.double(), beta.double()
    r = _stats_ref(x64, gamma, beta, K)
    y64, dz, dx_ref, dg_ref, db_ref = _autograd(x64, g64, b64, 'dy_y', dy.double(), None, 0)
    stats = _stats_run(x, P, C, code, gamma, beta)
    _report(f'chain {dtype} stats', stats, r['stats'], r['e_stats'])
    y = torch.full((P, C), float('nan'), dtype=tdt, device=DEV)
    _lib.call('sad_bn_apply_run', _lib.ptr(x), P, C, code, _lib.ptr(stats), None, None, 1, _lib.ptr(y), _stream())
    torch.cuda.synchronize()
    pre = x64 * r['scale'] + r['shift']
    assert (pre.clamp_min(0) - y64).abs().max().item() < 1e-9
    bar_pre = x64.abs() * r['e_scale'] + r['e_shift'] + 8 * U * ((x64 * r['scale']).abs() + r['shift'].abs())
    _report(f'chain {dtype} y', y, y64, bar_pre + (BF * y64.abs() if bf16 else 0))
    ambiguous = pre.abs() <= bar_pre
    e_dz = torch.where(ambiguous, dy.double().abs(), torch.zeros_like(dz))
    print(f'chain {dtype}: {int(ambiguous.sum())} of {P * C} elements have a reference |y| within its bar of 0')
    zero = torch.zeros(C, dtype=torch.float64, device=DEV)
    b = _bwd_bars(x64, r['mean'], r['istd'], r['e_mean'], r['e_istd'], g64, dz, e_dz, e_dz, K, zero, zero, bf16)
    dx = torch.full((P, C), float('nan'), dtype=tdt, device=DEV)
    dgm, dbt = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    _bwd_run(x, P, C, code, stats, gamma, dy, None, 0, y, dgm, dbt, 0, None, dx)
    _report(f'chain {dtype} dx', dx, dx_ref, b['bar_dx'])
    _report(f'chain {dtype} dgamma', dgm, dg_ref, b['bar_dg'])
    _report(f'chain {dtype} dbeta', dbt, db_ref, b['bar_db'])


def test_bn_backward_refuses_bad_arguments():
    from sad import _lib
    P, C = 8, 8
    x = torch.zeros(P, C, device=DEV)
    st = torch.ones(4 * C, device=DEV)
    g = torch.ones(C, device=DEV)
    dx = torch.full((P, C), 1.5, device=DEV)
    dp = torch.zeros(3, C, device=DEV)
    with pytest.raises(RuntimeError, match='exactly one of dy / dpool'):
        _bwd_run(x, P, C, _lib.SAD_F32, st, g, x, dp, 1, None, None, None, 0, None, dx)
    with pytest.raises(RuntimeError, match='pool_hw'):
        _bwd_run(x, P, C, _lib.SAD_F32, st, g, None, dp, 3, None, None, None, 0, None, dx)
    assert (dx == 1.5).all()
