"""GPU: the trainer's loss / optimizer / utility kernels of csrc/train.hip, each
called through its C entry and compared, element for element, with the same
operation in float64 torch on the same input values (hyper-parameters are
rounded to fp32 first, so both sides see the value the C ABI carries).

Every bar is an a-priori rounding bound with u = 2^-24 (one fp32 rounding),
never a measured error; every test prints its worst error / bar ratio.

  sad_ce_loss_run     one wave per row, lane j sums exp over ceil(C/64) logits,
                      then a 6-step butterfly; expf / logf are good to a few u.
                      The lse carries (C/64 + 16) u max(1, |lse|) at most, so
                        out[0] (sum of row losses): sum over rows of
                                (C/64 + 16) u max(1, |lse|, |z_t|)
                                (<= the B (C/64 + 16) u max(...) of the worst row);
                        dlogits: (C/64 + 16) u |scale| absolute (softmax <= 1);
                        out[1] and pred exact (first index of the maximum).
                      B = 0 has no 1/B, so it runs with scale 1 only.
  sad_clip_grad_norm_run  the squares are summed in float64, so the norm is one
                      fp32 rounding of a double: 2^-22 relative (margin 2 over
                      sqrt + cast).  coef and the scaled buffer are fp32
                      expressions of the returned norm: bit for bit.  Non-finite
                      input behaves as torch.nn.utils.clip_grad_norm_: an inf
                      gives coef 0 (inf * 0 = NaN), a NaN gives coef NaN.
                      [The NaN case caught clip_coef_kernel's
                      `coef < 1 ? coef : 1`, which turned a NaN norm into 1.]
  sad_adamw_run       reference: the formula in the kernel's comment in float64
                      (itself checked against torch.optim.AdamW in float64).
                      m = m + (g - m)(1 - b1) and v = v b2 + (1 - b2) g^2 are
                      three roundings each when nothing cancels: 4 u |ref|.
                      (1 - b1, 1 - b2 are exact in fp32.)  So that nothing
                      cancels in m, the state has the sign of the gradient
                      (m0 = g * U[0.5, 1.5]; where g = 0, m0 is arbitrary and
                      m = 0.9 m0 is two roundings).  The update
                      lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps) chains <= 12
                      roundings (bc1 and sqrt(bc2) are rounded to fp32 on the
                      host) and p (1 - lr wd) - update adds 3 u |p| <= 3 u |p_ref|
                      + 3 u |update|: p is held to 4 u |p_ref| + 16 u |update|.
  sad_adamw_pack_run  same arithmetic as sad_adamw_run: p / m / v bit-identical;
                      each packed copy bit-identical to sad_pack_conv_weight_run
                      of the updated p; guard words after each copy untouched.
  sad_axpy_run        y + alpha x: two roundings (or one, contracted to an FMA):
                      2 u (|y| + |alpha x|).
  sad_cast_run        fp32 -> bf16 is round-to-nearest-even, bit-identical to
                      torch's CPU cast (NaN stays NaN, any payload); bf16 ->
                      fp32 is exact.
  sad_avgpool_run     each of 4 waves sums ceil(hw/4) pixels, 3 adds combine
                      them, one division: K = ceil(hw/4) + 4,
                      bar = K u sum|x| / hw.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24


def _f32(v):
    return float(np.float32(v))


def _stream():
    from sad import _lib
    return _lib.stream_handle(torch.device(DEV))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _report(name, err, bar):
    """Worst err / bar over all elements (0/0 counts as 0); asserts err <= bar everywhere."""
    err, bar = err.double().flatten(), bar.double().flatten()
    assert err.numel() == bar.numel()
    if err.numel() == 0:
        print(f'{name}: empty')
        return
    assert torch.isfinite(err).all(), f'{name}: non-finite error'
    ratio = torch.where(err > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    print(f'{name}: worst err {err[i].item():.3e} vs bar {bar[i].item():.3e} (ratio {ratio[i].item():.3f}, '
          f'max err {err.max().item():.3e})')
    assert (err <= bar).all(), f'{name}: err {err[i].item():.3e} > bar {bar[i].item():.3e}'


# ------------------------------------------------------------ cross-entropy --
def _ce_case(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(max(B, 1), C, generator=g) * 2.0
    t = torch.randint(0, C, (max(B, 1),), generator=g)
    # row 0: two equal maxima, the target is the first of them
    j1, j2 = (0, 1) if C == 2 else (C // 3, C - 2)
    z[0, j1] = z[0, j2] = z[0].max() + 1.0
    t[0] = j1
    if B >= 3:
        k = C // 2
        z[1, k] = z[1].max() + 80.0      # one logit 80 above the rest
        t[1] = k if C == 2 else k - 1    # (C = 2: target the large one, the loss is ~0)
        z[2, ::3] = -float('inf')        # -inf entries; index 1 stays finite and is the target
        t[2] = 1
    return z[:B].contiguous(), t[:B].contiguous()


@pytest.mark.parametrize('C', [2, 63, 65, 512, 2048])
@pytest.mark.parametrize('B', [0, 1, 17, 33])
def test_ce_loss_vs_float64(B, C):
    from sad import _lib
    z, t = _ce_case(B, C, B * 4099 + C)
    zd = z.to(DEV) if B else torch.zeros(1, C, device=DEV)
    td = t.to(DEV) if B else torch.zeros(1, dtype=torch.int64, device=DEV)
    z64 = z.double()
    lse = torch.logsumexp(z64, 1)
    zt = z64.gather(1, t[:, None])[:, 0]
    k = C / 64 + 16
    first_max = torch.from_numpy(np.argmax(z.numpy(), axis=1)) if B else torch.zeros(0, dtype=torch.int64)
    for scale in ([1.0, _f32(1.0 / B)] if B else [1.0]):
        for with_pred in (True, False):
            dl = torch.full((max(B, 1), C), 7.5, device=DEV)
            out = torch.full((2,), -3.0, device=DEV)
            pred = torch.full((max(B, 1),), -5, dtype=torch.int32, device=DEV)
            _lib.call('sad_ce_loss_run', _lib.ptr(zd), _lib.ptr(td), B, C, scale, _lib.ptr(dl), _lib.ptr(out),
                      _lib.ptr(pred) if with_pred else None, _stream())
            torch.cuda.synchronize()
            tag = f'ce B{B} C{C} scale {scale:.4g} pred {int(with_pred)}'
            got = out.cpu().double()
            loss_ref = (lse - zt).sum()
            bar = (k * U * torch.maximum(torch.maximum(lse.abs(), zt.abs()), torch.ones_like(lse))).sum()
            _report(f'{tag} loss', (got[0] - loss_ref).abs()[None], bar[None] if B else torch.zeros(1))
            assert got[1].item() == int((first_max == t).sum()), tag
            if B == 0:
                assert torch.equal(dl.cpu(), torch.full((1, C), 7.5)), 'B = 0 wrote dlogits'
                continue
            ref = torch.softmax(z64, 1)
            ref[torch.arange(B), t] -= 1.0
            ref = ref * scale
            _report(f'{tag} dlogits', (dl.cpu().double() - ref).abs(), torch.full_like(ref, k * U * abs(scale)))
            if with_pred:
                assert torch.equal(pred.cpu().long(), first_max), tag
            else:
                assert (pred.cpu() == -5).all(), 'pred = NULL was written'


# ------------------------------------------------------------ clipping --
def _clip(g_dev, n, max_norm=0.5):
    from sad import _lib
    nc = torch.full((2,), -1.0, device=DEV)
    ws = torch.zeros(1024, dtype=torch.float64, device=DEV)
    _lib.call('sad_clip_grad_norm_run', _lib.ptr(g_dev), n, max_norm, _lib.ptr(nc), _lib.ptr(ws), ws.numel() * 8,
              _stream())
    torch.cuda.synchronize()
    return nc.cpu()


@pytest.mark.parametrize('kind', ['above', 'below', 'at'])
@pytest.mark.parametrize('n', [0, 1, 255, 4097, 1024 * 4096 + 3])
def test_clip_grad_norm_vs_float64(n, kind):
    gen = torch.Generator().manual_seed(n % 1000 + len(kind))
    g = torch.randn(max(n, 1), generator=gen)
    if kind == 'below':
        g = (g * (0.1 / g.double().norm().item())).float()
    elif kind == 'at':     # the sum of squares is exactly 0.25
        g.zero_()
        if n >= 4:
            g[[0, n // 3, n // 2, n - 1]] = torch.tensor([0.25, -0.25, 0.25, -0.25])
        else:
            g[0] = -0.5
    elif n == 1:
        g[0] = 0.75        # 'above' with one element
    g = g[:max(n, 1)]
    gd = g.clone().to(DEV)
    nc = _clip(gd, n)
    ref = g[:n].double().norm().item()
    if kind == 'at' and n:
        assert ref == 0.5
    err = abs(nc[0].item() - ref)
    print(f'clip n{n} {kind}: norm {nc[0].item():.8g} ref {ref:.8g} err {err:.3e} bar {2.0 ** -22 * ref:.3e} '
          f'coef {nc[1].item():.8g}')
    assert err <= 2.0 ** -22 * ref
    coef = torch.minimum(torch.tensor(0.5) / (nc[0] + torch.tensor(1e-6)), torch.tensor(1.0))
    assert coef.dtype == torch.float32
    assert torch.equal(_bits(nc[1:2]), _bits(coef[None])), (nc[1].item(), coef.item())
    if kind == 'above' and n:
        assert nc[1].item() < 1.0
    if kind == 'below' or n == 0:
        assert nc[1].item() == 1.0
    want = g * coef
    got = gd.cpu()
    assert torch.equal(_bits(got[:n]), _bits(want[:n])), f'{(got[:n] != want[:n]).sum().item()} elements differ'
    if n == 0:
        assert torch.equal(got, g), 'n = 0 touched the buffer'


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_clip_grad_norm_nonfinite_as_torch(bad):
    n = 4097
    g = torch.randn(n, generator=torch.Generator().manual_seed(11))
    g[1234] = bad
    p = torch.nn.Parameter(torch.zeros(n))
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], 0.5)
    want = p.grad
    gd = g.clone().to(DEV)
    nc = _clip(gd, n)
    got = gd.cpu()
    print(f'clip non-finite {bad}: norm {nc[0].item()} coef {nc[1].item()}; NaN elements {int(got.isnan().sum())} '
          f'(torch {int(want.isnan().sum())})')
    assert torch.equal(got.isnan(), want.isnan())
    ok = ~want.isnan()
    assert torch.equal(got[ok], want[ok])
    if math.isnan(bad):
        assert math.isnan(nc[1].item()) and bool(got.isnan().all())
    else:
        assert nc[1].item() == 0.0 and int(got.isnan().sum()) == 1


# ------------------------------------------------------------ AdamW --
HYPER = dict(lr=_f32(1e-3), b1=_f32(0.9), b2=_f32(0.999), eps=_f32(1e-8))


def _adamw_inputs(n, step, seed):
    gen = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, generator=gen) * 15.0 - 12.0)            # |g| in [1e-12, 1e3]
    g = mag * ((torch.rand(n, generator=gen) < 0.5).float() * 2.0 - 1.0)
    g[3::7] = 0.0                                                         # exact zeros
    if n > 2:
        g[1], g[2] = 1e-12, -1e3
    g = g.float()
    p = torch.randn(n, generator=gen)
    if step == 1:
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        m = g * (0.5 + torch.rand(n, generator=gen))
        v = g * g * (0.5 + torch.rand(n, generator=gen))
        zero = g == 0
        m[zero] = torch.randn(n, generator=gen)[zero] * 1e-3
        v[zero] = torch.rand(n, generator=gen)[zero] * 1e-6
    return p, g, m.float(), v.float()


def _adamw_ref(p, g, m, v, step, wd):
    lr, b1, b2, eps = HYPER['lr'], HYPER['b1'], HYPER['b2'], HYPER['eps']
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    p1 = p * (1.0 - lr * wd)
    m1 = m + (g - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    upd = (lr / bc1) * (m1 / (v1.sqrt() / math.sqrt(bc2) + eps))
    return p1 - upd, m1, v1, upd


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('n', [1, 255, 257, 4099])
def test_adamw_vs_float64(n, step, wd):
    from sad import _lib
    wd = _f32(wd)
    p, g, m, v = _adamw_inputs(n, step, n * 31 + step)
    p_ref, m_ref, v_ref, upd = _adamw_ref(p, g, m, v, step, wd)

    # the formula is the reference's optimizer: torch.optim.AdamW in float64
    q = torch.nn.Parameter(p.double().clone())
    q.grad = g.double().clone()
    opt = torch.optim.AdamW([q], lr=HYPER['lr'], betas=(HYPER['b1'], HYPER['b2']), eps=HYPER['eps'],
                            weight_decay=wd)
    opt.state[q] = {'step': torch.tensor(float(step - 1)), 'exp_avg': m.double().clone(),
                    'exp_avg_sq': v.double().clone()}
    opt.step()
    st = opt.state[q]
    assert st['step'].item() == step
    d64 = 2.0 ** -46
    assert ((q.detach() - p_ref).abs() <= d64 * (p_ref.abs() + upd.abs())).all()
    assert ((st['exp_avg'] - m_ref).abs() <= d64 * m_ref.abs()).all()
    assert ((st['exp_avg_sq'] - v_ref).abs() <= d64 * v_ref.abs()).all()

    pd, gd, md, vd = (t.clone().to(DEV) for t in (p, g, m, v))
    _lib.call('sad_adamw_run', _lib.ptr(pd), _lib.ptr(gd), _lib.ptr(md), _lib.ptr(vd), n, HYPER['lr'], HYPER['b1'],
              HYPER['b2'], HYPER['eps'], wd, step, _stream())
    torch.cuda.synchronize()
    tag = f'adamw n{n} step{step} wd{wd:.3g}'
    _report(f'{tag} m', (md.cpu().double() - m_ref).abs(), 4 * U * m_ref.abs())
    _report(f'{tag} v', (vd.cpu().double() - v_ref).abs(), 4 * U * v_ref.abs())
    _report(f'{tag} p', (pd.cpu().double() - p_ref).abs(), 4 * U * p_ref.abs() + 16 * U * upd.abs())
    assert torch.equal(gd.cpu(), g)


def _pack(w_dev, cout, cin, k, mode, code, tdt):
    from sad import _lib
    out = torch.empty(cout * cin * k * k, dtype=tdt, device=DEV)
    _lib.call('sad_pack_conv_weight_run', _lib.ptr(w_dev), cout, cin, k, mode, code, _lib.ptr(out), _stream())
    return out


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_adamw_pack_matches_adamw_then_pack(dtype):
    from sad import _lib
    code, tdt = (_lib.SAD_BF16, torch.bfloat16) if dtype == 'bf16' else (_lib.SAD_F32, torch.float32)
    na, nb = 16 * 24 * 9, 8 * 16
    off_b = na + 40
    n = off_b + nb
    step, wd = 3, _f32(0.01)
    p, g, m, v = _adamw_inputs(n, step, 77)
    args = (HYPER['lr'], HYPER['b1'], HYPER['b2'], HYPER['eps'], wd, step)
    ref = [t.clone().to(DEV) for t in (p, g, m, v)]
    _lib.call('sad_adamw_run', *[_lib.ptr(t) for t in ref], n, *args, _stream())
    got = [t.clone().to(DEV) for t in (p, g, m, v)]
    GUARD = 8
    sentinel = 1.5
    bufs = [torch.full((cnt + GUARD,), sentinel, dtype=tdt, device=DEV) for cnt in (na, na, nb)]
    segs = (_lib.PackSeg * 2)(_lib.PackSeg(0, 16, 24, 3, 0, _lib.ptr(bufs[0]), _lib.ptr(bufs[1])),
                              _lib.PackSeg(off_b, 8, 16, 1, 0, _lib.ptr(bufs[2]), None))
    _lib.call('sad_adamw_pack_run', *[_lib.ptr(t) for t in got], n, *args, segs, 2, code, _stream())
    torch.cuda.synchronize()
    for name, a, b in zip('pgmv', got, ref):
        assert torch.equal(_bits(a.cpu()), _bits(b.cpu())), f'{name} differs from sad_adamw_run'
    assert not torch.equal(ref[0].cpu(), p)
    pu = ref[0]
    want = [_pack(pu, 16, 24, 3, 0, code, tdt), _pack(pu, 16, 24, 3, 1, code, tdt),
            _pack(pu[off_b:], 8, 16, 1, 0, code, tdt)]
    torch.cuda.synchronize()
    for i, (b, w) in enumerate(zip(bufs, want)):
        cnt = w.numel()
        assert torch.equal(_bits(b[:cnt].cpu()), _bits(w.cpu())), f'pack buffer {i} ({dtype})'
        assert (b[cnt:].cpu().float() == sentinel).all(), f'guard words after pack buffer {i} were written'
    print(f'adamw_pack {dtype}: p/m/v and 3 packed copies bit-identical, guards intact')

    # argument checks: more than 16 segments; a segment reaching past n
    many = (_lib.PackSeg * 17)(*[_lib.PackSeg(0, 1, 1, 1, 0, None, None) for _ in range(17)])
    with pytest.raises(RuntimeError, match='16 pack segments'):
        _lib.call('sad_adamw_pack_run', *[_lib.ptr(t) for t in got], n, *args, many, 17, code, _stream())
    past = (_lib.PackSeg * 1)(_lib.PackSeg(off_b + 1, 8, 16, 1, 0, _lib.ptr(bufs[2]), None))
    with pytest.raises(RuntimeError, match='outside the parameter range'):
        _lib.call('sad_adamw_pack_run', *[_lib.ptr(t) for t in got], n, *args, past, 1, code, _stream())
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        assert torch.equal(_bits(a.cpu()), _bits(b.cpu())), 'a refused call changed the buffers'


# ------------------------------------------------------------ axpy --
@pytest.mark.parametrize('alpha', [1.0, -0.5])
@pytest.mark.parametrize('n', [0, 1, 255, 257])
def test_axpy_vs_float64(n, alpha):
    from sad import _lib
    gen = torch.Generator().manual_seed(n + 3)
    m = max(n, 1) + 4                       # 4 trailing elements no call may touch
    x, y = torch.randn(m, generator=gen) * 3.0, torch.randn(m, generator=gen)
    xd, yd = x.to(DEV), y.clone().to(DEV)
    _lib.call('sad_axpy_run', _lib.ptr(yd), _lib.ptr(xd), n, alpha, _stream())
    torch.cuda.synchronize()
    got = yd.cpu()
    ref = y[:n].double() + alpha * x[:n].double()
    _report(f'axpy n{n} alpha {alpha}', (got[:n].double() - ref).abs(),
            2 * U * (y[:n].double().abs() + (alpha * x[:n].double()).abs()))
    assert torch.equal(got[n:], y[n:]), 'axpy wrote past n'


# ------------------------------------------------------------ cast --
_SPECIAL_BITS = [
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,    # ties: to even downwards / upwards, both signs
    0x3F808001, 0x3F817FFF,                            # just above / just below a tie
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,    # +-0, +-inf
    0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x00400000,   # denormals (two of them ties)
    0x7F7FFFFF, 0xFF7FFFFF,                            # largest finite: rounds to +-inf
    0x7FC00000, 0x7F800001, 0xFFC12345,                # NaNs: quiet, signalling with a low payload, negative
    0x7F7F7FFF, 0x7F7F8000,                            # below / at the tie under the largest bf16
]


def _special_f32():
    return torch.from_numpy(np.array(_SPECIAL_BITS, dtype=np.uint32).view(np.float32).copy())


def _same_bits_or_nan(got, want):
    nan = want.float().isnan()
    assert torch.equal(got.float().isnan(), nan), 'NaN positions differ'
    gb, wb = _bits(got), _bits(want)
    assert torch.equal(gb[~nan], wb[~nan]), \
        f'bits differ at {torch.nonzero((gb != wb) & ~nan).flatten()[:8].tolist()}'


@pytest.mark.parametrize('n', [1, 7, 8, 9, 2047, 2049])
def test_cast_bit_exact(n):
    from sad import _lib
    S = _special_f32()
    ns = S.numel()
    gen = torch.Generator().manual_seed(n)
    rots = range(0, ns, n) if n < ns else [0]
    for rot in rots:
        src = torch.randn(n, generator=gen) * 10.0 ** torch.randint(-30, 30, (n,), generator=gen).float()
        k = min(n, ns)
        src[:k] = S[(torch.arange(k) + rot) % ns]
        if n >= 2 * ns:
            src[n - ns:] = S.flip(0)       # the specials also pass through the scalar tail (n % 8 != 0)
        # fp32 -> bf16
        sd = src.to(DEV)
        dst = torch.full((n + 8,), 1.5, dtype=torch.bfloat16, device=DEV)
        _lib.call('sad_cast_run', _lib.ptr(sd), _lib.SAD_F32, _lib.ptr(dst), _lib.SAD_BF16, n, _stream())
        torch.cuda.synchronize()
        want = src.to(torch.bfloat16)
        _same_bits_or_nan(dst[:n].cpu(), want)
        assert (dst[n:].cpu().float() == 1.5).all(), 'fp32->bf16 wrote past n'
        # bf16 -> fp32 (exact), from the rounded values and from raw bit patterns
        for hb in (want, torch.randint(-32768, 32768, (n,), generator=gen, dtype=torch.int16).view(torch.bfloat16)):
            hd = hb.to(DEV)
            back = torch.full((n + 8,), 1.5, device=DEV)
            _lib.call('sad_cast_run', _lib.ptr(hd), _lib.SAD_BF16, _lib.ptr(back), _lib.SAD_F32, n, _stream())
            torch.cuda.synchronize()
            _same_bits_or_nan(back[:n].cpu(), hb.float())
            assert (back[n:].cpu() == 1.5).all(), 'bf16->fp32 wrote past n'
    if n >= ns:
        w = S.to(torch.bfloat16)
        assert w[15].item() == float('inf') and w[16].item() == -float('inf') and bool(w[17:20].isnan().all())
    print(f'cast n{n}: {len(list(rots))} pass(es) bit-identical both ways')


def test_cast_refuses_misaligned_destination():
    from sad import _lib
    src = torch.zeros(16, dtype=torch.bfloat16, device=DEV)
    dst = torch.full((24,), 1.5, device=DEV)
    assert dst.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError, match='16-B aligned'):
        _lib.call('sad_cast_run', _lib.ptr(src), _lib.SAD_BF16, _lib.ptr(dst[1:]), _lib.SAD_F32, 16, _stream())
    torch.cuda.synchronize()
    assert (dst.cpu() == 1.5).all()


# ------------------------------------------------------------ average pool --
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
@pytest.mark.parametrize('C', [64, 192])
@pytest.mark.parametrize('hw', [1, 3, 49, 256])
@pytest.mark.parametrize('B', [0, 1, 3])
def test_avgpool_vs_float64(B, hw, C, dtype):
    from sad import _lib
    code, tdt = (_lib.SAD_BF16, torch.bfloat16) if dtype == 'bf16' else (_lib.SAD_F32, torch.float32)
    gen = torch.Generator().manual_seed(B * 1000 + hw + C)
    x = (torch.randn(max(B, 1), hw, C, generator=gen) + torch.randn(C, generator=gen)).to(tdt)
    xd = x.to(DEV)
    out = torch.full((max(B, 1) + 1, C), -7.0, device=DEV)
    _lib.call('sad_avgpool_run', _lib.ptr(xd), B, hw, C, code, _lib.ptr(out), _stream())
    torch.cuda.synchronize()
    got = out.cpu()
    assert (got[B:] == -7.0).all(), 'avgpool wrote past B rows'
    x64 = x[:B].double()
    K = math.ceil(hw / 4) + 4
    _report(f'avgpool {dtype} B{B} hw{hw} C{C}', (got[:B].double() - x64.mean(1)).abs(),
            K * U * x64.abs().sum(1) / hw)


def test_avgpool_refuses_channels_not_multiple_of_64():
    from sad import _lib
    x = torch.zeros(4, 32, device=DEV)
    out = torch.zeros(32, device=DEV)
    with pytest.raises(RuntimeError, match='multiple of 64'):
        _lib.call('sad_avgpool_run', _lib.ptr(x), 1, 4, 32, _lib.SAD_F32, _lib.ptr(out), _stream())
