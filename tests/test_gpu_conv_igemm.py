"""GPU: conv_igemm_kernel (csrc/conv.hip) through sad_conv2d_run, every tile
variant (1..8 and 0 = the default choice) in fp32 and bf16, element for
element against a float64 convolution of the exact operands (+ bias + residual,
ReLU) under a-priori bars:

  fp32   (K + 8) u (conv(|x|, |w|) + |bias| + |res|),  K = k k Cin, u = 2^-24
  bf16   the same (fp32 accumulation of exact bf16 products) + 2^-8 |ref| for
         the one output rounding
  ReLU   where the float64 pre-activation is <= -(accumulation bar) the
         output must be exactly 0

The heads' two wide layers and sad_conv2d_run stand on this kernel.  Shapes
are the smallest that reach each edge: 1, 2 and 3 K-steps (the three-stage variants' ring start-up), M below one tile, M one
past a multiple of every BM (128, 256, 512), H != W with odd sizes at 3x3
stride 1 and 2, 1x1 stride 2, 7x7 stride 2 pad 3, with and without residual
and ReLU, N = 0.  The image's border pixels carry large values, so that a
padding mistake is far above the bar.

A bf16 ratio close to 1 is the output rounding alone: bf16 keeps 8 significant
bits, so round-to-nearest errs by up to 2^-8 |v| just above a power of two (a
CPU fp32 convolution rounded to bf16 gives the same 0.75 .. 0.99); the
accumulation part of the error is what the fp32 cases show, below 0.1.

All variants of one dtype walk K in the same order (K-step by K-step, the same
chunk order inside a step, whatever the tile shape and ring depth), so their
outputs are also asserted equal bit for bit.
"""
import pytest
import torch
import torch.nn.functional as F

import heads_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
BF = 2.0 ** -8
GUARD = 4096
FILL = 0xFF
VARIANTS = [0, 1, 2, 3, 4, 5, 6, 7, 8]
WIDE = (3, 4, 5, 8)              # 128-wide tiles: Cout % 128 == 0 (1, 2, 6, 7: 64-wide)
BM = {1: 256, 2: 256, 3: 256, 4: 128, 5: 128, 6: 512, 7: 128, 8: 256}
KSTEP = {'fp32': 32, 'bf16': 64}  # input channels per K-step (128 bytes)

# name -> (N, H, W, Cin in K-steps (or channels: 'c32'), Cout, k, stride, pad, residual, relu)
SHAPES = {
    '1x1 nk1 M15': (1, 3, 5, 1, 128, 1, 1, 0, False, True),
    '1x1 nk2 M15': (1, 3, 5, 2, 128, 1, 1, 0, True, True),
    '1x1 nk3 M15': (1, 3, 5, 3, 128, 1, 1, 0, False, False),
    '1x1 M129': (129, 1, 1, 1, 128, 1, 1, 0, True, False),
    '1x1 M257': (1, 1, 257, 2, 128, 1, 1, 0, False, True),
    '1x1 M513': (27, 19, 1, 1, 128, 1, 1, 0, True, True),
    '3x3 s1 p1 5x9': (2, 5, 9, 1, 128, 3, 1, 1, True, True),
    '3x3 s2 p1 5x9': (3, 5, 9, 1, 128, 3, 2, 1, False, False),
    '3x3 s2 p1 9x5 res': (2, 9, 5, 2, 128, 3, 2, 1, True, True),
    '1x1 s2 p0 5x9': (2, 5, 9, 2, 128, 1, 2, 0, False, True),
    '7x7 s2 p3 9x11': (1, 9, 11, 'c32', 128, 7, 2, 3, False, True),
    '3x3 s1 p1 Cout64': (2, 5, 9, 1, 64, 3, 1, 1, True, True),
    '3x3 s1 p1 Cout192': (1, 7, 6, 1, 192, 3, 1, 1, False, True),
}


def _tensors(dtype, name):
    """Seeded operands (CPU, in the kernel's dtype): a quiet image with large
    border pixels, weights, bias, residual or None."""
    N, H, W, cin, Cout, k, s, p, res, relu = SHAPES[name]
    Cin = 32 if cin == 'c32' else cin * KSTEP[dtype]
    if cin == 'c32' and dtype == 'bf16':
        Cin = 64                                   # (32 bf16 channels are half a K-step: refused, see below)
    gen = torch.Generator().manual_seed(sum(map(ord, dtype + name)))
    td = torch.float32 if dtype == 'fp32' else torch.bfloat16
    x = torch.randn(N, H, W, Cin, generator=gen) * 0.5
    big = torch.randn(N, H, W, Cin, generator=gen) * 8.0
    x[:, [0, H - 1]] = big[:, [0, H - 1]]
    x[:, :, [0, W - 1]] = big[:, :, [0, W - 1]]
    w = torch.randn(Cout, k, k, Cin, generator=gen) * (2.0 / (k * k * Cin)) ** 0.5
    b = torch.randn(Cout, generator=gen)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    r = torch.randn(N, Ho, Wo, Cout, generator=gen).to(td) if res else None
    return x.to(td), w.to(td), b, r, (s, p, relu)


def _reference(dtype, x, w, b, r, s, p, relu):
    """-> (ref, bar, must_be_zero), NHWC float64."""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    z = F.conv2d(xd, wd, b.double(), s, p).permute(0, 2, 3, 1)
    S = F.conv2d(xd.abs(), wd.abs(), b.double().abs(), s, p).permute(0, 2, 3, 1)
    if r is not None:
        z, S = z + r.double(), S + r.double().abs()
    acc = (K + 8) * U * S
    ref = z.clamp_min(0) if relu else z
    bar = acc + (BF * ref.abs() if dtype == 'bf16' else 0.0)
    return ref, bar, (z <= -acc) if relu else None


def _run(x, w, b, r, s, p, relu, variant):
    """conv2d into a guarded buffer -> (out on the CPU, guards intact)."""
    from sad.engine import conv2d
    N, H, W, _ = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    nbytes = N * Ho * Wo * Cout * x.element_size()
    raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = raw[GUARD:GUARD + nbytes].view(x.dtype).view(N, Ho, Wo, Cout)
    conv2d(x, w, b, s, p, r, relu, variant, out=out)
    torch.cuda.synchronize()
    ok = bool((raw[:GUARD] == FILL).all() and (raw[GUARD + nbytes:] == FILL).all())
    return out.cpu(), ok, raw


@pytest.mark.parametrize('name', list(SHAPES))
@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_every_variant_against_float64(dtype, name):
    x, w, b, r, (s, p, relu) = _tensors(dtype, name)
    ref, bar, zero = _reference(dtype, x, w, b, r, s, p, relu)
    assert ref.numel() > 0 and (not relu or ((ref == 0).any() and (ref > 0).any()))
    dx, dw, db, dr = x.to(DEV), w.to(DEV), b.to(DEV), None if r is None else r.to(DEV)
    Cout = w.shape[0]
    outs, ratios = {}, {}
    for v in VARIANTS:
        if v in WIDE and Cout % 128:
            with pytest.raises(RuntimeError, match='tile width'):
                _run(dx, dw, db, dr, s, p, relu, v)
            continue
        out, ok, _ = _run(dx, dw, db, dr, s, p, relu, v)
        assert ok, (v, 'guard bytes behind out')
        ratios[v] = R.worst_ratio(out, ref, bar, zero)
        outs[v] = out
    print(f'RATIO conv {dtype} {name}: ' + ', '.join(f'v{v} {q:.3g}' for v, q in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    bits = torch.int32 if dtype == 'fp32' else torch.int16
    for v, out in outs.items():
        assert torch.equal(out.view(bits), outs[0].view(bits)), f'variant {v} differs from the default in some bit'


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_refusals_leave_out_untouched(dtype):
    """Cout = 64 on a 128-wide variant; half a K-step of input channels."""
    x, w, b, r, (s, p, relu) = _tensors(dtype, '3x3 s1 p1 Cout64')
    dx, dw, db, dr = x.to(DEV), w.to(DEV), b.to(DEV), r.to(DEV)
    from sad.engine import conv2d
    for v in WIDE:
        out = torch.full((2, 5, 9, 64), 7.0, dtype=x.dtype, device=DEV)
        with pytest.raises(RuntimeError, match='tile width'):
            conv2d(dx, dw, db, s, p, dr, relu, v, out=out)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all())
    half = KSTEP[dtype] // 2
    out = torch.full((2, 5, 9, 64), 7.0, dtype=x.dtype, device=DEV)
    with pytest.raises(RuntimeError, match='K-step'):
        conv2d(dx[..., :half].contiguous(), dw[..., :half].contiguous(), db, s, p, dr, relu, 0, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_empty_batch_writes_nothing(dtype):
    """N = 0 with valid pointers: accepted, and nothing is written."""
    from sad import _lib
    x, w, b, _, (s, p, relu) = _tensors(dtype, '3x3 s1 p1 5x9')
    dx, dw, db = x.to(DEV), w.to(DEV), b.to(DEV)
    out = torch.full((GUARD,), FILL, dtype=torch.uint8, device=DEV)
    for v in VARIANTS:
        with torch.cuda.device(DEV):
            _lib.call('sad_conv2d_run', dx.data_ptr(), 0, 5, 9, x.shape[3], dw.data_ptr(), db.data_ptr(), None,
                      out.data_ptr(), 128, 3, s, p, int(relu), _lib.DTYPES[dtype], v,
                      _lib.stream_handle(torch.device(DEV)))
        torch.cuda.synchronize()
        assert bool((out == FILL).all())
