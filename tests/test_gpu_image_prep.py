"""GPU: the tail of the trainer's front end, per kernel against float64 torch:
sad_specaug_norm_run (specaug_norm_kernel, csrc/train.hip), sad_resize_run
(resize_kernel, csrc/frontend.hip) and sad_crop_resize_run (crop_resize_kernel,
csrc/train.hip), at tiny shapes, at counts that are no multiple of the
workgroup, with masks and boxes on the edges, and past one launch chunk.

Every bar is an a-priori rounding bound from the float64 reference and the
data, u = 2^-24 (one fp32 rounding); none is a measured error.

specaug_norm.  v = the dB value, or 0.0 under a mask.  The kernel sums v and
(v - mean)^2 in float64 (error n 2^-53 relative: it does not count, and is
added all the same), then computes in fp32
  mean_f = (float) mean                        u |mean|
  den_f  = (float) sqrt(var) + 1e-6f           3 u den   (cast, add, the constant)
  y      = (v - mean_f) / den_f                u |v - mean| for the subtraction, 2 u |y| for the division
so  dy = (u |mean| + u |v - mean| + e64) / den + |y| (3 u + e64) + 2 u |y|,
all times (1 + 8 u) for the second-order terms.  A map masked whole is exactly 0
(0 / 1e-6).

resize (bilinear, align_corners=False).  The source coordinate
f = sc (o + 0.5) - 0.5 with sc = (float) in / out is computed in fp32: sc rounds
once, the product once (not at all when contracted into an FMA), the
subtraction once, so |df| <= 3 u (f + 1) for the float64 f >= 0 (the clamp at 0
is 1-Lipschitz).  These three roundings follow from the shapes alone, so _axis
evaluates them (both contractions) instead of taking the worst case: df is 0
where the scale and the products are exact (128 -> 512, 512 -> 512), which
leaves such a pixel the lerp roundings only.  f - floor(f) is exact.  The
interpolant is continuous and piecewise linear in f, its slope along an axis at
most the spread D = max - min of the source over the 4 x 4 neighbourhood of
(floor fy, floor fx) (rows / columns -1 .. +2, clamped: also right when the
fp32 floor lands one cell off), so the coordinate errors move a pixel by at
most (dfy + dfx) D.  1 - l rounds once, and the two lerp levels round three
times each on values <= A = max |source| over the neighbourhood: 8 u A.
  bar = (dfy + dfx) D + 8 u A  (+ the largest bar of the neighbourhood's source
  pixels, when the source is itself a computed image: crop_resize's second stage).
The bf16 image is the fp32 image rounded to nearest-even, bit for bit.

crop_resize.  Resize((512, 512)) then resized_crop(i, j, h, w) back to 512:
the reference composes two float64 F.interpolate calls as oracle.train.segment_image
does (antialias=True: for upsampling the plain bilinear filter); the bar is the
resize bar through both stages.  All cases upsample (map sides <= 512, box sides
<= 512 = out_hw), which is all the entry implements (include/sad.h)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
E64 = 2.0 ** -53
R = 512


def _stream():
    from sad import _lib
    return _lib.stream_handle(torch.device(DEV))


def report(name, got, ref, bar, note=''):
    """One record row; asserts err <= bar everywhere."""
    err = (got.double() - ref).abs().flatten()
    bar = bar.double().expand_as(ref).flatten()
    assert err.numel() == bar.numel() and err.numel() > 0
    assert torch.isfinite(got).all() and torch.isfinite(err).all(), f'{name}: non-finite'
    ratio = torch.where(err > 0, err / bar.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    print(f'R08 | {name} | {err.numel()} | {err[i].item():.3e} | {bar[i].item():.3e} | {ratio[i].item():.3f} | '
          f'max err {err.max().item():.3e} | {note}')
    assert (err <= bar).all(), f'{name}: err {err[i].item():.3e} > bar {bar[i].item():.3e}'


# ------------------------------------------------------------ specaug_norm --
def _specaug_ref(x, masks):
    """x [n, M, Fr] fp32 (CPU), masks [n, 4] int or None -> float64 map and bar."""
    n, M, Fr = x.shape
    v = x.double().clone()
    if masks is not None:
        m = torch.arange(M)[None, :, None]
        t = torch.arange(Fr)[None, None, :]
        mk = masks.long()
        hit = ((m >= mk[:, 0, None, None]) & (m < mk[:, 1, None, None])) | \
              ((t >= mk[:, 2, None, None]) & (t < mk[:, 3, None, None]))
        v[hit] = 0.0                                     # fill 0.0
    cnt = M * Fr
    mean = v.mean((1, 2), keepdim=True)
    std = v.std((1, 2), keepdim=True)                    # unbiased
    den = std + 1e-6
    y = (v - mean) / den
    e64 = cnt * E64 * v.abs().mean((1, 2), keepdim=True)
    bar = ((U * mean.abs() + U * (v - mean).abs() + e64) / den + y.abs() * (3.0 * U + 4.0 * cnt * E64) +
           2.0 * U * y.abs()) * (1.0 + 8.0 * U)
    return y, bar


def _specaug_run(x, masks):
    from sad import _lib
    n, M, Fr = x.shape
    xd = x.to(DEV).contiguous()
    md = None if masks is None else masks.to(device=DEV, dtype=torch.int32).contiguous()
    out = torch.full_like(xd, float('nan'))
    _lib.call('sad_specaug_norm_run', _lib.ptr(xd), n, M, Fr, _lib.ptr(md), _lib.ptr(out), _stream())
    torch.cuda.synchronize()
    return out.cpu()


def _db_like(n, M, Fr, seed):
    """dB-like values: around -40 with 15 dB of spread, floored as a clamp would."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, M, Fr, generator=g) * 15.0 - 40.0).clamp_min(-72.5)


def _mask_sets(M, Fr):
    """name -> {f0, f1, t0, t1} for an M x Fr map (a 1-wide axis can only be masked whole)."""
    fa, fb = (M // 3, max(M // 3 + 1, (2 * M) // 3)) if M > 1 else (0, 0)
    ta, tb = (Fr // 4, max(Fr // 4 + 1, Fr // 2)) if Fr > 1 else (0, 0)
    return {
        'f0 == f1': (M // 2, M // 2, Fr // 2, Fr // 2),
        'both edges': (max(M - 2, 0) if M > 1 else 0, M if M > 1 else 0, 0, max(1, Fr // 5) if Fr > 1 else 0),
        'overlapping': (fa, fb, ta, tb),
        'frequency only': (0, max(1, M // 4) if M > 1 else 0, 0, 0),
        'whole map': (0, M, 0, 0),
        'whole map by time': (0, 0, 0, Fr),
    }


@pytest.mark.parametrize('M,Fr', [(128, 251), (3, 5), (1, 2), (7, 1031)])
def test_specaug_norm_vs_float64(M, Fr):
    sets = _mask_sets(M, Fr)
    n = len(sets)
    x = _db_like(n, M, Fr, 5 + M)
    masks = torch.tensor(list(sets.values()), dtype=torch.int32)
    got = _specaug_run(x, masks)
    ref, bar = _specaug_ref(x, masks)
    note = f'{M}x{Fr}, count {M * Fr} ({"a multiple" if (M * Fr) % 1024 == 0 else "no multiple"} of 1024)'
    report(f'specaug_norm masks {M}x{Fr}', got, ref, bar, note)
    for i, name in enumerate(sets):
        if name.startswith('whole map'):
            assert torch.equal(got[i], torch.zeros(M, Fr)), name
            assert torch.equal(ref[i], torch.zeros(M, Fr).double())
    # f0 == f1 and NULL masks: no mask at all, the same bits
    got0 = _specaug_run(x, None)
    ref0, bar0 = _specaug_ref(x, None)
    report(f'specaug_norm NULL masks {M}x{Fr}', got0, ref0, bar0, note)
    assert torch.equal(got0[0], got[0])


def test_specaug_norm_second_launch_has_its_own_masks():
    """65,537 maps of 3 x 5: two launches (65,535 + 2); map 65,536 is the only one
    with a mask, read at masks + i * 4 of the second launch."""
    n, M, Fr = 65537, 3, 5
    x = _db_like(n, M, Fr, 9)
    masks = torch.zeros(n, 4, dtype=torch.int32)
    masks[65536] = torch.tensor([1, 2, 0, 3])
    got = _specaug_run(x, masks)
    ref, bar = _specaug_ref(x, masks)
    assert float(ref[65536].std()) > 0 and not torch.equal(ref[65536], _specaug_ref(x[65536:], None)[0][0])
    report('specaug_norm 65537 maps of 3x5', got, ref, bar, 'two launches, the mask on map 65536')
    report('specaug_norm map 65536', got[65536:], ref[65536:], bar[65536:], 'second launch, masks + i * 4')


# ------------------------------------------------------------------ resize --
def _axis(in_n, out_n):
    """float64 source coordinate (clamped at 0), its floor and the fp32 coordinate's error bound."""
    o = torch.arange(out_n, dtype=torch.float64)
    f = ((in_n / out_n) * (o + 0.5) - 0.5).clamp_min(0.0)
    i0 = f.floor().long().clamp_max(in_n - 1)
    # the fp32 coordinate, from the shapes alone: sc = (float) in / out is one correctly
    # rounded division; sc (o + 0.5) is exact in float64 (24 x 11 bits) and is rounded before
    # the subtraction or, contracted into an FMA, not at all -- the bound covers both
    sc = np.float64(np.float32(in_n) / np.float32(out_n))
    prod = sc * (o.numpy() + 0.5)
    fa = np.float32(np.float32(prod) - np.float32(0.5)).astype(np.float64)
    fb = np.float32(prod - 0.5).astype(np.float64)
    df = np.maximum(np.abs(np.maximum(fa, 0.0) - f.numpy()), np.abs(np.maximum(fb, 0.0) - f.numpy()))
    assert (df <= 3.0 * U * (f.numpy() + 1.0)).all()          # never more than three roundings
    return f, i0, torch.from_numpy(df)


def _neigh(t, op):
    """max (op = 1) or min (-1) of t [n, h, w] over rows / columns -1 .. +2, clamped at the borders."""
    p = F.pad((op * t)[:, None], (1, 2, 1, 2), mode='replicate')
    return op * F.max_pool2d(p, kernel_size=4, stride=1)[:, 0]


def _resize_ref(src, oh, ow, src_bar=None, antialias=False):
    """src [n, h, w] float64 -> float64 bilinear resize and the module docstring's bar."""
    n, h, w = src.shape
    ref = F.interpolate(src[:, None], size=(oh, ow), mode='bilinear', align_corners=False, antialias=antialias)[:, 0]
    _, y0, dfy = _axis(h, oh)
    _, x0, dfx = _axis(w, ow)

    def at(t):
        return t[:, y0][:, :, x0]
    D = at(_neigh(src, 1)) - at(_neigh(src, -1))
    A = at(_neigh(src.abs(), 1))
    bar = (dfy[:, None] + dfx[None, :])[None] * D + 8.0 * U * A
    if src_bar is not None:
        bar = bar + at(_neigh(src_bar, 1)) * (1.0 + 8.0 * U)
    return ref, bar


def _resize_run(src, oh, ow, dtype):
    from sad import _lib
    n, h, w = src.shape
    s = src.to(DEV).contiguous()
    bf = dtype == 'bf16'
    out = torch.zeros(n, oh, ow, device=DEV, dtype=torch.bfloat16 if bf else torch.float32)
    _lib.call('sad_resize_run', _lib.ptr(s), n, h, w, oh, ow, _lib.SAD_BF16 if bf else _lib.SAD_F32, _lib.ptr(out),
              _stream())
    torch.cuda.synchronize()
    return out.cpu()


def _maps(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, h, w, generator=g) * 1.5


@pytest.mark.parametrize('h,w,oh,ow', [(128, 251, 512, 512), (1, 1, 4, 4), (2, 3, 5, 7), (6, 6, 6, 6)])
def test_resize_vs_float64(h, w, oh, ow):
    src = _maps(3, h, w, 31 + h)
    got = _resize_run(src, oh, ow, 'fp32')
    ref, bar = _resize_ref(src.double(), oh, ow)
    report(f'resize {h}x{w} -> {oh}x{ow} fp32', got, ref, bar)
    if (h, w) == (oh, ow):
        assert torch.equal(got, src)                         # scale 1: a bit-exact copy
    if (h, w) == (1, 1):                                     # constant: the lerps' roundings alone
        assert torch.equal(bar, 8.0 * U * src.double().abs().expand(3, oh, ow))
    got16 = _resize_run(src, oh, ow, 'bf16')
    assert torch.equal(got16, got.to(torch.bfloat16))        # round to nearest even of the fp32 image


# ------------------------------------------------------------- crop_resize --
def _crop_run(maps, boxes, dtype):
    from sad import _lib
    n, h, w = maps.shape
    s = maps.to(DEV).contiguous()
    b = None if boxes is None else torch.tensor(boxes, dtype=torch.int32, device=DEV).contiguous()
    bf = dtype == 'bf16'
    out = torch.zeros(n, R, R, device=DEV, dtype=torch.bfloat16 if bf else torch.float32)
    _lib.call('sad_crop_resize_run', _lib.ptr(s), n, h, w, _lib.ptr(b), R, _lib.SAD_BF16 if bf else _lib.SAD_F32,
              _lib.ptr(out), _stream())
    torch.cuda.synchronize()
    return out.cpu()


def _boxes():
    from sad import augment
    g = torch.Generator().manual_seed(4)
    drawn = [augment.random_resized_crop_params(generator=g) for _ in range(3)]
    named = {
        'full': (0, 0, R, R),
        'corner top-left': (0, 0, 300, 350),
        'corner j + w = 512': (0, R - 350, 300, 350),
        'corner i + h = 512': (R - 300, 0, 300, 350),
        'corner both': (R - 300, R - 350, 300, 350),
        'one pixel': (200, 300, 1, 1),
        'full height': (0, 0, R, 343),
        'full width': (0, 0, 343, R),
    }
    for k, b in enumerate(drawn):
        named[f'drawn {k}'] = tuple(int(v) for v in b)
    for i, j, h, w in named.values():
        assert 0 <= i and 0 <= j and 1 <= h and 1 <= w and i + h <= R and j + w <= R
    return named


@pytest.mark.parametrize('h,w', [(128, 251), (2, 3), (1, 1), (512, 512)])
def test_crop_resize_vs_float64(h, w):
    boxes = _boxes()
    n = len(boxes)
    maps = _maps(n, h, w, 57 + h)
    got = _crop_run(maps, list(boxes.values()), 'fp32')
    img, img_bar = _resize_ref(maps.double(), R, R, antialias=True)       # Resize((512, 512))
    for k, (name, (i, j, bh, bw)) in enumerate(boxes.items()):
        ref, bar = _resize_ref(img[k:k + 1, i:i + bh, j:j + bw], R, R, src_bar=img_bar[k:k + 1, i:i + bh, j:j + bw],
                               antialias=True)
        report(f'crop_resize {h}x{w} box {name}', got[k:k + 1], ref, bar, f'box {(i, j, bh, bw)}')
        if name == 'one pixel':   # a constant image: D = 0, so the bar is the lerps' roundings alone
            assert float(ref.max() - ref.min()) <= 1e-14 * float(ref.abs().max())
            assert float(bar.max()) <= 8.0 * U * float(ref.abs().max()) + float(img_bar[k, i, j]) * (1.0 + 1e-6)
    got16 = _crop_run(maps, list(boxes.values()), 'bf16')
    assert torch.equal(got16, got.to(torch.bfloat16))
    # NULL boxes, the full box and sad_resize_run(.., 512, 512): the same bits
    for dt in ('fp32', 'bf16'):
        a = _crop_run(maps[:2], None, dt)
        b = _crop_run(maps[:2], [(0, 0, R, R)] * 2, dt)
        c = _resize_run(maps[:2], R, R, dt)
        assert torch.equal(a, b), dt
        assert torch.equal(a, c), dt
