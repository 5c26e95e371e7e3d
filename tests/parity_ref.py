"""Float64 contracts of the two parity modes' block convs, fp32 and split-bf16
('bf16x3'), with their a-priori per-element bars and the case tables of the GPU
tests (no GPU work here; tests/test_parity_reference.py checks this file on the
CPU, tests/test_gpu_block_fp32.py and tests/test_gpu_x3_kernels.py compare the
kernels with it).

fp32 contract.  out = relu?(conv(x, w) [+ 1x1/sc_stride(sc) as K columns] + bias
[+ res]), every operand fp32, accumulated in fp32 in any order.  Bar per
element, u = 2^-24, K = taps x Cin + Cin1:

    |out - ref| <= (K + 8) u S,   S = conv(|x|, |w|) [+ |sc| |w1|] + |bias| [+ |res|]

It holds for any summation order of an fp32 FMA chain of K products plus the
bias and the residual (tests/test_gpu_conv_igemm.py's bar).  ReLU is
1-Lipschitz: the bar is unchanged, and where the float64 pre-activation is
<= -bar the output must be exactly 0.

split-bf16 contract (csrc/block.hip, the X3 comment and the register epilogue).
Every tensor stores a logical value v as hi = bf16(v), lo = bf16(v - hi), both
round-to-nearest-even; the operands of a launch are those stored halves.
  three products:  z = W_hi.X_hi + W_lo.X_hi + W_hi.X_lo over the taps and, in the
                   same form, over the shortcut's K columns, + bias + res_hi + res_lo
  four products:   the same + W_lo.X_lo                       (four=True)
accumulated in fp32 in any order; v = relu?(z) is stored as hi = bf16(v),
lo = bf16(v - hi).  Bar per element, P = 3 or 4 products:

    |hi + lo - ref| <= A + 2^-16 (|ref| + A),   A = (P K + 8) u S3

  * A: the fp32 accumulation of P K exact bf16 x bf16 products (8 + 8 significant
    bits: exact in fp32), the bias and the two residual halves, in any order; S3
    is the same sum on absolute values -- the P product convs of |.| halves,
    |bias|, |res_hi| + |res_lo|.
  * the device's fp32 value v' then satisfies |v' - ref| <= A (ReLU 1-Lipschitz)
    and |v'| <= |ref| + A.
  * hi = bf16(v'): |v' - hi| <= 2^-8 |v'| (8 significant bits, RNE).  r = v' - hi
    is exact in fp32 (its bits lie inside v's 24).  lo = bf16(r):
    |r - lo| <= 2^-8 |r| <= 2^-16 |v'| <= 2^-16 (|ref| + A): the second rounding
    of the stored pair.
  * where z <= -A under ReLU, v' = 0: both halves must be exactly 0.
  * the pair is well formed: |v' - hi| <= half an ulp of hi <= 2^-8 |hi|, a bf16
    value, and rounding is monotonic, so |lo| <= 2^-8 |hi| exactly (hi + lo is
    symmetric in the halves; this is what tells a swapped pair).

Exact operands.  fp32: fp16_ref.exact_operands (small integers).  split-bf16:
integers would leave every lo half 0, so
    x, sc, res = a + s 2^-9,  a in {0..3}, s in {-1, 0, 1}
    w = +-(1 + t 2^-9),  t in {-1, 0, 1}, at most 16 non-zeros per output row
    bias integer in -4..8; an identity shortcut adds the columns W1 = I
Every value survives the split (hi = a or +-1 -- or +-2^-9 when a = 0 --, lo =
+-2^-9 or 0), every product of two halves and every partial sum is a multiple of
2^-18 below 64 in magnitude, so all are exact in fp32 whatever the order
(checked per case: max S3 2^18 < 2^24).  The expected output is then, bit for
bit, to_split(ref.float()): the reference is exact in fp32 and the kernel's
re-split is the same two RNE roundings.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

import fp16_ref as R16
from heads_ref import worst_ratio

U = 2.0 ** -24
U2 = 2.0 ** -16           # the stored pair's second rounding
F64 = torch.float64
BF16 = torch.bfloat16
LSB = 2.0 ** -9


# ------------------------------------------------------------ case tables --
# N, H, W: the conv input; form: None | 'id' (identity K columns, a [N,Ho,Wo,Cout]
# source) | 'ds' (1x1/2 K columns over a [N,2Ho,2Wo,cin1] source) | 'res'
# (epilogue residual); channels are logical (32 per 128-B K-step in both modes)
Case = namedtuple('Case', 'N H W cin cout k stride pad form cin1 relu')


def _c(N, H, W, cin, cout, k=3, stride=1, form=None, cin1=0, relu=True):
    return Case(N, H, W, cin, cout, k, stride, k // 2, form, cout if form == 'id' else cin1, relu)


# The implicit-GEMM variants 9..19 (block.hip), shared by the fp32 and the
# split-bf16 tests: the smallest shapes that reach each edge.
GEMM_SHAPES = {
    '1x1 nk1 M15': _c(1, 3, 5, 32, 128, k=1),                      # 1 K-step: the ring never refills
    '1x1 nk2 M15': _c(1, 3, 5, 64, 128, k=1),                      # 2: the 2-stage ring's start-up
    '1x1 nk3 M15 linear': _c(1, 3, 5, 96, 128, k=1, relu=False),   # 3: the 3-stage ring's
    '1x1 M129 linear': _c(129, 1, 1, 32, 128, k=1, relu=False),    # one past the 128-pixel tile
    '1x1 M257': _c(1, 1, 257, 64, 128, k=1),                       # ... the 256-pixel tile
    '1x1 M513': _c(27, 19, 1, 32, 128, k=1),                       # ... the 512-pixel tile (16, 19)
    '3x3 s1 5x9': _c(2, 5, 9, 32, 128),
    '3x3 s2 5x9 linear': _c(3, 5, 9, 32, 128, stride=2, relu=False),
    '3x3 s2 9x5': _c(2, 9, 5, 64, 128, stride=2),
    '1x1 s2 5x9': _c(2, 5, 9, 64, 128, k=1, stride=2),
    '3x3 id 5x9 Cout64': _c(2, 5, 9, 64, 64, form='id'),
    '3x3 ds 5x9': _c(2, 5, 9, 32, 128, form='ds', cin1=32),
    '3x3 s1 7x6 Cout192': _c(1, 7, 6, 32, 192),
    '1x1 res M15 Cout256': _c(1, 3, 5, 64, 256, k=1, form='res'),  # variant 13's epilogue residual
    '1x1 ds M45 Cout256': _c(3, 3, 5, 32, 256, k=1, form='ds', cin1=64),  # ... its downsample columns
    '3x3 id 5x9 Cout256 linear': _c(1, 5, 9, 32, 256, form='id', relu=False),
}
GEMM_VARIANTS = [0, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19]
GEMM_BC = {9: 64, 10: 128, 11: 64, 12: 128, 13: 256, 14: 128, 15: 128, 16: 64, 17: 256, 18: 128, 19: 128}
FOUR_VARIANTS = [9, 13, 15]


def gemm_refusal(v, case):
    """None where launch_block_conv / launch_block_t accept the launch, else the
    text of the refusal (variant_fits first, then the residual rule).  Variant 0
    is the library's own choice and always fits."""
    if v == 0:
        return None
    if case.cout % GEMM_BC[v]:
        return 'channel tile does not divide Cout'
    if case.form == 'res' and v != 13:
        return 'no epilogue residual'
    return None


# The four-product form's own shape classes (tests/test_gpu_x3.py's
# test_block_conv_four_products) at small maps: name -> (case, variant)
FOUR_SHAPES = {
    'c1 1x1 64-64 v9': (_c(2, 5, 9, 64, 64, k=1), 9),
    'c2 3x3 64-64 v9': (_c(2, 5, 9, 64, 64), 9),
    'c2 3x3 s2 128-128 v15': (_c(2, 9, 5, 128, 128, stride=2), 15),
    'c3 1x1 res 128-256 v13': (_c(2, 5, 9, 128, 256, k=1, form='res'), 13),
    'c3 1x1 ds 64-256 v13': (_c(2, 5, 9, 64, 256, k=1, form='ds', cin1=128), 13),
    'c1 1x1 256-512 v15': (_c(2, 5, 9, 256, 512, k=1), 15),
}

# The 16 x 16-tiled split kernels.  form name -> (variant, cin, cout, stride, form, cin1).
# K-steps per tile in the split form: 9 per 32 logical channels + 1 per 32
# shortcut channels; halo31_ok / halo256_ok / halo256rs2_ok ask for whole
# 64-channel multiples, so the count is always even -- the carried weight-set /
# patch-buffer parity of variants 31 and 44 alternates per 64 channels instead:
# Cin 64 is 18 steps (an odd number of step pairs), Cin 128 is 36, Cin 64 + a
# 64-channel downsample 20 (even).
TILED_FORMS = {
    '42 plain': (42, 64, 64, 1, None, 0),
    '42 res': (42, 64, 64, 1, 'res', 0),
    '26 plain': (26, 64, 64, 1, None, 0),
    '26 res': (26, 64, 64, 1, 'res', 0),
    '20 c64 plain': (20, 64, 64, 1, None, 0),
    '20 c64 res': (20, 64, 64, 1, 'res', 0),
    '20 c128 plain': (20, 128, 128, 1, None, 0),
    '20 c128 res': (20, 128, 128, 1, 'res', 0),
    '30 c64 plain': (30, 64, 256, 1, None, 0),
    '30 c128 plain': (30, 128, 256, 1, None, 0),
    '30 c64 id': (30, 64, 256, 1, 'id', 256),
    '30 c128 ds': (30, 128, 256, 1, 'ds', 64),
    '31 t128 c64 plain': (31, 64, 128, 1, None, 0),       # 18 steps
    '31 t128 c128 id': (31, 128, 128, 1, 'id', 128),      # 36 + 4
    '31 t128 c64 ds': (31, 64, 128, 1, 'ds', 64),         # 18 + 2
    '31 t256 c64 plain': (31, 64, 256, 1, None, 0),
    '31 t256 c128 plain': (31, 128, 256, 1, None, 0),     # 36
    '31 t256 c64 id': (31, 64, 256, 1, 'id', 256),
    '31 t256 c64 ds': (31, 64, 256, 1, 'ds', 64),
    '44 c64-128': (44, 64, 128, 2, None, 0),              # 18 steps, 128-channel tiles
    '44 c128-256': (44, 128, 256, 2, None, 0),            # 36 steps, 256-channel tiles
    # without ReLU (negative outputs: the stored pair's signs; variants 20 and 26
    # have their own instantiations for it)
    '42 res linear': (42, 64, 64, 1, 'res', 0),
    '26 plain linear': (26, 64, 64, 1, None, 0),
    '20 c64 res linear': (20, 64, 64, 1, 'res', 0),
    '30 c64 plain linear': (30, 64, 256, 1, None, 0),
    '31 t128 c64 ds linear': (31, 64, 128, 1, 'ds', 64),
    '44 c64-128 linear': (44, 64, 128, 2, None, 0),
}
# output maps: one tile with all four edges, one tile row, one tile column,
# every edge class on a non-square map
TILED_MAPS = [(1, 16, 16), (1, 16, 32), (1, 32, 16), (2, 48, 32)]
# more tiles than workgroups: 257 images of one tile, five distinct ones, at each
# variant's smallest channel counts
MANY_FORMS = ['42 plain', '26 res', '20 c64 plain', '30 c64 plain', '31 t128 c64 plain', '31 t256 c64 plain',
              '44 c64-128']
MANY_N, MANY_DISTINCT = 257, 5
SPLIT_DEFAULTS = (42, 31, 30, 44)


def tiled_case(form, N, Ho, Wo):
    v, cin, cout, stride, f, cin1 = TILED_FORMS[form]
    return Case(N, Ho * stride, Wo * stride, cin, cout, 3, stride, 1, f, cin1, not form.endswith('linear')), v


def tiled_cases():
    """name -> (case, variant, slots): slots None, or the distinct-image index of
    each of the launch's images."""
    out = {}
    for form in TILED_FORMS:
        for (N, Ho, Wo) in TILED_MAPS:
            out[f'{form} {N}x{Ho}x{Wo}'] = tiled_case(form, N, Ho, Wo) + (None,)
    for form in MANY_FORMS:
        case, v = tiled_case(form, MANY_DISTINCT, 16, 16)
        g = torch.Generator().manual_seed(MANY_N)
        slots = torch.randperm(MANY_N, generator=g) % MANY_DISTINCT
        out[f'{form} {MANY_N}x16x16'] = (case, v, slots)
    return out


def out_hw(c):
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def shapes(c, extra=0):
    """(x, sc or None, res or None) shapes of a case with `extra` more images."""
    Ho, Wo = out_hw(c)
    n = c.N + extra
    sc = {'id': (n, Ho, Wo, c.cin1), 'ds': (n, 2 * Ho, 2 * Wo, c.cin1)}.get(c.form)
    return (n, c.H, c.W, c.cin), sc, (n, Ho, Wo, c.cout) if c.form == 'res' else None


def sc_stride(c):
    return 2 if c.form == 'ds' else 1


def k_terms(c):
    return c.k * c.k * c.cin + (c.cin1 if c.form in ('id', 'ds') else 0)


# ---------------------------------------------------------------- operands --
def _border(x, gen, scale):
    """large values on the image's border pixels: a padding slip is far over the bar"""
    big = torch.randn(x.shape, generator=gen) * scale
    if x.min() >= 0:
        big = big.abs()
    H, W = x.shape[1], x.shape[2]
    x[:, [0, H - 1]] = big[:, [0, H - 1]]
    x[:, :, [0, W - 1]] = big[:, :, [0, W - 1]]
    return x


def random_operands(gen, c, post_relu, extra=0):
    """(x, w, bias, sc, res) fp32: a quiet image with large border pixels (as
    tests/test_gpu_conv_igemm.py's), He-scaled weights, identity columns = I.
    post_relu: non-negative activations (the split mode's)."""
    xs, scs, rs = shapes(c, extra)
    act = (lambda t: t.clamp_min(0)) if post_relu else (lambda t: t * 0.5)
    x = _border(act(torch.randn(xs, generator=gen)), gen, 8.0)
    K0, K = c.k * c.k * c.cin, k_terms(c)
    w = torch.randn(c.cout, K, generator=gen) * (2.0 / K) ** 0.5
    if c.form == 'id':
        w[:, K0:] = torch.eye(c.cout)
    bias = torch.randn(c.cout, generator=gen)
    sc = _border(act(torch.randn(scs, generator=gen)), gen, 8.0) if scs else None
    res = act(torch.randn(rs, generator=gen)) if rs else None
    return x, w, bias, sc, res


def exact_operands_f32(gen, c):
    """fp16_ref.exact_operands as it is: for a 3x3 conv directly; for a 1x1 conv
    its weight matrix comes from a second call whose K = 9 * 0 + (cin + cin1)."""
    xs, scs, rs = shapes(c)
    cin1 = c.cin1 if c.form in ('id', 'ds') else 0
    x, w, bias, sc, _ = R16.exact_operands(gen, c.N, c.H, c.W, c.cin, c.cout, cin1, scs[1:3] if scs else None)
    if c.k == 1:
        w = R16.exact_operands(gen, 1, 1, 1, 0, c.cout, c.cin + cin1, (1, 1))[1]
    if c.form == 'id':
        w[:, c.k * c.k * c.cin:] = torch.eye(c.cout)
    res = torch.randint(0, 4, rs, generator=gen).float() if rs else None
    return x, w, bias, sc, res


def exact_operands_split(gen, c, nnz=16):
    """The split mode's exact operands (module docstring)."""
    def val(shape):
        return (torch.randint(0, 4, shape, generator=gen).float() +
                torch.randint(-1, 2, shape, generator=gen).float() * LSB)
    xs, scs, rs = shapes(c)
    K0, K = c.k * c.k * c.cin, k_terms(c)
    Kr = K0 if c.form == 'id' else K           # the identity's columns stay I
    w = torch.zeros(c.cout, K)
    cols = torch.rand(c.cout, Kr, generator=gen).argsort(1)[:, :nnz]
    sign = torch.randint(0, 2, cols.shape, generator=gen).float() * 2.0 - 1.0
    w.scatter_(1, cols, sign * (1.0 + torch.randint(-1, 2, cols.shape, generator=gen).float() * LSB))
    if c.form == 'id':
        w[:, K0:] = torch.eye(c.cout)
    bias = torch.randint(-4, 9, (c.cout,), generator=gen).float()
    return val(xs), w, bias, val(scs) if scs else None, val(rs) if rs else None


def sent_weights(c, w):
    """The weight matrix a launch gets.  With `res` the engine keeps the identity's
    K columns behind the taps (they are not read): rows are longer than K."""
    return torch.cat([w, torch.eye(c.cout)], dim=1).contiguous() if c.form == 'res' else w


# -------------------------------------------------------------- the split --
def parts(t):
    """fp32 -> (hi, lo) as fp32 values: hi = bf16(t), lo = bf16(t - hi), RNE."""
    hi = t.to(BF16).float()
    return hi, (t - hi).to(BF16).float()


def interleave(hi, lo):
    """(hi, lo) [..., C] -> the split layout [..., 2C] bf16, [hi(32) | lo(32)] per
    32 channels (sad.engine.to_split's layout; test_parity_reference checks it)."""
    C = hi.shape[-1]
    g = torch.stack([hi.to(BF16).reshape(*hi.shape[:-1], C // 32, 32),
                     lo.to(BF16).reshape(*hi.shape[:-1], C // 32, 32)], dim=-2)
    return g.reshape(*hi.shape[:-1], 2 * C).contiguous()


def halves(t):
    """the split layout [..., 2C] -> (hi, lo) [..., C] bf16"""
    g = t.reshape(*t.shape[:-1], t.shape[-1] // 64, 2, 32)
    C = t.shape[-1] // 2
    return g[..., 0, :].reshape(*t.shape[:-1], C), g[..., 1, :].reshape(*t.shape[:-1], C)


# -------------------------------------------------------------- contracts --
def _conv(c, x, w, sc, res=None, bias=None):
    """the pre-activation in float64 (fp16_ref.conv_ref without bias / ReLU unless given)"""
    b = bias if bias is not None else torch.zeros(w.shape[0], dtype=F64)
    return R16.conv_ref(x, w, b, c.stride, sc, sc_stride(c), res, relu=False, k=c.k, pad=c.pad)


def fp32_contract(c, x, w, bias, sc, res):
    """-> (ref, bar, must_be_zero or None), NHWC float64."""
    z = _conv(c, x, w, sc, res, bias)
    ab = lambda t: None if t is None else t.abs()  # noqa: E731
    S = _conv(c, x.abs(), w.abs(), ab(sc), ab(res), bias.abs())
    bar = (k_terms(c) + 8) * U * S
    return (z.clamp_min(0) if c.relu else z), bar, ((z <= -bar) if c.relu else None)


def split_pre(c, x, w, bias, sc, res, four):
    """(z, S3) float64: the pre-activation of the three- or four-product form on
    the stored halves of the fp32 operands, and the same sum on absolute values.
    (hi + lo)(hi + lo) - lo lo is the three products' sum, term for term."""
    d = lambda t: None if t is None else t.to(F64)  # noqa: E731
    xh, xl = parts(x)
    wh, wl = parts(w)
    sh, sl = parts(sc) if sc is not None else (None, None)
    add = lambda a, b: None if a is None else d(a) + d(b)  # noqa: E731
    ab = lambda t: None if t is None else t.abs()  # noqa: E731
    z = _conv(c, add(xh, xl), add(wh, wl), add(sh, sl))
    S = _conv(c, add(xh.abs(), xl.abs()), add(wh.abs(), wl.abs()), add(ab(sh), ab(sl)))
    if not four:
        z = z - _conv(c, xl, wl, sl)
        S = S - _conv(c, xl.abs(), wl.abs(), ab(sl))
    bb = bias.to(F64).view(1, 1, 1, -1)
    z, S = z + bb, S + bb.abs()
    if res is not None:
        rh, rl = parts(res)
        z, S = z + d(rh) + d(rl), S + d(rh).abs() + d(rl).abs()
    return z, S


def split_contract(c, x, w, bias, sc, res, four=False):
    """-> (ref, bar, must_be_zero or None, accumulation part A)."""
    z, S = split_pre(c, x, w, bias, sc, res, four)
    A = ((4 if four else 3) * k_terms(c) + 8) * U * S
    ref = z.clamp_min(0) if c.relu else z
    return ref, A + U2 * (ref.abs() + A), ((z <= -A) if c.relu else None), A


def split_ratio(out, ref, bar, zero):
    """worst |hi + lo - ref| / bar of a split-layout output; inf where the zero
    rule holds and either half is not exactly 0."""
    hi, lo = halves(out)
    hi, lo = hi.to(F64), lo.to(F64)
    r = worst_ratio(hi + lo, ref, bar, zero)
    if zero is not None and bool((zero & ((hi != 0) | (lo != 0))).any()):
        return float('inf')
    if bool((lo.abs() > 2.0 ** -8 * hi.abs()).any()):    # not a hi / lo pair (the sum alone is symmetric)
        return float('inf')
    return r


def split_expected(ref):
    """the stored output of an exact-in-fp32 reference, bit for bit"""
    from sad.engine import to_split
    return to_split(ref.float())


def differing(a, b):
    """per logical output [..., C]: either stored half differs in some bit"""
    (ah, al), (bh, bl) = halves(a), halves(b)
    i16 = lambda t: t.contiguous().view(torch.int16)  # noqa: E731
    return (i16(ah) != i16(bh)) | (i16(al) != i16(bl))


def exact_conditions(c, x, w, bias, sc, res):
    """The helper conditions of the split mode's exact operands -> dict of figures
    and the two stored expectations (three, four).  All must hold (check())."""
    from sad.engine import from_split, to_split
    z3, S3 = split_pre(c, x, w, bias, sc, res, False)
    z4, S4 = split_pre(c, x, w, bias, sc, res, True)
    post = (lambda t: t.clamp_min(0)) if c.relu else (lambda t: t)
    e3, e4 = split_expected(post(z3)), split_expected(post(z4))
    ops = [t for t in (x, w, sc, res) if t is not None]
    nzw = w[w != 0]
    fig = {
        'round_trip': all(torch.equal(from_split(to_split(t)), t) for t in ops),
        'ref_is_fp32': bool(torch.equal(z3.float().to(F64), z3) and torch.equal(z4.float().to(F64), z4)),
        'abs_sum_max': S4.max().item(),
        'nonzero_out': (post(z3) != 0).double().mean().item(),
        'x_lo': (parts(x)[1] != 0).double().mean().item(),
        'w_lo': (parts(nzw)[1] != 0).double().mean().item(),
        'three_four_differ': differing(e3, e4).double().mean().item(),
    }
    return fig, e3, e4


def check_conditions(fig):
    assert fig['round_trip'], 'an operand does not survive the split round trip'
    assert fig['ref_is_fp32'], 'the reference is not exact in fp32'
    assert fig['abs_sum_max'] * 2.0 ** 18 < 2.0 ** 24, fig
    assert fig['nonzero_out'] >= 0.25 and fig['x_lo'] >= 0.25 and fig['w_lo'] >= 0.25, fig
    assert fig['three_four_differ'] >= 0.05, fig


# ------------------------------------------------- CPU fp32 emulations ------
MUTANTS = [
    'W_lo.X_hi dropped at one tap for 4 channels',
    'X_lo zeroed at one corner pixel',
    "the residual's lo half ignored in one 32-channel group",
    'lo truncated, not rounded',
    'the other number of products',
    'hi and lo swapped within one 64-wide group',
]


def _conv_t(c, x, w, sc, dtype):
    """one product term in `dtype` (fp32: the emulation; float64: a mutant's effect), NHWC"""
    K0 = c.k * c.k * c.cin
    wc = w[:, :K0].to(dtype).reshape(w.shape[0], c.k, c.k, c.cin).permute(0, 3, 1, 2)
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), wc, stride=c.stride, padding=c.pad)
    if sc is not None:
        s = sc.to(dtype)[:, ::sc_stride(c), ::sc_stride(c), :][:, :y.shape[2], :y.shape[3], :]
        y = y + torch.einsum('nhwc,oc->nohw', s, w[:, K0:K0 + sc.shape[3]].to(dtype))
    return y.permute(0, 2, 3, 1)


def emulate_fp32(c, x, w, bias, sc, res):
    v = _conv_t(c, x, w, sc, torch.float32) + bias.view(1, 1, 1, -1)
    if res is not None:
        v = v + res
    return v.clamp_min(0) if c.relu else v


def emulate_split(c, x, w, bias, sc, res, four=False, mutant=None, dtype=torch.float32):
    """The split contract term by term in fp32 on the CPU (separate product convs,
    summed in fp32, re-split): the split-layout output a correct kernel could
    give.  mutant: one of MUTANTS, a plausible kernel slip."""
    xh, xl = parts(x)
    wh, wl = parts(w)
    sh, sl = parts(sc) if sc is not None else (None, None)
    wl_lh = wl
    if mutant == MUTANTS[0]:
        wl_lh = wl.clone()
        tap = (c.k * c.k) // 2
        wl_lh[:, tap * c.cin:tap * c.cin + 4] = 0
    if mutant == MUTANTS[1]:
        xl = xl.clone()
        xl[:, 0, 0, :] = 0
    if mutant == MUTANTS[4]:
        four = not four
    v = _conv_t(c, xh, wh, sh, dtype) + _conv_t(c, xh, wl_lh, sh, dtype) + _conv_t(c, xl, wh, sl, dtype)
    if four:
        v = v + _conv_t(c, xl, wl, sl, dtype)
    v = v + bias.to(dtype).view(1, 1, 1, -1)
    if res is not None:
        rh, rl = parts(res)
        if mutant == MUTANTS[2]:
            rl = rl.clone()
            rl[..., :32] = 0
        v = v + (rh + rl).to(dtype)
    v = (v.clamp_min(0) if c.relu else v).float()
    hi = v.to(BF16).float()
    r = v - hi
    lo = (r.view(torch.int32) & -65536).view(torch.float32) if mutant == MUTANTS[3] else r.to(BF16).float()
    out = interleave(hi, lo)
    if mutant == MUTANTS[5]:
        out = torch.cat([out[..., 32:64], out[..., :32], out[..., 64:]], dim=-1).contiguous()
    return out


def generator(kind, name):
    """the seeded generator of one case's operands (kind: 'exact' | 'random' | ...)"""
    import zlib
    return torch.Generator().manual_seed(zlib.crc32(f'{kind}-{name}'.encode()))
