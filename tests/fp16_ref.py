"""Float64 contract of an fp16 (SAD_F16) conv, with its a-priori bar (no GPU
work here; tests/test_fp16_reference.py checks this file on the CPU, the GPU
tests of the fp16 kernels compare with it).

Contract.  Operands (activations, weights, shortcut source, residual) are fp16
values; products are exact in fp32's accumulator format up to its rounding;
out = fp16_rne(relu(conv(x, w) + shortcut + bias + res)), accumulated in fp32
in any order, saturated to +-65504.

Bar, written down before any run:

    |out - ref| <= 2^-11 |ref| + 4 sqrt(K) 2^-24 max|ref|

  * 2^-11 |ref|: one round-to-nearest-even of the output to fp16 (11 significant
    bits);
  * 4 sqrt(K) 2^-24 max|ref|: the fp32 accumulation of K terms under any
    summation order (K = taps x channels + shortcut channels), as a floor on the
    tensor's scale.
Random operands stay in fp16's normal range: |x| and |w| are zero or in
[2^-8, 8], so flush-to-zero of subnormals cannot decide a case.

The stem's bar is tests/stem_ref.py's bf16 formula evaluated with the output
and operand rounding of fp16, u16 = 2^-11 (stem_ref hard-codes bf16's 2^-8).
"""
import math

import torch
import torch.nn.functional as F

import stem_ref as S

U16 = 2.0 ** -11
U32 = 2.0 ** -24
F16_MAX = 65504.0
F64 = torch.float64


def f16(x):
    """float64 -> the float64 value of its fp16 RNE rounding."""
    return x.to(torch.float32).to(torch.float16).to(F64)


def rand_f16(gen, *shape, zero_frac=0.05, lo=-8, hi=3):
    """fp16 tensor: zero with probability ~zero_frac, else +-2^e m with e uniform
    in [lo, hi) and m in [1, 2) (all 10 mantissa bits random): magnitudes in
    [2^-8, 8), fp16-exact.  One random word per element, assembled as fp16 bits."""
    r = torch.randint(0, (1 << 31) - 1, shape, generator=gen, dtype=torch.int32)
    sign, mant = r & 1, (r >> 1) & 1023
    e = ((r >> 11) & 1023) % (hi - lo) + lo + 15               # the biased exponent field
    bits = (sign << 15) | (e << 10) | mant
    bits = torch.where(((r >> 21) & 1023) < int(zero_frac * 1024), torch.zeros_like(bits), bits)
    v = (bits - ((bits >> 15) << 16)).to(torch.int16).view(torch.float16)
    return v


def conv_ref(x, w, bias, stride=1, sc=None, sc_stride=1, res=None, relu=True, k=3, pad=None):
    """float64 NHWC reference of the block-conv contract on exact operands:
    x [N,H,W,Cin], w [Cout, k k Cin (+ Cin1)] (taps first, k = (ky, kx, ci), then
    the shortcut's columns), bias [Cout], sc [N,H1,W1,Cin1] sampled at
    (oy, ox) sc_stride, res [N,Ho,Wo,Cout]."""
    cin = x.shape[3]
    pad = k // 2 if pad is None else pad
    wc = w[:, :k * k * cin].to(F64).reshape(w.shape[0], k, k, cin).permute(0, 3, 1, 2)
    y = F.conv2d(x.to(F64).permute(0, 3, 1, 2), wc, stride=stride, padding=pad)
    if sc is not None:
        w1 = w[:, k * k * cin:k * k * cin + sc.shape[3]].to(F64)
        s = sc.to(F64)[:, ::sc_stride, ::sc_stride, :][:, :y.shape[2], :y.shape[3], :]
        y = y + torch.einsum('nhwc,oc->nohw', s, w1)
    y = y + bias.to(F64).view(1, -1, 1, 1)
    if res is not None:
        y = y + res.to(F64).permute(0, 3, 1, 2)
    if relu:
        y = y.clamp_min(0)
    return y.permute(0, 2, 3, 1).contiguous()


def bar(ref, K):
    """The bar above, elementwise, for a reference tensor and its K."""
    return U16 * ref.abs() + 4.0 * math.sqrt(K) * U32 * ref.abs().max()


def over_bar(out, ref, K):
    """(fraction of elements over the bar, worst |d| / bar); non-finite outputs count as over."""
    d = (out.to(F64) - ref).abs()
    b = bar(ref, K)
    bad = ~(d <= b) | ~torch.isfinite(out.to(F64))
    ratio = torch.where(b > 0, d / b.clamp_min(1e-300), torch.where(d > 0, math.inf, 0.0))
    return bad.double().mean().item(), ratio.max().item()


def saturate(ref):
    """The contract's saturation: fp16 stores clamp to +-65504."""
    return ref.clamp(-F16_MAX, F16_MAX)


# ---- exact operands: every operand, product, partial sum and output is an
# integer of small magnitude, exact in bf16, fp16 and fp32 alike
def exact_operands(gen, N, H, W, cin, cout, cin1=0, sc_hw=None, res=False, nnz=16):
    """x, sc, res: integers 0..3; w [cout, 9 cin + cin1]: {-1, 0, 1} with at
    most `nnz` non-zeros per output row; bias: integers -4..8 (fp32)."""
    x = torch.randint(0, 4, (N, H, W, cin), generator=gen).float()
    K = 9 * cin + cin1
    w = torch.zeros(cout, K)
    for o in range(cout):
        idx = torch.randperm(K, generator=gen)[:nnz]
        w[o, idx] = torch.randint(0, 2, (nnz,), generator=gen).float() * 2.0 - 1.0
    bias = torch.randint(-4, 9, (cout,), generator=gen).float()
    sc = torch.randint(0, 4, (N, sc_hw[0], sc_hw[1], cin1), generator=gen).float() if cin1 else None
    r = torch.randint(0, 4, (N, H, W, cout), generator=gen).float() if res else None
    return x, w, bias, sc, r


# ---- the stem: stem_ref's bf16 bar formula with u = 2^-11
K_ACC_STEM = 64 + 8  # the bf16 / fp16 stems' 64 tap slots (stem_ref.K_ACC['bf16'])


def stem_reference(fd, map=None, img=None, image_err=None):
    """(ref, bar) NHWC [B,128,128,64] float64 of one fp16 stem launch: the image
    (the resized map, or img) and the folded weights rounded to fp16."""
    assert (map is not None) + (img is not None) == 1
    x = f16(S.resize(map) if map is not None else img.to(F64))
    w = f16(fd.w32)
    c = S.conv7(x, w)
    e = K_ACC_STEM * S.U * S.conv7(x.abs(), w.abs())
    if image_err is not None:
        e = e + S.conv7(image_err.to(F64), w.abs())
    v = S.pool(c) + fd.bias.view(1, -1, 1, 1)
    ref = torch.relu(v)
    b = S.pool(e) + S.U * v.abs() + U16 * ref
    return ref.permute(0, 2, 3, 1).contiguous(), b.permute(0, 2, 3, 1).contiguous()
