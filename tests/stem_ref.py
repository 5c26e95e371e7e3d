"""Float64 reference of the inference stem's contract, with a-priori rounding
bars (no GPU work here; tests/test_stem_reference.py checks this file on the
CPU, tests/test_gpu_stem.py compares the kernels of csrc/conv.hip with it).

The contract (what api.hip fold_stem and the three stem kernels promise; stated
from the operation, not from their code):

Weights.  scale = gamma / sqrt(var + 1e-5), float64.  The folded stems sum the
three identical input channels: w[co][ky][kx] = (sum_c W[co,c,ky,kx]) scale[co],
rounded once to fp32 (fp32 stem), then to bf16 RNE (bf16 stem), or split
hi = bf16(w32), lo = bf16(w32 - hi) (split-bf16 stem).  bias = fp32(beta - mean
scale).  The distinct-channel stem keeps fp32(W scale) per channel.

Image.  map path: bilinear resize to 512 x 512, align_corners=False, source
coordinate clamped at 0 from below and the second tap at the last row/column;
then quantised as the dtype demands (bf16 RNE | hi/lo split | nothing).  img /
img3 paths: the input itself (img3: fp32 arithmetic whatever the plan dtype).

Conv 7x7 stride 2 pad 3 in float64 on exactly those operands; the split stem is
the full product minus the lo.lo term (the deep plans' X4 stem keeps it); then
max over the 3x3 stride 2 pad 1 window, + bias, ReLU, and the output rounding
(fp32 | bf16 | split: hi + lo).

Bars, u = 2^-24 (one fp32 rounding), BF = 2^-8, written down before any run:
  accumulation  K u S,  S = conv(|x|, |w|),  K = accumulate length + 8:
                64 tap slots (bf16, split-bf16), 49 (fp32), 147 (distinct channels)
  image error   conv(e_img, |w|) where the caller passes e_img (a map whose
                fp32 resize is not exact: 8 u of the lerp terms)
  pooled        the largest such bar in the window (max and ReLU are 1-Lipschitz)
  bias add      + u |v|
  output        bf16: + BF |ref|;  split: + 2^-16 |ref|
Every element is compared; none is left out.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
BF = 2.0 ** -8
DTYPES = ('fp32', 'bf16', 'bf16x3')
K_ACC = {'fp32': 49 + 8, 'bf16': 64 + 8, 'bf16x3': 64 + 8}
K_ACC3 = 147 + 8
F64 = torch.float64

Folded = namedtuple('Folded', 'w32 bias w3 scale')


def f32(x):
    """float64 -> the float64 value of its fp32 rounding."""
    return x.to(torch.float32).to(F64)


def bf16(x):
    """float64 (holding fp32 values) -> the float64 value of its bf16 RNE rounding."""
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def split(x):
    """(hi, lo) of an fp32-valued float64 tensor: hi = bf16(x), lo = bf16(x - hi)."""
    hi = bf16(x)
    return hi, bf16(x - hi)


def fold(W, gamma, beta, mean, var):
    """conv1.weight [64,3,7,7] and bn1's four vectors (fp32 tensors) -> Folded:
    w32 [64,7,7] (fp32 values), bias [64] (fp32 values), w3 [64,3,7,7], scale."""
    scale = gamma.to(F64) / torch.sqrt(var.to(F64) + 1e-5)
    w = W.to(F64).sum(dim=1) * scale.view(-1, 1, 1)
    bias = f32(beta.to(F64) - mean.to(F64) * scale)
    w3 = f32(W.to(F64) * scale.view(-1, 1, 1, 1))
    return Folded(f32(w), bias, w3, scale)


def weight_planes(dtype, fd):
    """The folded stem's weight operands: (w,) or (hi, lo), each [64,7,7]."""
    if dtype == 'fp32':
        return (fd.w32,)
    if dtype == 'bf16':
        return (bf16(fd.w32),)
    return split(fd.w32)


def quantise(x, dtype):
    """The image operands of an fp32-valued image: (x,), (bf16 x,) or (hi, lo)."""
    if dtype == 'fp32':
        return (x,)
    if dtype == 'bf16':
        return (bf16(x),)
    return split(f32(x))


def _axis(n_src, dt, clamp):
    """512 output coordinates on a source axis of n_src: (i0, i1, l).  The
    coordinate n_src (2i + 1) / 1024 - 1/2 has at most 20 significant bits."""
    src = torch.arange(512, dtype=dt) + 0.5
    src = src * (n_src / 512.0) - 0.5
    if clamp:
        src = src.clamp(min=0.0)
    i0 = src.floor().clamp(min=0.0)        # (no clamp: the first tap stays in the map, l goes negative)
    lam = src - i0
    i0 = i0.long().clamp(max=n_src - 1)
    return i0, (i0 + 1).clamp(max=n_src - 1), lam


def resize(m, dt=F64, order='xy', clamp=True):
    """[B, mh, mw] -> [B, 512, 512] in arithmetic `dt`.  order 'xy' lerps along
    x first, 'yx' along y first (the same value where every step is exact)."""
    m = m.to(dt)
    y0, y1, ly = _axis(m.shape[1], dt, clamp)
    x0, x1, lx = _axis(m.shape[2], dt, clamp)
    ly = ly.view(1, -1, 1)
    lx = lx.view(1, 1, -1)
    if order == 'xy':
        u = (1 - lx) * m[:, :, x0] + lx * m[:, :, x1]
        return (1 - ly) * u[:, y0, :] + ly * u[:, y1, :]
    v = (1 - ly) * m[:, y0, :] + ly * m[:, y1, :]
    return (1 - lx) * v[:, :, x0] + lx * v[:, :, x1]


def exact_map(gen, B, mh, mw):
    """Values k/4, k a random integer in [-8, 8): with lerp weights of at most
    10 fractional bits per axis every intermediate of the resize fits 24 bits."""
    return torch.randint(-8, 8, (B, mh, mw), generator=gen).to(torch.float32) / 4.0


def random_stem_params(gen):
    """conv1.weight and bn1 (weight, bias, running_mean, running_var) with every
    fifth gamma negative, one gamma zero and non-trivial running statistics."""
    W = torch.randn(64, 3, 7, 7, generator=gen) * 0.05
    gamma = torch.rand(64, generator=gen) + 0.5
    gamma[::5] *= -1.0
    gamma[7] = 0.0
    beta = torch.randn(64, generator=gen) * 0.2
    mean = torch.randn(64, generator=gen) * 0.3
    var = torch.rand(64, generator=gen) * 1.5 + 0.25
    return W, gamma, beta, mean, var


def adversarial_image(gen, B):
    """[B,512,512]: a quiet image with large values where the kernels' tiles
    meet, so that a seam decides the max: image rows and columns 0 and 511, the
    centre columns of conv columns 63/64, 127/128, 191/192 (wave seams), and the
    centre rows of the conv rows around every pooled-row pair boundary 8k-1 / 8k
    (block and workgroup seams)."""
    x = torch.randn(B, 512, 512, generator=gen) * 0.25
    big = torch.randn(B, 512, 512, generator=gen) * 4.0
    cols = [0, 511] + [2 * c for c in (63, 64, 127, 128, 191, 192)]
    rows = [0, 511] + [2 * r for k in range(1, 16) for r in range(16 * k - 3, 16 * k + 2)]
    x[:, :, cols] = big[:, :, cols]
    x[:, rows, :] = big[:, rows, :]
    return x


def resize_is_exact(m):
    """The precondition of the quantised map paths: the float32 resize, in
    either order, equals the float64 one bit for bit, and that equals torch's."""
    r64 = resize(m)
    ok = torch.equal(resize(m, torch.float32, 'xy').to(F64), r64)
    ok = ok and torch.equal(resize(m, torch.float32, 'yx').to(F64), r64)
    ok = ok and torch.equal(resize(m, F64, 'yx'), r64)
    ti = F.interpolate(m.to(F64).unsqueeze(1), size=(512, 512), mode='bilinear', align_corners=False).squeeze(1)
    return ok and torch.equal(ti, r64)


def conv7(x, w):
    """x [B,512,512] or [B,C,512,512], w [64,7,7] or [64,C,7,7] (float64) -> [B,64,256,256]."""
    if x.dim() == 3:
        x = x.unsqueeze(1)
    if w.dim() == 3:
        w = w.unsqueeze(1)
    return F.conv2d(x, w, stride=2, padding=3)


def pool(c):
    """max over the 3x3 stride 2 pad 1 window, [B,64,256,256] -> [B,64,128,128]."""
    return F.max_pool2d(c, 3, 2, 1)


def band_source_rows(mh):
    """Per workgroup of the bf16 stems (16 of them, 8 pooled rows each: image
    rows 32g - 5 .. 32g + 34 clipped to the image): the number of map rows its
    band reads, first tap of the first row to second tap of the last."""
    y0, y1, _ = _axis(mh, F64, True)
    return [int(y1[min(32 * g + 34, 511)]) - int(y0[max(32 * g - 5, 0)]) + 1 for g in range(16)]


def separable_workgroups(mh):
    """Which workgroups take the two-pass resize: those whose band spans at most
    12 map rows (STEM_HROWS); the others resize per pixel."""
    return [n <= 12 for n in band_source_rows(mh)]


def reference(dtype, fd, map=None, img=None, img3=None, four=False, image_err=None, resize_fn=resize,
              quantise_fn=quantise, edit_image=None, edit_weights=None, edit_conv=None, pool_fn=pool):
    """(ref, bar), both NHWC [B,128,128,64] float64, of one stem launch with
    exactly one of map [B,mh,mw], img [B,512,512], img3 [B,3,512,512] (fp32
    tensors).  four: keep the split stem's lo.lo product.  image_err [B,512,512]:
    a bound of |image used - image here|.  The *_fn / edit_* hooks replace or
    edit one stage (the sharpness tests' mutated references)."""
    assert dtype in DTYPES and (map is not None) + (img is not None) + (img3 is not None) == 1
    if img3 is not None:
        xs, ws, K = (img3.to(F64),), (fd.w3,), K_ACC3
    else:
        x = resize_fn(map) if map is not None else img.to(F64)
        xs, ws, K = quantise_fn(x, dtype), weight_planes(dtype, fd), K_ACC[dtype]
    if edit_image:
        xs = edit_image(xs)
    if edit_weights:
        ws = edit_weights(ws)
    xf, wf = sum(xs), sum(ws)
    c = conv7(xf, wf)
    if len(xs) == 2 and not four:
        c = c - conv7(xs[1], ws[1])
    if edit_conv:
        c = edit_conv(c, xs, ws)
    e = K * U * conv7(xf.abs(), wf.abs())
    if image_err is not None:
        e = e + conv7(image_err.to(F64), wf.abs())
    v = pool_fn(c) + fd.bias.view(1, -1, 1, 1)
    ref = torch.relu(v)
    bar = pool(e) + U * v.abs()
    if dtype == 'bf16':
        bar = bar + BF * ref
    elif dtype == 'bf16x3':
        bar = bar + 2.0 ** -16 * ref
    return ref.permute(0, 2, 3, 1).contiguous(), bar.permute(0, 2, 3, 1).contiguous()


def round_output(ref, dtype):
    """The float64 value a stem stores for `ref` in the plan dtype."""
    if dtype == 'fp32':
        return f32(ref)
    if dtype == 'bf16':
        return bf16(ref)
    hi, lo = split(f32(ref))
    return hi + lo


def decode(out, dtype):
    """A stem's output tensor (CPU; fp32 [..,64], bf16 [..,64] or split bf16
    [..,128] = per 32 channels [hi 32 | lo 32]) -> float64 [..,64]."""
    if dtype != 'bf16x3':
        return out.to(F64)
    g = out.to(F64).reshape(*out.shape[:-1], 2, 2, 32)
    return (g[..., 0, :] + g[..., 1, :]).reshape(*out.shape[:-1], 64)


def worst_ratio(got, ref, bar):
    """max over ALL elements of |got - ref| / bar (inf where an element with a
    zero bar differs; nan and inf in got count as failures)."""
    d = (got - ref).abs()
    r = torch.where(bar > 0, d / bar.clamp(min=np.finfo(np.float64).tiny), torch.where(d > 0, np.inf, 0.0))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, np.inf))
    return r.max().item()
