"""Float64 reference of the heads + merge contract, with a-priori rounding bars
(no GPU work here; tests/test_heads_reference.py checks this file on the CPU,
tests/test_gpu_heads.py compares sad_heads_merge_run with it).

The contract (inference_runner.py:36-73 in eval mode; stated from the
operation, not from the code of csrc/api.hip and csrc/heads.hip): per head h,
on the pooled features x of backbone feat_index[h],
  y1 = relu(bn1(Linear(feat_dim, 512)(x)))
  y2 = relu(bn2(Linear(512, 256)(y1)))
  z  = Linear(256, 2)(y2)                       [Real, Synthetic]
and merged = [z_1[1] .. z_N[1], mean_h z_h[0]].

Fold.  scale = gamma / sqrt(var + 1e-5) in float64; w' = fp32(W scale), rounded
once; b' = fp32(b scale + beta - mean scale).  The last Linear is unfolded.

Stage references.  Every stage is computed in float64 on exactly the input the
device had for it: the features (stage 1), the device's own stored y1 (stage
2), its own stored y2 (stage 3).  A stage's bar then covers that stage's
arithmetic alone.

Bars, u = 2^-24, written down before any run:
  per element  (K + 8) u (sum_i |x_i| |w'_oi| + |b'_o|),  K = feat_dim, 512, 256.
  It holds for ANY summation order of an fp32 FMA chain of K terms plus the
  bias (the MFMA 16x16x4 chains; heads_final's 4 products per lane + 6 shuffle
  steps).  ReLU is 1-Lipschitz: the bar is unchanged, and where the float64
  pre-activation is <= -bar the stored value must be exactly 0.
  merged[:, h] == logits[:, h, 1] bit for bit;
  |merged[:, N] - mean64(logits[:, :, 0])| <= (N + 2) u sum_h |logits[:, h, 0]| / N.
Every element is compared; none is left out.  No whole-chain bar is asserted: a
worst-case bar propagated through the three layers reaches 1e-2..1e-1 of |z|
with the small-variance channels used here, which would check nothing.

Workspace layout (include/sad.h): y1 [B][N*512] at the start, head h at column
512 rank(h), rank ordering heads by (feat_index[h], h); y2 [B][N*256] at float
offset B*N*512, head h at column 256 h.
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
F64 = torch.float64
EPS = 1e-5
HEAD_KEYS = ['2.weight', '2.bias', '3.weight', '3.bias', '3.running_mean', '3.running_var',
             '6.weight', '6.bias', '7.weight', '7.bias', '7.running_mean', '7.running_var',
             '10.weight', '10.bias']

Folded = namedtuple('Folded', 'w1 b1 w2 b2 w3 b3')
Case = namedtuple('Case', 'name n_heads feat_index n_feat feat_dim B seed')

# (N, feat_index, n_feat, feat_dim)
PLANS = [
    (1, [0], 1, 512),
    (2, [0, 0], 1, 512),
    (6, [0] * 6, 1, 512),            # the bench's plan
    (7, [0] * 7, 1, 512),
    (3, [0, 1, 2], 3, 512),
    (4, [0, 1, 0, 1], 2, 512),
    (2, [1, 0], 2, 512),
    (4, [0, 1, 2, 0], 3, 512),
    (2, [0, 2], 3, 512),             # feature group 1 is empty: its pointer is NULL
    (2, [0, 1], 2, 64),
    (3, [0, 0, 1], 2, 2048),
]
# either side of the 128-row GEMM tile, B % 4 != 0 (heads_final: 4 rows per block)
ROW_COUNTS = [1, 3, 127, 128, 129, 257]
SMALL_B = 5


def _cases():
    out = []
    for i, (n, fi, nf, d) in enumerate(PLANS):
        full = (n, fi) in ((6, [0] * 6), (4, [0, 1, 2, 0]))
        for B in (ROW_COUNTS if full else [SMALL_B]):
            name = f"N{n}-{''.join(map(str, fi))}-nf{nf}-d{d}-B{B}"
            out.append(Case(name, n, fi, nf, d, B, 1000 + 17 * i + B))
    return out


CASES = _cases()


def row_range(N, feat_dim):
    """Rows per GEMM launch of sad_heads_merge_run, restated from the 2 GiB
    buffer range of its two input operands: ((rows - 1) stride + K) 4 bytes
    < 2^31 - 64 with (stride, K) = (feat_dim, feat_dim) and (512 N, 512); whole
    512-row tiles."""
    room = (2 ** 31 - 64 - 1) // 4
    r = min((room - feat_dim) // feat_dim + 1, (room - 512) // (512 * N) + 1)
    return r - r % 512 if r >= 512 else r


# The large batch: 64 heads on one backbone, one full row range and a ragged
# second one (2 tiles + 5 rows, B % 4 != 0).  LARGE_ROWS: the rows around the
# range boundary, the first rows (the zero and the 1e4 row among them) and the
# last; as a small batch they are an input set like any other.
LARGE_N = 64
LARGE_B = row_range(LARGE_N, 512) + 261
LARGE_ROWS = sorted({0, 1, 2, 127, 128, LARGE_B - 3, LARGE_B - 2, LARGE_B - 1}
                    | {row_range(LARGE_N, 512) + d for d in (-3, -2, -1, 0, 1, 2)})
LARGE = Case(f'N{LARGE_N}-large-rows', LARGE_N, [0] * LARGE_N, 1, 512, LARGE_B, 4242)


def make_large():
    """-> (head_sds [64], features [LARGE_B, 512] fp32)."""
    gen = torch.Generator().manual_seed(LARGE.seed)
    sds = [random_head(gen, 512) for _ in range(LARGE_N)]
    return sds, random_features(gen, LARGE_B, 512)


def f32(x):
    """float64 -> the float64 value of its fp32 rounding."""
    return x.to(torch.float32).to(F64)


# ------------------------------------------------------------------ inputs --
def random_head(gen, feat_dim):
    """One head's state dict (nn.Sequential index keys, fp32).  BN statistics
    under which a fold mistake shows: var in [0.25, 4] with every 16th channel in
    1e-6 .. 1e-3 (eps matters), gamma of both signs with every 7th exactly 0."""
    def bn(c):
        var = torch.rand(c, generator=gen) * 3.75 + 0.25
        small = torch.arange(0, c, 16)
        var[small] = 10.0 ** (torch.rand(len(small), generator=gen) * 3.0 - 6.0)
        gamma = (torch.rand(c, generator=gen) + 0.5) * torch.where(torch.rand(c, generator=gen) < 0.4, -1.0, 1.0)
        gamma[::7] = 0.0
        return gamma, torch.randn(c, generator=gen) * 0.3, torch.randn(c, generator=gen) * 0.5, var
    sd = {}
    for idx, (o, i) in ((2, (512, feat_dim)), (6, (256, 512)), (10, (2, 256))):
        sd[f'{idx}.weight'] = torch.randn(o, i, generator=gen) * (2.0 / i) ** 0.5
        sd[f'{idx}.bias'] = torch.randn(o, generator=gen) * 0.2
    for idx, c in ((3, 512), (7, 256)):
        g, b, m, v = bn(c)
        sd[f'{idx}.weight'], sd[f'{idx}.bias'], sd[f'{idx}.running_mean'], sd[f'{idx}.running_var'] = g, b, m, v
    return sd


def random_features(gen, B, feat_dim):
    """[B, feat_dim] fp32, both signs; row 1 all zero and row 2 scaled by 1e4
    where the batch has them."""
    x = torch.randn(B, feat_dim, generator=gen)
    if B > 1:
        x[1] = 0.0
    if B > 2:
        x[2] *= 1e4
    return x


def make_case(case):
    """-> (head_sds [N], feats [n_feat] of fp32 [B, feat_dim] or None for a
    feature group no head reads).  Weights differ per head."""
    gen = torch.Generator().manual_seed(case.seed)
    sds = [random_head(gen, case.feat_dim) for _ in range(case.n_heads)]
    used = set(case.feat_index)
    feats = [random_features(gen, case.B, case.feat_dim) if f in used else None for f in range(case.n_feat)]
    return sds, feats


# -------------------------------------------------------------------- fold --
def bn_scale(gamma, var):
    return gamma.to(F64) / torch.sqrt(var.to(F64) + EPS)


def fold_linear_bn(W, b, gamma, beta, mean, var, scale_fn=bn_scale, rounded=True, scaled_bias=True):
    scale = scale_fn(gamma, var)
    shift = beta.to(F64) - mean.to(F64) * scale
    w = W.to(F64) * scale.view(-1, 1)
    bb = (b.to(F64) * scale if scaled_bias else b.to(F64)) + shift
    return (f32(w), f32(bb)) if rounded else (w, bb)


def fold(sd, **kw):
    """One head's state dict -> Folded (float64 tensors holding fp32 values;
    rounded=False: the exact float64 fold).  scale_fn / scaled_bias: the fold
    mutants of the sharpness tests."""
    w1, b1 = fold_linear_bn(*[sd[k] for k in HEAD_KEYS[0:6]], **kw)
    w2, b2 = fold_linear_bn(*[sd[k] for k in HEAD_KEYS[6:12]], **kw)
    return Folded(w1, b1, w2, b2, sd['10.weight'].to(F64), sd['10.bias'].to(F64))


# ------------------------------------------------------------------ layout --
def rank(feat_index):
    """rank[h] = position of head h among the heads ordered by (feat_index[h], h)."""
    order = sorted(range(len(feat_index)), key=lambda h: (feat_index[h], h))
    r = [0] * len(feat_index)
    for pos, h in enumerate(order):
        r[h] = pos
    return r


def is_regular(feat_index):
    """The second layer runs as one grouped launch iff the heads' hidden
    columns are in head order; otherwise as one launch per head."""
    return all(r == h for h, r in enumerate(rank(feat_index)))


def workspace_floats(B, N):
    return B * N * (512 + 256)


def split_workspace(ws, B, feat_index):
    """Flat fp32 workspace -> (y1 [B,N,512], y2 [B,N,256]) in HEAD order."""
    N = len(feat_index)
    y1 = ws[:B * N * 512].view(B, N, 512)[:, rank(feat_index), :]
    y2 = ws[B * N * 512:B * N * 768].view(B, N, 256)
    return y1, y2


# --------------------------------------------------------------- reference --
def stage(x, w, b, relu=True):
    """x [B,K], w [O,K], b [O] float64 -> (pre-activation z, ref, bar), [B,O]."""
    K = x.shape[1]
    z = x @ w.t() + b
    bar = (K + 8) * U * (x.abs() @ w.abs().t() + b.abs())
    return z, (torch.relu(z) if relu else z), bar


def chain(folded, feats, feat_index):
    """The whole contract in float64 from the features: (y1, y2, logits, merged)."""
    y1, y2, lg = [], [], []
    for h, fd in enumerate(folded):
        a = stage(feats[feat_index[h]].to(F64), fd.w1, fd.b1)[1]
        b = stage(a, fd.w2, fd.b2)[1]
        y1.append(a)
        y2.append(b)
        lg.append(stage(b, fd.w3, fd.b3, relu=False)[1])
    logits = torch.stack(lg, dim=1)
    merged = torch.cat([logits[:, :, 1], logits[:, :, 0].mean(dim=1, keepdim=True)], dim=1)
    return torch.stack(y1, dim=1), torch.stack(y2, dim=1), logits, merged


def worst_ratio(got, ref, bar, must_be_zero=None):
    """max over ALL elements of |got - ref| / bar (inf where an element with a
    zero bar differs, where got is nan or inf, and where must_be_zero holds and
    got is not exactly 0)."""
    got = got.to(F64)
    d = (got - ref).abs()
    tiny = np.finfo(np.float64).tiny
    r = torch.where(bar > 0, d / bar.clamp(min=tiny), torch.where(d > 0, np.inf, 0.0).to(F64))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, np.inf))
    if must_be_zero is not None:
        r = torch.where(must_be_zero & (got != 0), torch.full_like(r, np.inf), r)
    return r.max().item() if r.numel() else 0.0


def compare(folded, feats, feat_index, ws, logits, merged):
    """The comparison both the CPU stand-in and the GPU run go through.
    ws: flat fp32 workspace (>= B N 768 floats), logits [B,N,2], merged [B,N+1]
    (CPU fp32 tensors).  -> {'stage1', 'stage2', 'stage3', 'merge_syn',
    'merge_real'}: worst error / bar over all elements; pass iff every one <= 1."""
    N, B = len(feat_index), logits.shape[0]
    y1, y2 = split_workspace(ws, B, feat_index)
    r = {'stage1': 0.0, 'stage2': 0.0, 'stage3': 0.0}
    for h, fd in enumerate(folded):
        z, ref, bar = stage(feats[feat_index[h]].to(F64), fd.w1, fd.b1)
        r['stage1'] = max(r['stage1'], worst_ratio(y1[:, h], ref, bar, z <= -bar))
        z, ref, bar = stage(y1[:, h].to(F64), fd.w2, fd.b2)
        r['stage2'] = max(r['stage2'], worst_ratio(y2[:, h], ref, bar, z <= -bar))
        z, ref, bar = stage(y2[:, h].to(F64), fd.w3, fd.b3, relu=False)
        r['stage3'] = max(r['stage3'], worst_ratio(logits[:, h], ref, bar))
    syn_same = torch.equal(merged[:, :N].contiguous().view(torch.int32), logits[:, :, 1].contiguous().view(torch.int32))
    r['merge_syn'] = 0.0 if syn_same else float('inf')
    real = logits[:, :, 0].to(F64)
    r['merge_real'] = worst_ratio(merged[:, N], real.mean(dim=1), (N + 2) * U * real.abs().sum(dim=1) / N)
    return r


def passes(ratios):
    return all(v <= 1.0 for v in ratios.values())


# ---------------------------------------------------- CPU fp32 stand-in ------
FILL = -777.0


def standin(head_sds, feats, feat_index, mutant=None):
    """The three stages + merge in fp32 on the CPU, writing the device's
    workspace layout: (ws flat fp32, logits, merged).  mutant: one of MUTANTS
    (a plausible kernel or plan bug) or None."""
    N = len(feat_index)
    B = next(f for f in feats if f is not None).shape[0]
    kw = {}
    if mutant == 'eps dropped':
        kw['scale_fn'] = lambda g, v: g.to(F64) / torch.sqrt(v.to(F64))
    elif mutant == 'eps outside the square root':
        kw['scale_fn'] = lambda g, v: g.to(F64) / (torch.sqrt(v.to(F64)) + EPS)
    elif mutant == 'Linear bias not scaled':
        kw['scaled_bias'] = False
    folded = [fold(sd, **kw) for sd in head_sds]
    f = lambda t: t.to(torch.float32)
    rk = rank(feat_index)
    ws = torch.full((workspace_floats(B, N),), FILL, dtype=torch.float32)
    y1 = ws[:B * N * 512].view(B, N, 512)
    y2 = ws[B * N * 512:].view(B, N, 256)
    logits = torch.full((B, N, 2), FILL, dtype=torch.float32)
    merged = torch.full((B, N + 1), FILL, dtype=torch.float32)
    for h, fd in enumerate(folded):
        src = feat_index[h - 1] if mutant == 'head h reads the features of head h-1' else feat_index[h]
        x = feats[src]
        w1 = f(fd.w1)
        if mutant == 'last 32 features dropped':
            x, w1 = x[:, :-32], w1[:, :-32]
        a = torch.relu(x @ w1.t() + f(fd.b1))
        if mutant == 'rows >= 128 repeat row - 128' and B > 128:
            a[128:] = a[:B - 128].clone()
        y1[:, h if mutant == 'y1 columns in head order' else rk[h]] = a
    for h, fd in enumerate(folded):
        w = folded[(h + 1) % N] if mutant == "head h+1's second-layer weights on head h" else fd
        a = y1[:, rk[h]] @ f(w.w2).t() + f(w.b2)
        y2[:, h] = a if mutant == 'ReLU missing after layer 2' else torch.relu(a)
    for h, fd in enumerate(folded):
        z = y2[:, h] @ f(fd.w3).t() + f(fd.b3)
        logits[:, h] = z.flip(1) if mutant == '[Real, Synthetic] swapped' else z
    merged[:, :N] = logits[:, :, 0 if mutant == 'merged synthetic columns from column 0' else 1]
    real = logits[:, :, 0].sum(dim=1)
    merged[:, N] = {'real mean over N + 1': real / (N + 1), 'real sum, not mean': real}.get(mutant, real / N)
    if mutant == 'last B % 4 rows unwritten' and B % 4:
        logits[B - B % 4:] = FILL
        merged[B - B % 4:] = FILL
    return ws, logits, merged


MUTANTS = [
    'eps dropped',
    'eps outside the square root',
    'Linear bias not scaled',
    'ReLU missing after layer 2',
    '[Real, Synthetic] swapped',
    'merged synthetic columns from column 0',
    'real mean over N + 1',
    'real sum, not mean',
    'head h reads the features of head h-1',
    'y1 columns in head order',
    "head h+1's second-layer weights on head h",
    'last 32 features dropped',
    'rows >= 128 repeat row - 128',
    'last B % 4 rows unwritten',
]
