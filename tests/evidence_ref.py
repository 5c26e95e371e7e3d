"""Float64 reference of the evidence-map contract (include/sad.h "evidence",
DESIGN.md 5e), with a-priori rounding bars.  No GPU work here:
tests/test_evidence_reference.py proves this file against torch autograd on the
CPU; the GPU tests compare sad_heads_grad_run, sad_evidence_run and
Engine.explain with it.

The contract, for window b and head h reading backbone j = feat_index[h], with
A = backbone j's stored layer4 activation [HW, C], f = its pooled features, the
head's eval-mode forward  y1 = relu(W1 f + b1), y2 = relu(W2 y1 + b2),
z = W3 y2 + b3  (W1, W2 BN-folded and rounded to fp32 as the plan holds them):
  m1 = (y1 > 0), m2 = (y2 > 0)               a unit at exactly 0 is off
  g  = W1^T (m1 * (W2^T (m2 * W3[cls])))     = d z[cls] / d f, fp32
  E[p] = (1 / HW) sum_c g[c] A[p, c]         signed, unnormalised
  sum_p E[p] = g . f   and   z[cls] = g . f + beta,
  beta = b3[cls] + (m2 * W3[cls]) . b2 + (m1 * (W2^T (m2 * W3[cls]))) . b1.

Bars, u = 2^-24, written down before any run:
  evidence   (C + 4) u sum_c |g_c a_c| / HW per element: the only rounding is
             the fp32 accumulation of C exact-operand products (any order) and
             the final division;
  gradient   two fp32 GEMMs, K = 256 then 512, each (K + 2) u sum |terms| for
             any summation order.  The first GEMM's error e1 passes the mask and
             the second GEMM:  e1 = 258 u (|u2| |W2|) * m1,
             bar = 514 u ((|t1| + e1) |W1|) + e1 |W1|,
             u2 = m2 * W3[cls], t1 = (u2 W2) * m1.  The masks are GIVEN (the
             device's own y1 / y2), so no mask can differ.
"""
import numpy as np
import torch

from heads_ref import F64, U, fold, split_workspace, worst_ratio  # noqa: F401  (re-exported for the tests)

HW = 256


def masks(y1, y2, at_zero_on=False):
    """ReLU gradient masks of stored activations (at_zero_on: the '>= 0' mutant)."""
    return (y1 >= 0, y2 >= 0) if at_zero_on else (y1 > 0, y2 > 0)


def _w2(fd, transposed_w2):
    # the mutant: W2's memory read with the other index order
    return fd.w2.t().contiguous().view(256, 512) if transposed_w2 else fd.w2


def head_grad(fd, m1, m2, cls, transposed_w2=False):
    """fd: heads_ref.Folded (float64 holding fp32 values); m1 [B,512], m2
    [B,256] bool -> (g [B, feat_dim], bar [B, feat_dim]) float64."""
    w2 = _w2(fd, transposed_w2)
    u2 = m2.to(F64) * fd.w3[cls]
    t1 = (u2 @ w2) * m1.to(F64)
    g = t1 @ fd.w1
    e1 = (256 + 2) * U * (u2.abs() @ w2.abs()) * m1.to(F64)
    bar = (512 + 2) * U * ((t1.abs() + e1) @ fd.w1.abs()) + e1 @ fd.w1.abs()
    return g, bar


def beta(fd, m1, m2, cls):
    """z[cls] - g . f for the given masks: [B] float64."""
    u2 = m2.to(F64) * fd.w3[cls]
    t1 = (u2 @ fd.w2) * m1.to(F64)
    return fd.b3[cls] + u2 @ fd.b2 + t1 @ fd.b1


def evidence(A, g, scale=None):
    """A [B, HW, C] float64 (the stored values, decoded exactly), g [B, C]
    float64 -> (E [B, HW], bar [B, HW]).  scale: 1 / HW unless given (the
    'missing 1 / HW' mutant passes 1)."""
    hw, C = A.shape[1], A.shape[2]
    s = 1.0 / hw if scale is None else scale
    E = torch.einsum('bpc,bc->bp', A, g) * s
    bar = (C + 4) * U * torch.einsum('bpc,bc->bp', A.abs(), g.abs()) / hw
    return E, bar


def decode(l4, dtype):
    """A plan's activation tensor [B, H, W, C'] (bf16x3: the split layout, 2C
    bf16 per pixel as [hi 32 | lo 32] per 32 channels) -> float64 [B, H W, C],
    exactly the stored values (split: hi + lo)."""
    t = l4.detach().cpu()
    B = t.shape[0]
    if dtype == 'bf16x3':
        C2 = t.shape[-1]
        g = t.reshape(B, -1, C2 // 64, 2, 32).to(F64)
        return (g[..., 0, :] + g[..., 1, :]).reshape(B, -1, C2 // 2)
    return t.reshape(B, -1, t.shape[-1]).to(F64)


def timeline(E, timestamps, window_sec):
    """E [W, N, 16, 16], window starts [W] (s) -> [N, bins] float64: bin width
    window / 16; a bin is the mean over every (window, column) whose centre
    falls in it of the column's sum over the rows; nan where none does."""
    E = np.asarray(E, dtype=np.float64)
    W, N = E.shape[:2]
    width = window_sec / 16.0
    entries = {}
    for w in range(W):
        for x in range(16):
            centre = float(timestamps[w]) + (x + 0.5) * width
            k = int(np.floor(centre / width + 1e-9))
            entries.setdefault(k, []).append(E[w, :, :, x].sum(axis=1))
    bins = max(entries) + 1 if entries else 0
    out = np.full((N, bins), np.nan)
    for k, v in entries.items():
        out[:, k] = np.mean(np.stack(v), axis=0)
    return out
