"""GPU: sad_evidence_run alone, against float64 of the exact stored values
(tests/evidence_ref.py).  C in {64, 512, 2048}, hw in {1, 256}, n_maps in
{1, 2, 6, 16}, the four activation layouts; B = 3 and B = 1 inside every case.

Inputs per case:
  random    random A, a DISTINCT random g per map (a map mix-up shows), large
            values (x 1e3) in A and g on channel 0, channel C - 1 and on either
            side of every 32-channel boundary;
  one-hot   g[m][b] = 1 at one channel, 0 elsewhere: the output must equal
            A[b, :, c] / hw EXACTLY.  The channels walk the seams: the lane
            seams at 8 and 16, the hi / lo seam at 32, the chunk seams at 256
            and 512, the last channel;
  zero      all-zero g must give exact zeros.
Bar, a priori (evidence_ref): the only rounding is the fp32 accumulation, so
|err| <= (C + 4) 2^-24 sum_c |g_c a_c| / hw per element.  The output of B = 3
equals the three B = 1 runs bit for bit.  The output sits between guard
regions that must stay intact.
"""
import ctypes

import pytest
import torch

import evidence_ref as E

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 1024      # floats


def _stored(x, dtype):
    """fp32 [B, hw, C] -> the layout tensor [B, hw, 1, C'] a plan would store."""
    from sad.engine import to_split
    t = {'bf16': lambda: x.to(torch.bfloat16), 'fp16': lambda: x.to(torch.float16), 'fp32': lambda: x.clone(),
         'bf16x3': lambda: to_split(x)}[dtype]()
    return t.unsqueeze(2).contiguous()


def _run(l4, dtype, g):
    """l4: stored layout (host), g: list of [B, C] fp32 (host) -> out [B, n_maps, hw] (host), guards checked."""
    from sad import _lib as L
    B, hw = l4.shape[0], l4.shape[1]
    C = g[0].shape[1]
    n = B * len(g) * hw
    raw = torch.full((GUARD + n + GUARD,), float('nan'), device=DEV)
    dl4 = l4.to(DEV)
    dg = [t.contiguous().to(DEV) for t in g]
    gp = (ctypes.c_void_p * len(g))(*[t.data_ptr() for t in dg])
    with torch.cuda.device(DEV):
        L.call('sad_evidence_run', L.ptr(dl4), L.DTYPES[dtype], B, hw, C, gp, len(g), raw.data_ptr() + 4 * GUARD,
               L.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    host = raw.cpu()
    assert torch.isnan(host[:GUARD]).all() and torch.isnan(host[GUARD + n:]).all(), 'guard region written'
    return host[GUARD:GUARD + n].view(B, len(g), hw)


def _boundary_channels(C):
    s = {0, C - 1}
    for k in range(32, C, 32):
        s |= {k - 1, k}
    return sorted(s)


def _seam_channels(C):
    want = [0, 7, 8, 15, 16, 31, 32, 33, 63, 255, 256, 511, 512, C - 33, C - 32, C - 1]
    return sorted({c for c in want if 0 <= c < C})


CASES = [(d, C, hw, nm) for d in ('bf16', 'fp16', 'fp32', 'bf16x3') for C in (64, 512, 2048) for hw in (1, 256)
         for nm in (1, 2, 6, 16)]


@pytest.mark.parametrize('dtype, C, hw, n_maps', CASES, ids=lambda v: str(v))
def test_evidence_kernel(dtype, C, hw, n_maps):
    gen = torch.Generator().manual_seed(C * 31 + hw * 7 + n_maps)
    B = 3
    # ---- random, distinct g per map, large values at the boundaries
    x = torch.randn(B, hw, C, generator=gen)
    g = [torch.randn(B, C, generator=gen) * (m + 1) for m in range(n_maps)]
    bc = _boundary_channels(C)
    x[:, :, bc] *= 1e3
    for t in g:
        t[:, bc] *= 1e3
    l4 = _stored(x, dtype)
    A = E.decode(l4, dtype)
    got = _run(l4, dtype, g)
    worst = 0.0
    for m in range(n_maps):
        ref, bar = E.evidence(A, g[m].double())
        worst = max(worst, E.worst_ratio(got[:, m], ref, bar))
    print(f'RATIO evidence {dtype} C{C} hw{hw} maps{n_maps}: {worst:.3g}')
    assert worst <= 1.0
    if n_maps > 1:
        assert not torch.equal(got[:, 0], got[:, 1])
    # ---- B = 3 is the three B = 1 runs, bit for bit
    for b in range(B):
        one = _run(l4[b:b + 1], dtype, [t[b:b + 1] for t in g])
        assert torch.equal(one[0].view(torch.int32), got[b].view(torch.int32)), b
    # ---- all-zero g: exact zeros
    zero = _run(l4[:1], dtype, [torch.zeros(1, C) for _ in range(n_maps)])
    assert (zero == 0).all()
    # ---- one-hot g on the seams: exactly A[b, :, c] / hw
    seams = _seam_channels(C)
    S = len(seams)
    xs = torch.randn(S, hw, C, generator=gen)
    ls = _stored(xs, dtype)
    As = E.decode(ls, dtype)
    gs, ch = [], []
    for m in range(n_maps):
        t = torch.zeros(S, C)
        c = [seams[(b + m) % S] for b in range(S)]
        t[torch.arange(S), c] = 1.0
        gs.append(t)
        ch.append(c)
    hot = _run(ls, dtype, gs)
    for m in range(n_maps):
        want = torch.stack([As[b, :, ch[m][b]] for b in range(S)]) / hw
        assert torch.equal(hot[:, m].double(), want), (m, ch[m])
