"""GPU: sad_heads_grad_run against tests/evidence_ref.py, fed the device's OWN
y1 / y2 read from the merge run's workspace -- so no ReLU mask can differ
between device and reference, and the bar covers the two GEMMs' arithmetic
alone.  N in {1, 2, 6}, feat_dim in {512, 2048}, grouped and per-head second
layer, B in {1, 5, 127, 129} (either side of the 128-row GEMM tile), cls 0 / 1.

The heads carry zero and negative BN gammas (heads_ref.random_head) and hidden
units forced to exactly 0:
  layer 1, unit 5   reads feature columns 0..7 only, which are zero, with zero
                    bias / BN shift: y1[5] = relu(0) = 0 while W1[5, :8] != 0;
  layer 2, unit 3   reads y1 unit 5 only (weight 1, zero bias / BN shift):
                    y2[3] = relu(1 * 0) = 0.
A mask taken at >= 0 would switch both on and put gradient on feature columns
0..7 (the test asserts that the reference itself moves under that mutation).

Bar, a priori (evidence_ref.head_grad): (K + 2) 2^-24 sum |terms| through the
two GEMMs, K = 256 then 512, on the plan's rounded folded weights.
`pytest -s` prints the worst ratio per case (profiles/evidence_tests_ratios.txt
is one such run).
"""
import pytest
import torch

import evidence_ref as E
import heads_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (N, feat_index, n_feat): grouped second layer (regular) and per-head (irregular)
PLANS = [(1, [0], 1), (2, [0, 0], 1), (2, [1, 0], 2), (6, [0] * 6, 1), (6, [0, 1, 0, 1, 2, 0], 3)]
CASES = [(n, fi, nf, d, B) for (n, fi, nf) in PLANS for d in (512, 2048) for B in (1, 5, 127, 129)
         if d == 512 or B in (5, 129)]


def _head(gen, D):
    sd = R.random_head(gen, D)
    sd['2.weight'][5] = 0.0
    sd['2.weight'][5, :8] = 1.0
    for k, v in (('2.bias', 0.0), ('3.running_mean', 0.0), ('3.bias', 0.0), ('3.weight', 1.5)):
        sd[k][5] = v
    sd['6.weight'][3] = 0.0
    sd['6.weight'][3, 5] = 1.0
    for k, v in (('6.bias', 0.0), ('7.running_mean', 0.0), ('7.bias', 0.0), ('7.weight', 1.5)):
        sd[k][3] = v
    return sd


@pytest.mark.parametrize('N, feat_index, n_feat, D, B', CASES, ids=lambda v: str(v).replace(' ', ''))
def test_heads_grad_against_float64(N, feat_index, n_feat, D, B):
    from sad.engine import Heads
    gen = torch.Generator().manual_seed(N * 1000 + D + B + len(set(feat_index)))
    sds = [_head(gen, D) for _ in range(N)]
    folded = [R.fold(sd) for sd in sds]
    feats = [R.random_features(gen, B, D) for _ in range(n_feat)]
    for f in feats:
        f[:, :8] = 0.0
    heads = Heads(sds, feat_index, n_feat, DEV, feat_dim=D)
    assert bool(R.is_regular(feat_index)) == (feat_index == sorted(feat_index))
    dev = [f.to(DEV) for f in feats]
    heads(dev)
    torch.cuda.synchronize()
    ws = heads._ws.view(torch.float32).cpu()
    y1, y2 = R.split_workspace(ws, B, feat_index)
    assert (y1[:, :, 5] == 0).all() and (y2[:, :, 3] == 0).all()
    worst, moved = 0.0, False
    for cls in (0, 1):
        g = heads.grad(B, cls)
        torch.cuda.synchronize()
        assert g.shape == (N, B, D)
        g = g.cpu()
        for h, fd in enumerate(folded):
            m1, m2 = E.masks(y1[:, h], y2[:, h])
            ref, bar = E.head_grad(fd, m1, m2, cls)
            worst = max(worst, E.worst_ratio(g[h], ref, bar))
            bad, _ = E.head_grad(fd, *E.masks(y1[:, h], y2[:, h], at_zero_on=True), cls)
            moved = moved or (bad - ref).abs().max().item() > 10 * bar.max().item()
        # the workspace is only read: a second call gives the same bits
        again = heads.grad(B, cls).cpu()
        assert torch.equal(again.view(torch.int32), g.view(torch.int32))
    print(f'RATIO heads_grad N{N}-{"".join(map(str, feat_index))}-d{D}-B{B}: {worst:.3g}')
    assert worst <= 1.0
    assert moved, 'the exact-zero units would not show a mask taken at >= 0'
    ws2 = heads._ws.view(torch.float32).cpu()
    assert torch.equal(ws2.view(torch.int32), ws.view(torch.int32))


def test_row_does_not_depend_on_its_position():
    """Row 3 of a 5-row batch, run alone, gives the same gradient bits."""
    from sad.engine import Heads
    gen = torch.Generator().manual_seed(5)
    sds = [_head(gen, 512) for _ in range(2)]
    x = R.random_features(gen, 5, 512).to(DEV)
    heads = Heads(sds, [0, 0], 1, DEV)
    heads([x])
    g5 = heads.grad(5, 1).cpu()
    heads([x[3:4].contiguous()])
    g1 = heads.grad(1, 1).cpu()
    assert torch.equal(g1[:, 0].view(torch.int32), g5[:, 3].view(torch.int32))


def test_grad_needs_the_forward_of_the_same_rows():
    from sad.engine import Heads
    gen = torch.Generator().manual_seed(6)
    heads = Heads([_head(gen, 512)], [0], 1, DEV)
    with pytest.raises(RuntimeError, match='must follow a forward'):
        heads.grad(2, 1)
    heads([R.random_features(gen, 2, 512).to(DEV)])
    with pytest.raises(RuntimeError, match='must follow a forward'):
        heads.grad(3, 1)
    with pytest.raises(ValueError, match='cls'):
        heads.grad(2, 2)
    assert heads.grad(2, 0).shape == (1, 2, 512)
