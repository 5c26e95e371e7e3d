"""GPU: Engine.explain end to end.  B = 3 golden maps with micro-batch 2 (a
chunk seam and a ragged tail), N = 2 heads: resnet18 in all four precisions
with two DISTINCT backbones (one map per evidence pass, A and g must come from
the right backbone), resnet34 / resnet50 in bf16 and bf16x3 with one shared
backbone (two maps per pass; BN statistics calibrated as in
test_gpu_deep_resnet).

Checks, per chunk, on the device's own stored A, f, g, y1, y2:
  * evidence == evidence_ref.evidence(A, g) within its bar
    (C + 4) u sum_c |g_c a_c| / HW;
  * sum_yx E == g . f (f the keep path's pooled features) within that bar summed
    over the pixels plus the average pool's own rounding of f,
    (C + 4 + HW + 4) u sum_c |g_c| sum_p |a_pc| / HW: A and g from different
    chunks or backbones miss it by orders of magnitude;
  * the returned Synthetic logit == g . f + beta(device masks), within the
    heads' stage bars (heads_ref.stage: (K + 8) u (sum |x| |w| + |b|))
    propagated through the masked layers plus the gradient's own bar times |f|;
  * micro-batch 2 and micro-batch 3 give the same bits;
  * margin == synthetic - real exactly;
  * the two sub-models' maps differ.
How far the keep path's logits sit from forward_maps' is MEASURED and printed
per precision (`pytest -s`; profiles/evidence_tests_ratios.txt) and bounded by
the precision's existing logit tolerance against fp32: 1e-3 for fp32 and bf16x3
(the parity bar), 0.15 for bf16 and 0.15 / 8 for fp16 (the accuracy gates of
test_gpu_accuracy_gate.py and test_gpu_fp16_plan.py).
"""
import os

import pytest
import torch

import evidence_ref as E
import heads_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = R.U
LOGIT_TOL = {'fp32': 1e-3, 'bf16x3': 1e-3, 'bf16': 0.15, 'fp16': 0.15 / 8}
CONFIGS = [('resnet18', d) for d in ('fp32', 'bf16x3', 'bf16', 'fp16')] + \
          [(a, d) for a in ('resnet34', 'resnet50') for d in ('bf16', 'bf16x3')]

_SD = {}


def _state(arch, maps):
    if arch not in _SD:
        from sad import weights as sw
        if arch == 'resnet18':
            _SD[arch] = sw.merged_state_dict(0, 2, True,
                                             bn_stats=sw.load_bn_stats(os.path.join(GOLDEN, 'bn_stats_n6.npz')))
        else:
            from test_gpu_deep_resnet import _calibrated
            _SD[arch] = _calibrated(arch, maps)[0]
    return _SD[arch]


def _head_sds(sd, n):
    return [{k: sd[f'sub_models.{i}.head.{k}'].float() for k in R.HEAD_KEYS} for i in range(n)]


@pytest.mark.parametrize('arch, dtype', CONFIGS)
def test_explain(arch, dtype, golden_frontend):
    from sad.engine import Engine
    maps = torch.from_numpy(golden_frontend['std_map'][:3]).contiguous()
    sd = _state(arch, maps)
    eng = Engine(sd, DEV, dtype=dtype, micro_batch=2)
    N, D = 2, eng.num_features
    fi = eng.grouping.feat_index
    assert eng.n_heads == N and len(eng.backbones) == (2 if arch == 'resnet18' else 1)
    x = maps.to(DEV)
    det = []
    merged, ev = eng.explain(x, 'maps', 'synthetic', details=det)
    torch.cuda.synchronize()
    assert merged.shape == (3, N + 1) and ev.shape == (3, N, 16, 16) and ev.dtype == torch.float32
    assert [d[0] for d in det] == [slice(0, 2), slice(2, 3)]
    merged, ev = merged.cpu(), ev.cpu()
    assert torch.isfinite(ev).all() and torch.isfinite(merged).all()
    folded = [R.fold(h) for h in _head_sds(sd, N)]
    r_ev = r_sum = r_logit = 0.0
    for rows, feats, l4s, gs, y in det:
        n = rows.stop - rows.start
        y1, y2 = R.split_workspace(y.cpu(), n, fi)
        for h in range(N):
            j = fi[h]
            A = E.decode(l4s[j], dtype)                          # [n, 256, D]
            f = feats[j].cpu().double()
            g = gs[0][h].cpu().double()
            assert A.shape == (n, 256, D)
            got = ev[rows, h].reshape(n, 256)
            ref, bar = E.evidence(A, g)
            r_ev = max(r_ev, E.worst_ratio(got, ref, bar))
            gf = (g * f).sum(dim=1)
            sbar = (D + 4 + 256 + 4) * U * torch.einsum('bpc,bc->b', A.abs(), g.abs()) / 256
            r_sum = max(r_sum, E.worst_ratio(got.double().sum(dim=1), gf, sbar))
            # logit = g . f + beta under the device's masks
            fd = folded[h]
            m1, m2 = E.masks(y1[:, h], y2[:, h])
            gref, gbar = E.head_grad(fd, m1, m2, 1)
            _, _, b1 = R.stage(f, fd.w1, fd.b1)
            _, _, b2 = R.stage(y1[:, h].double(), fd.w2, fd.b2)
            _, _, b3 = R.stage(y2[:, h].double(), fd.w3, fd.b3, relu=False)
            u2 = m2.double() * fd.w3[1].abs()
            lbar = b3[:, 1] + (u2 * (b2 + (b1 * m1.double()) @ fd.w2.abs().t())).sum(dim=1) + (gbar * f.abs()).sum(dim=1)
            want = gf + E.beta(fd, m1, m2, 1)
            r_logit = max(r_logit, E.worst_ratio(merged[rows, h], want, lbar))
            assert E.worst_ratio(gs[0][h].cpu(), gref, gbar) <= 1.0
    print(f'RATIO explain {arch} {dtype}: evidence {r_ev:.3g}, sum = g.f {r_sum:.3g}, logit = g.f + beta {r_logit:.3g}')
    assert r_ev <= 1.0 and r_sum <= 1.0 and r_logit <= 1.0
    assert not torch.equal(ev[:, 0], ev[:, 1])

    # the keep path against the ordinary forward: measured, bounded by the precision's logit tolerance
    _, ordinary = eng.forward_maps(x)
    torch.cuda.synchronize()
    d_keep = (ordinary.cpu() - merged).abs().max().item()
    print(f'RATIO explain {arch} {dtype}: max|dlogit| keep path vs forward_maps {d_keep:.3e} '
          f'(tolerance {LOGIT_TOL[dtype]:.3g})')
    assert d_keep <= LOGIT_TOL[dtype]

    # margin = synthetic - real, exactly; the merged logits do not depend on the target
    m_r, ev_r = eng.explain(x, 'maps', 'real')
    m_m, ev_m = eng.explain(x, 'maps', 'margin')
    torch.cuda.synchronize()
    assert torch.equal(ev_m.cpu(), ev - ev_r.cpu())
    assert torch.equal(m_r.cpu(), merged) and torch.equal(m_m.cpu(), merged)
    assert not torch.equal(ev_r.cpu(), ev)

    # micro-batch 3 (one chunk) gives the bits of micro-batch 2 (two chunks)
    for bb in eng.backbones:
        bb.micro_batch = 3
    det3 = []
    m3, ev3 = eng.explain(x, 'maps', 'synthetic', details=det3)
    torch.cuda.synchronize()
    assert len(det3) == 1
    assert torch.equal(ev3.cpu().view(torch.int32), ev.view(torch.int32))
    assert torch.equal(m3.cpu().view(torch.int32), merged.view(torch.int32))


def test_explain_refuses_unknown_target(golden_frontend):
    from sad.engine import Engine
    maps = torch.from_numpy(golden_frontend['std_map'][:1]).contiguous()
    eng = Engine(_state('resnet18', maps), DEV, dtype='bf16', micro_batch=2)
    with pytest.raises(ValueError, match='target'):
        eng.explain(maps.to(DEV), 'maps', 'both')
