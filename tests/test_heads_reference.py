"""CPU: the float64 heads reference of tests/heads_ref.py is itself right, and
the comparison it feeds is sharp.

Reference checks: its chain is oracle.resnet.make_head x N under
ModularMultiHeadClassifier in float64 eval mode -- to 1e-12 relative with the
exact fold, and stage by stage within 2 u S (S = sum |x| |w'| + |b'|) with the
fold rounded to fp32 as the plan stores it.

Sharpness: a CPU fp32 stand-in of the three stages, writing the device's
workspace layout, goes through the SAME comparison function as the GPU run, on
every input set the GPU test uses.  The clean stand-in must pass all of them;
each mutant (a plausible kernel or plan bug) must be rejected on at least one.
"""
import pytest
import torch
import torch.nn as nn

import heads_ref as R

F64 = torch.float64


class _Sub(nn.Module):
    """A sub-model that is only its head, reading feature group `idx`."""

    def __init__(self, head, idx):
        super().__init__()
        self.head, self.idx = head, idx

    def forward(self, feats):
        x = feats[self.idx]
        return self.head(x.view(*x.shape, 1, 1))


def _oracle_heads(sds, feat_dim):
    from oracle.resnet import make_head
    heads = []
    for sd in sds:
        m = make_head(feat_dim).double().eval()
        m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
        for k in R.HEAD_KEYS:
            assert torch.equal(m.state_dict()[k], sd[k].double()), k
        heads.append(m)
    return heads


@pytest.fixture(scope='module')
def inputs():
    """case name -> (case, head_sds, feats): every input set of the GPU test."""
    out = {}
    for c in R.CASES:
        out[c.name] = (c,) + R.make_case(c)
    sds, big = R.make_large()
    out[R.LARGE.name] = (R.LARGE._replace(B=len(R.LARGE_ROWS)), sds, [big[R.LARGE_ROWS].clone()])
    return out


# ------------------------------------------------------------ the reference --
def test_exact_chain_is_the_oracle_model():
    """Tame statistics (the 1e-12 is relative to the largest logit; with the
    adversarial small-variance channels the float64 chain itself amplifies its
    roundings by the scale of those channels)."""
    from oracle.resnet import ModularMultiHeadClassifier, per_head_logits
    gen = torch.Generator().manual_seed(31)
    fi = [0, 1, 2, 0]
    sds = [R.random_head(gen, 512) for _ in fi]
    for sd in sds:
        for k in ('3.running_var', '7.running_var'):
            sd[k] = sd[k].clamp(min=0.25)
    feats = [torch.randn(9, 512, generator=gen) for _ in range(3)]
    model = ModularMultiHeadClassifier([_Sub(m, f) for m, f in zip(_oracle_heads(sds, 512), fi)]).eval()
    with torch.no_grad():
        want_merged = model([f.double() for f in feats])
        want_logits = per_head_logits(model, [f.double() for f in feats])
    _, _, logits, merged = R.chain([R.fold(sd, rounded=False) for sd in sds], feats, fi)
    assert (logits - want_logits).abs().max().item() <= 1e-12 * want_logits.abs().max().item()
    assert (merged - want_merged).abs().max().item() <= 1e-12 * want_merged.abs().max().item()
    assert merged.shape == (9, 5)


@pytest.mark.parametrize('feat_dim', [64, 512, 2048])
def test_stages_are_the_oracle_layers(feat_dim):
    """Stage by stage on one input, adversarial statistics: the exact fold to
    1e-12 S, the fp32-rounded fold within 2 u S."""
    gen = torch.Generator().manual_seed(32 + feat_dim)
    sd = R.random_head(gen, feat_dim)
    assert sd['3.running_var'].min() < 1e-3 and (sd['3.weight'] == 0).any() and (sd['3.weight'] < 0).any()
    (m,) = _oracle_heads([sd], feat_dim)
    x = R.random_features(gen, 7, feat_dim).double()
    a = torch.relu(torch.randn(7, 512, generator=gen)).double()
    b = torch.relu(torch.randn(7, 256, generator=gen)).double()
    exact, rounded = R.fold(sd, rounded=False), R.fold(sd)
    with torch.no_grad():
        want = [m[2:5](x), m[6:9](a), m[10](b)]
    for s, (inp, relu) in enumerate(((x, True), (a, True), (b, False))):
        for fd, tol in ((exact, 1e-12), (rounded, 2 * R.U)):
            w, bias = fd[2 * s], fd[2 * s + 1]
            _, ref, bar = R.stage(inp, w, bias, relu)
            S = bar / ((inp.shape[1] + 8) * R.U)
            assert torch.all((ref - want[s]).abs() <= tol * S + 1e-300), (s, tol)
    assert (want[0] == 0).any() and (want[0] > 0).any()


def test_layout_and_path():
    assert R.rank([0, 1, 2, 0]) == [0, 2, 3, 1]
    assert R.rank([0, 1, 0, 1]) == [0, 2, 1, 3]
    assert R.rank([1, 0]) == [1, 0]
    assert R.rank([0, 2]) == [0, 1] and R.rank([0, 0, 1]) == [0, 1, 2]
    regular = [R.is_regular(p[1]) for p in R.PLANS]
    assert regular == [True, True, True, True, True, False, False, False, True, True, True]
    # the row range of the two GEMM operands (include/sad.h)
    assert R.row_range(6, 512) == 174592 and R.row_range(64, 512) == 16384
    assert R.row_range(1, 2048) == 261632
    assert R.LARGE_B % 4 == 1 and R.LARGE_B > R.row_range(64, 512)


def test_inputs_are_the_ones_asked_for(inputs):
    for name, (c, sds, feats) in inputs.items():
        assert [f is None for f in feats] == [i not in c.feat_index for i in range(c.n_feat)]
        for f in feats:
            if f is not None:
                assert f.shape == (c.B, c.feat_dim) and (f < 0).any()
                assert c.B < 2 or (f[1] == 0).all()
                assert c.B < 3 or f[2].abs().max() > 1e4
        assert not torch.equal(sds[0]['6.weight'], sds[-1]['6.weight']) or c.n_heads == 1
        v, g = sds[0]['3.running_var'], sds[0]['3.weight']
        assert v[::16].max() <= 1e-3 and v[::16].min() >= 1e-6 and (g[::7] == 0).all()
        others = torch.ones(512, dtype=torch.bool)
        others[::16] = False
        assert v[others].min() >= 0.25 and v[others].max() <= 4.0 and (g < 0).any() and (g > 0).any()


# ---------------------------------------------------------------- sharpness --
def test_clean_standin_passes_every_input_set(inputs):
    worst = {}
    for name, (c, sds, feats) in inputs.items():
        folded = [R.fold(sd) for sd in sds]
        r = R.compare(folded, feats, c.feat_index, *R.standin(sds, feats, c.feat_index))
        assert R.passes(r), (name, r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('clean stand-in, worst |d|/bar: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_mutant_is_rejected(inputs, mutant):
    worst, rejected = {}, []
    for name, (c, sds, feats) in inputs.items():
        if name == R.LARGE.name:
            continue                                   # (64 heads: the smaller sets decide)
        folded = [R.fold(sd) for sd in sds]
        r = R.compare(folded, feats, c.feat_index, *R.standin(sds, feats, c.feat_index, mutant))
        worst[name] = max(r.values())
        if not R.passes(r):
            rejected.append(name)
    top = max(worst, key=worst.get)
    print(f'{mutant}: rejected on {len(rejected)}/{len(worst)} input sets, worst |d|/bar {worst[top]:.3g} ({top})')
    assert rejected, worst
