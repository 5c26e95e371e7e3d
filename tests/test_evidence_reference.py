"""CPU: the float64 evidence contract of tests/evidence_ref.py is right, and
sharp.

Right: a reference-structured eval head (oracle.resnet.make_head: average
pool, Linear, BatchNorm1d, ReLU, Dropout, ...) in float64 on an activation A;
torch autograd of logit[cls] with respect to A must be g / HW broadcast over
the pixels, g the reference's gradient from the EXACT fold and the head's own
masks -- so the evidence sum_c (dlogit/dA)[p, c] A[p, c] is the reference's
E[p].  Also sum_p E = g . f and logit = g . f + beta.

Sharp: four mutated references (mask at >= 0, W3 row of the other class, a
missing 1 / HW, W2 read transposed) must each miss the autograd result.

The timeline on hand-made inputs, hops of 1.0 and 0.15 windows.
"""
import numpy as np
import pytest
import torch

import evidence_ref as E
import heads_ref as R

F64 = torch.float64
HW = 256


def _head(sd, feat_dim):
    from oracle.resnet import make_head
    m = make_head(feat_dim).double().eval()
    m.load_state_dict({k: v.double() for k, v in sd.items()}, strict=False)
    return m


@pytest.fixture(scope='module', params=[512, 2048])
def case(request):
    """One head, B = 4 windows, and a hidden unit at exactly 0 that still has
    weights: unit 5 reads channels 0..7 only, which are zero in A, with zero
    bias, BN mean and BN beta -- y1[5] = relu(0) = 0 while W1[5, :8] != 0, so a
    mask taken at >= 0 puts a gradient on channels 0..7 that autograd does not."""
    D = request.param
    gen = torch.Generator().manual_seed(77 + D)
    sd = R.random_head(gen, D)
    sd['2.weight'][5] = 0.0
    sd['2.weight'][5, :8] = 1.0
    sd['2.bias'][5] = 0.0
    sd['3.running_mean'][5] = 0.0
    sd['3.bias'][5] = 0.0
    sd['3.weight'][5] = 1.5
    A = torch.relu(torch.randn(4, 16, 16, D, generator=gen)).double()          # NHWC, post-ReLU like layer4
    A[..., :8] = 0.0
    model = _head(sd, D)
    fd = R.fold(sd, rounded=False)
    x = A.permute(0, 3, 1, 2).contiguous().requires_grad_(True)                # the reference's NCHW
    z = model(x)
    grads = [torch.autograd.grad(z[:, cls].sum(), x, retain_graph=True)[0].permute(0, 2, 3, 1) for cls in (0, 1)]
    f = A.mean(dim=(1, 2))
    y1 = torch.relu(f @ fd.w1.t() + fd.b1)
    y2 = torch.relu(y1 @ fd.w2.t() + fd.b2)
    assert (y1[:, 5] == 0).all() and (y1 > 0).any() and (y2 == 0).any()
    return dict(D=D, A=A, fd=fd, z=z.detach(), grads=grads, f=f, y1=y1, y2=y2)


def _rel(a, b):
    return (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize('cls', [0, 1])
def test_gradient_is_autograd(case, cls):
    m1, m2 = E.masks(case['y1'], case['y2'])
    g, bar = E.head_grad(case['fd'], m1, m2, cls)
    want = case['grads'][cls]                                                  # [B,16,16,D]
    assert _rel((g / HW)[:, None, None, :].expand_as(want), want) <= 1e-12
    assert (want[:, 0, 0] == want[:, 7, 3]).all()                              # the same at every pixel
    assert (bar >= 0).all() and bar.max() > 0


@pytest.mark.parametrize('cls', [0, 1])
def test_evidence_sums_and_logit(case, cls):
    m1, m2 = E.masks(case['y1'], case['y2'])
    g, _ = E.head_grad(case['fd'], m1, m2, cls)
    A = case['A'].reshape(4, HW, case['D'])
    ev, bar = E.evidence(A, g)
    want = (case['grads'][cls].reshape(4, HW, -1) * A).sum(dim=2)              # sum_c dz/dA * A
    assert _rel(ev, want) <= 1e-12
    gf = (g * case['f']).sum(dim=1)
    assert _rel(ev.sum(dim=1), gf) <= 1e-12
    assert _rel(gf + E.beta(case['fd'], m1, m2, cls), case['z'][:, cls]) <= 1e-12
    assert (bar > 0).all()


MUTANTS = ['mask at >= 0', 'W3 row of the other class', 'missing 1 / HW', 'W2 transposed']


@pytest.mark.parametrize('mutant', MUTANTS)
def test_mutated_reference_fails(case, mutant):
    cls = 1
    m1, m2 = E.masks(case['y1'], case['y2'], at_zero_on=mutant == 'mask at >= 0')
    g, _ = E.head_grad(case['fd'], m1, m2, 1 - cls if mutant == 'W3 row of the other class' else cls,
                       transposed_w2=mutant == 'W2 transposed')
    A = case['A'].reshape(4, HW, case['D'])
    ev, _ = E.evidence(A, g, scale=1.0 if mutant == 'missing 1 / HW' else None)
    want = (case['grads'][cls].reshape(4, HW, -1) * A).sum(dim=2)
    gw = case['grads'][cls][:, 0, 0]                                           # autograd's g / HW
    err = max(_rel(ev, want), _rel(g / (1.0 if mutant == 'missing 1 / HW' else HW), gw))
    print(f'{mutant}: relative error {err:.3g}')
    assert err > 1e-6, mutant


def test_decode_split_layout():
    from sad.engine import to_split
    x = torch.randn(2, 3, 3, 64) * 3
    got = E.decode(to_split(x), 'bf16x3')
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    assert torch.equal(got, (hi.double() + lo.double()).reshape(2, 9, 64))
    assert torch.equal(E.decode(x.to(torch.float16), 'fp16'), x.to(torch.float16).double().reshape(2, 9, 64))


# ------------------------------------------------------------------ timeline --
def _one_hot_windows(W, N=2):
    """E[w, n] has column sums (w + 1) * (n + 1) * (x + 1), spread over two rows."""
    ev = np.zeros((W, N, 16, 16))
    for w in range(W):
        for n in range(N):
            for x in range(16):
                ev[w, n, 3, x] = 0.25 * (w + 1) * (n + 1) * (x + 1)
                ev[w, n, 11, x] = 0.75 * (w + 1) * (n + 1) * (x + 1)
    return ev


@pytest.mark.parametrize('impl', ['reference', 'product'])
def test_timeline_hop_one_window(impl):
    from sad.evidence import timeline
    fn = E.timeline if impl == 'reference' else timeline
    ev = _one_hot_windows(3)
    t = fn(ev, [0.0, 4.0, 8.0], 4.0)
    assert t.shape == (2, 48)
    for w in range(3):
        for x in range(16):
            assert t[0, 16 * w + x] == (w + 1) * (x + 1) and t[1, 16 * w + x] == 2 * (w + 1) * (x + 1)
    # a gap between windows: bins without a column centre are nan
    t = fn(ev[:2], [0.0, 6.0], 4.0)
    assert t.shape == (2, 40) and np.isnan(t[:, 16:24]).all() and not np.isnan(t[:, :16]).any()
    assert t[1, 24] == 2 * 2 * 1


@pytest.mark.parametrize('impl', ['reference', 'product'])
def test_timeline_hop_015_windows(impl):
    """hop 0.6 s = 2.4 bins: window w's column x has its centre in bin
    floor(2.4 w + x + 0.5); overlapping columns average."""
    from sad.evidence import timeline
    fn = E.timeline if impl == 'reference' else timeline
    W = 5
    ev = _one_hot_windows(W)
    ts = [0.6 * w for w in range(W)]
    t = fn(ev, ts, 4.0)
    want = {}
    for w in range(W):
        for x in range(16):
            want.setdefault(int(np.floor(2.4 * w + x + 0.5 + 1e-9)), []).append((w + 1) * (x + 1))
    assert t.shape == (2, max(want) + 1)
    for k in range(t.shape[1]):
        assert t[0, k] == pytest.approx(np.mean(want[k]), rel=1e-14)
        assert t[1, k] == pytest.approx(2 * np.mean(want[k]), rel=1e-14)
    assert len(want[2]) == 2 and len(want[0]) == 1          # bin 2: window 0 column 2 (2.5) and window 1 column 0 (2.9)


def test_axes():
    from sad.audio import melscale_fbanks
    from sad.evidence import col_sec, row_hz
    assert np.array_equal(col_sec(4.0), np.arange(16) * 0.25)
    fb = melscale_fbanks(1025, 20.0, 12000.0, 128, 32000, True).numpy()
    r = row_hz(fb, 32000)
    assert r.shape == (16, 2) and (r[:, 0] < r[:, 1]).all()
    assert (np.diff(r[:, 0]) > 0).all() and (np.diff(r[:, 1]) > 0).all()      # row 0 is the lowest band
    assert 20.0 <= r[0, 0] <= 40.0 and 11000.0 <= r[15, 1] <= 12000.0
