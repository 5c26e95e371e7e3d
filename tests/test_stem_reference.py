"""CPU: the float64 stem reference of tests/stem_ref.py is itself right, and
the comparison it feeds is sharp.

Reference checks: with fp32 operands it is float64 torch's
max_pool2d(relu(bn1(conv1(x)))) on the image repeated over 3 channels (up to
the one fp32 rounding of the folded weights and bias); its resize is the
oracle's; the k/4 maps make the fp32 resize exact (the precondition of the
quantised map paths) for every map shape the GPU tests use; the workgroup
branch counts are those of the kernel's index arithmetic.

Sharpness: got := the clean reference rounded to the output dtype.  Each
mutated reference below is a kernel bug that the loose global bars of the older
stem tests let through; compared under its own a-priori bar it must reject
`got` on at least one case, and the clean reference must accept it on all.
"""
import pytest
import torch
import torch.nn.functional as F

import stem_ref as R

MAP_SHAPES = [(128, 251), (1, 1), (7, 5), (64, 2), (129, 300), (136, 511), (512, 512), (64, 100)]


@pytest.fixture(scope='module')
def params():
    return R.random_stem_params(torch.Generator().manual_seed(21))


@pytest.fixture(scope='module')
def cases(params):
    """name -> (dtype, kwargs, clean ref, clean bar, got), B = 1."""
    g = torch.Generator().manual_seed(22)
    fd = R.fold(*params)
    spec = {
        'bf16 map 128x251': ('bf16', dict(map=R.exact_map(g, 1, 128, 251))),
        'bf16x3 map 7x5': ('bf16x3', dict(map=R.exact_map(g, 1, 7, 5))),
        'fp32 img': ('fp32', dict(img=torch.randn(1, 512, 512, generator=g))),
        'bf16 img seams': ('bf16', dict(img=R.adversarial_image(g, 1).bfloat16().float())),
    }
    out = {}
    for name, (dtype, kw) in spec.items():
        ref, bar = R.reference(dtype, fd, **kw)
        out[name] = (dtype, kw, ref, bar, R.round_output(ref, dtype))
    return out


# ------------------------------------------------------------ the reference --
@pytest.mark.parametrize('bn', ['identity', 'random'])
def test_fp32_reference_is_torch_conv_bn_relu_maxpool(params, bn):
    W, gamma, beta, mean, var = params
    if bn == 'identity':
        gamma, beta, mean, var = torch.ones(64), torch.zeros(64), torch.zeros(64), torch.ones(64)
    g = torch.Generator().manual_seed(3)
    img = torch.randn(2, 512, 512, generator=g)
    fd = R.fold(W, gamma, beta, mean, var)
    ref, _ = R.reference('fp32', fd, img=img)
    x3 = img.double().unsqueeze(1).repeat(1, 3, 1, 1)
    y = F.conv2d(x3, W.double(), stride=2, padding=3)
    y = F.batch_norm(y, mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    want = F.max_pool2d(torch.relu(y), 3, 2, 1).permute(0, 2, 3, 1)
    # the reference's operands are the fp32 roundings of the folded weights and bias
    S = R.pool(R.conv7(img.double().abs(), fd.w32.abs())).permute(0, 2, 3, 1)
    tol = 2 * R.U * (S + fd.bias.abs().view(1, 1, 1, -1)) + 1e-300
    assert torch.all((ref - want).abs() <= tol)
    assert ref.max() > 1.0 and (ref == 0).any() and not (ref == 0).all()   # ReLU clamps some, not all


def test_distinct_channel_reference_is_torch(params):
    W, gamma, beta, mean, var = params
    g = torch.Generator().manual_seed(4)
    x3 = torch.randn(1, 3, 512, 512, generator=g)
    fd = R.fold(*params)
    ref, _ = R.reference('bf16', fd, img3=x3)
    y = F.conv2d(x3.double(), W.double(), stride=2, padding=3)
    y = F.batch_norm(y, mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, 1e-5)
    want = F.max_pool2d(torch.relu(y), 3, 2, 1).permute(0, 2, 3, 1)
    S = R.pool(R.conv7(x3.double().abs(), fd.w3.abs())).permute(0, 2, 3, 1)
    assert torch.all((ref - want).abs() <= 2 * R.U * (S + fd.bias.abs().view(1, 1, 1, -1)) + 1e-300)


def test_resize_is_the_oracles(golden_frontend):
    from oracle import frontend as ofe
    m = torch.from_numpy(golden_frontend['std_map'][:2])
    assert m.shape[1:] == (128, 251)
    want = ofe.resize_bilinear(m.double().unsqueeze(1), (512, 512)).squeeze(1)
    got = R.resize(m)
    assert (got - want).abs().max().item() <= 1e-13 * m.abs().max().item()
    assert (R.resize(m, order='yx') - got).abs().max().item() <= 1e-13 * m.abs().max().item()


@pytest.mark.parametrize('shape', MAP_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_quarter_maps_resize_exactly_in_fp32(shape):
    g = torch.Generator().manual_seed(5)
    m = R.exact_map(g, 2, *shape)
    assert R.resize_is_exact(m)
    # and the values do need the bf16 rounding (the quantised paths are exercised)
    if min(shape) > 1 and shape != (512, 512):                     # (512 x 512: the identity)
        r = R.resize(m)
        assert not torch.equal(R.bf16(r), r)


def test_real_maps_do_not_resize_exactly(golden_frontend):
    """Why the fixture map's cases carry the resize's fp32 rounding in their bar."""
    m = torch.from_numpy(golden_frontend['std_map'][:1])
    assert not torch.equal(R.resize(m, torch.float32).double(), R.resize(m))
    e = (R.resize(m, torch.float32).double() - R.resize(m)).abs()
    assert torch.all(e <= 8 * R.U * R.resize(m.abs()))


def test_workgroup_branches():
    """The branch table of the bf16 stems' resize (separable workgroups of 16)."""
    assert sum(R.separable_workgroups(128)) == 16
    assert sum(R.separable_workgroups(129)) == 16 and max(R.band_source_rows(129)) == 12
    assert (min(R.band_source_rows(128)), max(R.band_source_rows(128))) == (10, 12)
    assert (min(R.band_source_rows(136)), max(R.band_source_rows(136))) == (10, 13)
    assert min(R.band_source_rows(200)) >= 14
    assert sum(R.separable_workgroups(136)) == 9
    assert sum(R.separable_workgroups(200)) == 0 and sum(R.separable_workgroups(512)) == 0
    assert all(sum(R.separable_workgroups(h)) == 16 for h in (1, 7, 64))


def test_split_reference_drops_only_the_lo_lo_product(params):
    g = torch.Generator().manual_seed(6)
    img = torch.randn(1, 512, 512, generator=g)
    fd = R.fold(*params)
    (xh, xl), (wh, wl) = R.quantise(img.double(), 'bf16x3'), R.weight_planes('bf16x3', fd)
    three = R.conv7(xh, wh) + R.conv7(xh, wl) + R.conv7(xl, wh)
    ref3, _ = R.reference('bf16x3', fd, img=img)
    ref4, _ = R.reference('bf16x3', fd, img=img, four=True)
    b = fd.bias.view(1, -1, 1, 1)
    want3 = torch.relu(R.pool(three) + b).permute(0, 2, 3, 1)
    want4 = torch.relu(R.pool(three + R.conv7(xl, wl)) + b).permute(0, 2, 3, 1)
    assert (ref3 - want3).abs().max().item() <= 1e-13 and (ref4 - want4).abs().max().item() <= 1e-13
    assert (ref3 - ref4).abs().max().item() > 0


def test_output_codecs_round_trip():
    g = torch.Generator().manual_seed(7)
    v = torch.randn(3, 5, 64, generator=g)
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    packed = torch.stack([hi.view(3, 5, 2, 32), lo.view(3, 5, 2, 32)], dim=-2).reshape(3, 5, 128)
    assert torch.equal(R.decode(packed, 'bf16x3'), R.round_output(v.double(), 'bf16x3'))
    assert torch.equal(R.decode(hi, 'bf16'), R.round_output(v.double(), 'bf16'))


# ---------------------------------------------------------------- sharpness --
def _truncate(x, dtype):
    assert dtype == 'bf16'
    bits = x.to(torch.float32).view(torch.int32) & -65536          # drop the low 16 bits
    return (bits.view(torch.float32).double(),)


def _drop_tap(ws):
    ws = tuple(w.clone() for w in ws)
    for w in ws:
        w[:, 6, 6] = 0.0
    return ws


def _no_left_neighbour(q):
    def pool_fn(c):
        p = R.pool(c).clone()
        p[..., q] = F.max_pool2d(c[..., 2 * q:2 * q + 2], (3, 2), (2, 2), (1, 0))[..., 0]
        return p
    return pool_fn


def _pad_line(axis):
    def edit(xs):
        xs = tuple(x.clone() for x in xs)
        for x in xs:
            x.select(axis, 511).zero_()
        return xs
    return edit


def _unclamped_resize(m):
    return R.resize(m, clamp=False)


def _omit_whi_xlo(c, xs, ws):
    return c - R.conv7(xs[1], ws[0])


def _min_pool_negative_gamma(gamma):
    """The pool taken on the conv BEFORE the sign of a negative scale (bias and
    all), i.e. a min where the folded conv needs a max."""
    neg = (gamma < 0).view(1, -1, 1, 1)

    def pool_fn(c):
        return torch.where(neg, -R.pool(-c), R.pool(c))
    return pool_fn


def _mutations(gamma):
    return {
        'band truncated, not RNE': (dict(quantise_fn=_truncate), ['bf16 map 128x251']),
        'tap (6,6) dropped': (dict(edit_weights=_drop_tap), None),
        'pooled column 32 without conv column 63': (dict(pool_fn=_no_left_neighbour(32)), None),
        'pooled column 64 without conv column 127': (dict(pool_fn=_no_left_neighbour(64)), None),
        'pooled column 96 without conv column 191': (dict(pool_fn=_no_left_neighbour(96)), None),
        'image row 511 as padding': (dict(edit_image=_pad_line(-2)), None),
        'image column 511 as padding': (dict(edit_image=_pad_line(-1)), None),
        'fy < 0 clamp removed': (dict(resize_fn=_unclamped_resize), ['bf16 map 128x251', 'bf16x3 map 7x5']),
        'W_hi.X_lo omitted': (dict(edit_conv=_omit_whi_xlo), ['bf16x3 map 7x5']),
        'min-pool for negative gamma': (dict(pool_fn=_min_pool_negative_gamma(gamma)), None),
    }


MUTATIONS = list(_mutations(torch.zeros(64)))


def test_clean_reference_accepts_its_own_rounding(cases):
    for name, (dtype, kw, ref, bar, got) in cases.items():
        r = R.worst_ratio(got, ref, bar)
        print(f'{name}: clean worst |d|/bar {r:.3f}')
        assert r <= 1.0, name


@pytest.mark.parametrize('mutation', MUTATIONS)
def test_mutated_reference_rejects(params, cases, mutation):
    hooks, only = _mutations(params[1])[mutation]
    fd = R.fold(*params)
    worst = {}
    for name, (dtype, kw, ref, bar, got) in cases.items():
        if only is not None and name not in only:
            continue
        mref, mbar = R.reference(dtype, fd, **kw, **hooks)
        worst[name] = R.worst_ratio(got, mref, mbar)
        if worst[name] > 1.0:
            break
    print(f'{mutation}: ' + ', '.join(f'{k} {v:.3g}' for k, v in worst.items()))
    assert max(worst.values()) > 1.0, worst
