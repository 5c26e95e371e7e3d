"""GPU: every path of the fused inference stem (csrc/conv.hip stem_kernel,
stem_bf16_kernel<X3, false, X4>, stem3_kernel<0|1|2>) at its own output,
element for element against the float64 reference of tests/stem_ref.py, under
that file's a-priori rounding bars (u = 2^-24, BF = 2^-8; K u conv(|x|, |w|)
accumulation, the largest bar of the pool window, + u |v| for the bias add,
+ BF |ref| or 2^-16 |ref| for the output rounding).  No bar is a measured
error, no element is left out, and every case prints its worst error / bar.

What is reached that the one 128 x 251 fixture never reached:
  * map shapes 1 x 1 .. 512 x 512 (plans take any map_h, map_w <= 512), with the
    bf16 stems' per-workgroup resize branch asserted from the band's source-row
    count: all separable, the 12-row limit, both branches in one launch, all direct
  * the img path of all three stems, with an image whose large values sit on
    the kernels' block, wave and workgroup seams
  * the distinct-channel stem in all three output dtypes (bf16: first test)
  * the deep Bottleneck plans' stem (split-bf16: four products) on map, img, img3
  * B = 0, B = 65536, ambiguous sources; guard regions round every output
  * run_front's per-sub-batch map pointer on a non-default map shape

The quantised map paths use maps of values k/4: their fp32 resize is exact in
any evaluation order (asserted per case, float32 against float64), so the
bf16 / split rounding of the band is unambiguous.  The fixture map (real
values) runs in fp32 and split-bf16 with the resize's own fp32 rounding, 8 u of
the lerp terms, carried through conv(., |w|) into the bar.  For split-bf16 that
term stands for the image the kernel splits: a value that differs in its last
fp32 bit splits into the same hi and, almost always, the same lo.
"""
import ctypes

import pytest
import torch

import stem_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SAD_ERR_ARG = -1
GUARD = 4096                     # sentinel bytes before and after every output
FILL = 0xA5

# map shape -> number of separable workgroups (of 16) in the bf16 stems
MAP_SHAPES = {(128, 251): 16, (1, 1): 16, (7, 5): 16, (64, 2): 16, (129, 300): 16, (136, 511): 9, (512, 512): 0}


def _stream():
    from sad import _lib
    return _lib.stream_handle(torch.device(DEV))


@pytest.fixture(scope='module')
def params():
    return R.random_stem_params(torch.Generator().manual_seed(31))


@pytest.fixture(scope='module')
def folded(params):
    return R.fold(*params)


def _with_stem(sd, params):
    sd = dict(sd)
    W, gamma, beta, mean, var = params
    sd['conv1.weight'], sd['bn1.weight'], sd['bn1.bias'] = W, gamma, beta
    sd['bn1.running_mean'], sd['bn1.running_var'] = mean, var
    return sd


@pytest.fixture(scope='module')
def plans(params):
    """(dtype, map_h, map_w) -> ResNet-18 plan with the random conv1 / bn1; 'deep'
    -> the smallest Bottleneck plan ([1,1,1,1], split-bf16) on the same stem."""
    from sad import _lib
    from sad import weights as sw
    from sad.engine import _backbone_arrays
    lib = _lib.load()
    arrays = _backbone_arrays(_with_stem(sw.backbone_state_dict(0), params), sw.backbone_param_shapes())
    cache = {}

    def get(dtype, mh, mw):
        key = (dtype, mh, mw)
        if key not in cache:
            p = _lib.P()
            _lib.call('sad_backbone_plan_create', _lib.pointer_array(arrays), len(arrays), _lib.DTYPES[dtype], mh, mw,
                      ctypes.byref(p))
            cache[key] = p
        return cache[key]

    def deep(dtype, mh, mw):
        key = ('deep', dtype, mh, mw)
        if key not in cache:
            shapes = sw.backbone_param_shapes((1, 1, 1, 1), 'bottleneck')
            g = torch.Generator().manual_seed(32)
            sd = {}
            for name, shape, kind in shapes:
                if kind == 'conv':
                    std = (2.0 / (shape[0] * shape[2] * shape[3])) ** 0.5
                    sd[f'{name}.weight'] = torch.randn(*shape, generator=g) * std
                else:
                    sd[f'{name}.weight'], sd[f'{name}.bias'] = torch.ones(shape), torch.zeros(shape)
                    sd[f'{name}.running_mean'], sd[f'{name}.running_var'] = torch.zeros(shape), torch.ones(shape)
            arr = _backbone_arrays(_with_stem(sd, params), shapes)
            p = _lib.P()
            lay = (_lib.I32 * 4)(1, 1, 1, 1)
            _lib.call('sad_resnet_plan_create', _lib.pointer_array(arr), len(arr), 1, lay, _lib.DTYPES[dtype], mh, mw,
                      ctypes.byref(p))
            cache[key] = p
        return cache[key]

    get.deep = deep
    yield get
    torch.cuda.synchronize()
    for key, p in cache.items():
        (lib.sad_resnet_plan_destroy if key[0] == 'deep' else lib.sad_backbone_plan_destroy)(p)


def _run(entry, plan, dtype, B, srcs):
    """One stem launch into a guarded buffer -> (decoded output [B,128,128,64]
    float64 on the CPU, raw bytes incl. guards).  srcs: the entry's source
    tensors (None = null pointer), already on the device."""
    from sad import _lib
    nbytes = B * 128 * 128 * 64 * (2 if dtype == 'bf16' else 4)
    buf = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = buf.data_ptr() + GUARD                          # (B = 0: still a non-null pointer)
    assert out % 256 == 0
    rc = getattr(_lib.load(), entry)(plan, *[_lib.ptr(s) for s in srcs], B, out, _stream())
    torch.cuda.synchronize()
    raw = buf.cpu()
    if rc != 0 or B == 0:
        return rc, raw
    assert torch.all(raw[:GUARD] == FILL) and torch.all(raw[GUARD + nbytes:] == FILL), 'guard region overwritten'
    o = raw[GUARD:GUARD + nbytes]
    if dtype == 'fp32':
        t = o.view(torch.float32).view(B, 128, 128, 64)
    else:
        t = o.view(torch.bfloat16).view(B, 128, 128, -1)
    return R.decode(t, dtype), raw


def _check(label, got, ref, bar):
    r = R.worst_ratio(got, ref, bar)
    print(f'stem {label}: worst |d|/bar {r:.3f}  (max |ref| {ref.max().item():.3f}, elements {ref.numel()})')
    assert r <= 1.0, label
    return r


# ----------------------------------------------------------------- map path --
@pytest.mark.parametrize('shape', list(MAP_SHAPES), ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('dtype', R.DTYPES)
def test_map_path(plans, folded, dtype, shape):
    mh, mw = shape
    sep = R.separable_workgroups(mh)
    assert sum(sep) == MAP_SHAPES[shape]                   # the branch each of the 16 workgroups takes
    if shape == (129, 300):                                # the separable limit: a band of 12 map rows
        assert max(R.band_source_rows(mh)) == 12
    if shape == (136, 511):
        assert any(sep) and not all(sep)
    g = torch.Generator().manual_seed(100 + mh * 513 + mw)
    m = R.exact_map(g, 2, mh, mw)
    if torch.equal(m[0], m[1]):                            # (1 x 1: the two images must differ)
        m[1, 0, 0] = m[0, 0, 0] + 0.25
    assert R.resize_is_exact(m)                            # float32 == float64, either order
    ref, bar = R.reference(dtype, folded, map=m)
    got, _ = _run('sad_backbone_stem_run', plans(dtype, mh, mw), dtype, 2, [m.to(DEV)])
    _check(f'map {mh}x{mw} {dtype} (separable workgroups {sum(sep)}/16)', got, ref, bar)


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_map_path_fixture_map(plans, folded, golden_frontend, dtype):
    m = torch.from_numpy(golden_frontend['std_map'][:4])
    assert m.shape == (4, 128, 251)
    e_img = 8 * R.U * R.resize(m.abs())
    ref, bar = R.reference(dtype, folded, map=m, image_err=e_img)
    got, _ = _run('sad_backbone_stem_run', plans(dtype, 128, 251), dtype, 4, [m.to(DEV)])
    _check(f'map 128x251 fixture {dtype}', got, ref, bar)


# --------------------------------------------------------------- image path --
@pytest.fixture(scope='module')
def images():
    g = torch.Generator().manual_seed(41)
    return {'random': torch.randn(2, 512, 512, generator=g), 'seams': R.adversarial_image(g, 2)}


@pytest.mark.parametrize('kind', ['random', 'seams'])
@pytest.mark.parametrize('dtype', R.DTYPES)
def test_img_path(plans, folded, images, dtype, kind):
    img = images[kind]
    if dtype == 'bf16':
        img = img.bfloat16().float()                       # bf16-representable: the band's rounding is exact
    ref, bar = R.reference(dtype, folded, img=img)
    got, _ = _run('sad_backbone_stem_run_img', plans(dtype, 128, 251), dtype, 2, [img.to(DEV), None])
    _check(f'img {kind} {dtype}', got, ref, bar)


@pytest.mark.parametrize('dtype', R.DTYPES)
def test_distinct_channels(plans, folded, dtype):
    g = torch.Generator().manual_seed(42)
    x3 = torch.randn(2, 3, 512, 512, generator=g)
    ref, bar = R.reference(dtype, folded, img3=x3)
    got, _ = _run('sad_backbone_stem_run_img', plans(dtype, 128, 251), dtype, 2, [None, x3.to(DEV)])
    _check(f'img3 {dtype}', got, ref, bar)


# --------------------------------------------------------------- deep plans --
def _rms(a, b):
    return ((a - b) ** 2).mean().sqrt().item()


def test_deep_plan_stem_keeps_the_fourth_product(plans, folded, images):
    """Split-bf16: the Bottleneck plan's stem is the four-product form, the
    ResNet-18 plan's on the same weights the three-product form; each is nearer
    (RMS) to its own reference than to the other's."""
    img = images['random']
    ref3, bar3 = R.reference('bf16x3', folded, img=img)
    ref4, bar4 = R.reference('bf16x3', folded, img=img, four=True)
    deep = plans.deep('bf16x3', 128, 251)
    got4, _ = _run('sad_resnet_stem_run', deep, 'bf16x3', 2, [None, img.to(DEV), None])
    got3, _ = _run('sad_backbone_stem_run_img', plans('bf16x3', 128, 251), 'bf16x3', 2, [img.to(DEV), None])
    _check('deep img bf16x3 (four products)', got4, ref4, bar4)
    _check('img random bf16x3 (three products, same weights)', got3, ref3, bar3)
    r44, r43, r33, r34 = _rms(got4, ref4), _rms(got4, ref3), _rms(got3, ref3), _rms(got3, ref4)
    print(f'stem deep: rms X4 vs four {r44:.3e} / vs three {r43:.3e}; X3 vs three {r33:.3e} / vs four {r34:.3e}')
    assert r44 < r43 and r33 < r34


def test_deep_plan_stem_map_and_img3(plans, folded):
    g = torch.Generator().manual_seed(43)
    m = R.exact_map(g, 2, 136, 511)
    assert R.resize_is_exact(m)
    ref, bar = R.reference('bf16x3', folded, map=m, four=True)
    got, _ = _run('sad_resnet_stem_run', plans.deep('bf16x3', 136, 511), 'bf16x3', 2, [m.to(DEV), None, None])
    _check('deep map 136x511 bf16x3 (four products)', got, ref, bar)
    x3 = torch.randn(2, 3, 512, 512, generator=g)
    ref, bar = R.reference('bf16x3', folded, img3=x3)
    got, _ = _run('sad_resnet_stem_run', plans.deep('bf16x3', 136, 511), 'bf16x3', 2, [None, None, x3.to(DEV)])
    _check('deep img3 bf16x3', got, ref, bar)


# -------------------------------------------------------------------- edges --
def test_empty_batch_launches_nothing(plans):
    m = torch.zeros(1, 128, 251, device=DEV)
    for dtype in R.DTYPES:
        rc, raw = _run('sad_backbone_stem_run', plans(dtype, 128, 251), dtype, 0, [m])
        assert rc == 0
        assert torch.all(raw == FILL)


def test_oversized_batch_and_ambiguous_sources_are_refused(plans):
    from sad import _lib
    lib = _lib.load()
    p = plans('bf16', 128, 251)
    deep = plans.deep('bf16x3', 128, 251)
    buf = torch.full((GUARD,), FILL, dtype=torch.uint8, device=DEV)   # never written: every call is refused
    a, s = buf.data_ptr(), _stream()
    calls = [
        ('B > 65535', lambda: lib.sad_backbone_stem_run(p, a, 65536, a, s)),
        ('B > 65535', lambda: lib.sad_backbone_stem_run_img(p, a, None, 65536, a, s)),
        ('B > 65535', lambda: lib.sad_backbone_stem_run_img(p, None, a, 65536, a, s)),
        ('B > 65535', lambda: lib.sad_resnet_stem_run(deep, a, None, None, 65536, a, s)),
        ('exactly one of img / img3', lambda: lib.sad_backbone_stem_run_img(p, a, a, 1, a, s)),
        ('exactly one of img / img3', lambda: lib.sad_backbone_stem_run_img(p, None, None, 1, a, s)),
        ('exactly one of map / img / img3', lambda: lib.sad_resnet_stem_run(deep, None, None, None, 1, a, s)),
        ('exactly one of map / img / img3', lambda: lib.sad_resnet_stem_run(deep, a, a, None, 1, a, s)),
        ('exactly one of map / img / img3', lambda: lib.sad_resnet_stem_run(deep, a, None, a, 1, a, s)),
        ('exactly one of map / img / img3', lambda: lib.sad_resnet_stem_run(deep, a, a, a, 1, a, s)),
    ]
    for want, fn in calls:
        assert fn() == SAD_ERR_ARG
        assert want.encode() in lib.sad_last_error(), (want, lib.sad_last_error())
    torch.cuda.synchronize()
    assert torch.all(buf.cpu() == FILL)


# -------------------------------------------------------------- composition --
@pytest.mark.parametrize('dtype,B,sub', [('fp32', 40, 32), ('bf16x3', 70, 64), ('bf16', 260, 256)])
def test_front_sub_batches_advance_the_map_pointer(plans, dtype, B, sub):
    """sad_backbone_run on a 64 x 100 plan: segments past the first front
    sub-batch (run_front: map + i * map_h * map_w) give bit for bit the features
    of the same segments run as calls of their own."""
    from sad import _lib
    plan = plans(dtype, 64, 100)
    g = torch.Generator().manual_seed(50)
    maps = torch.randn(B, 64, 100, generator=g).to(DEV)
    sz = _lib.SZ()
    _lib.call('sad_backbone_workspace_size', plan, B, ctypes.byref(sz))
    ws = torch.empty(sz.value, dtype=torch.uint8, device=DEV)

    def run(x):
        feats = torch.full((x.shape[0], 512), float('nan'), device=DEV)
        _lib.call('sad_backbone_run', plan, _lib.ptr(x), x.shape[0], x.shape[0], _lib.ptr(feats), _lib.ptr(ws),
                  ws.numel(), _stream())
        torch.cuda.synchronize()
        return feats.cpu()

    whole = run(maps)
    parts = torch.cat([run(maps[:sub].contiguous()), run(maps[sub:].contiguous())])
    assert torch.isfinite(whole).all()
    assert not torch.equal(whole[0], whole[sub])           # different content per segment
    n_diff = (whole != parts).sum().item()
    print(f'stem front sub-batches {dtype} B={B}: features differing from separate calls {n_diff}')
    assert torch.equal(whole, parts)
