"""GPU: the fp16 (SAD_F16) form of every tuned kernel, one kernel at a time
through block_conv(..., variant=v), conv2d and the fused layer1 block wrapper,
against the float64 contract of tests/fp16_ref.py.

Shapes are the existing tables', imported: tests/test_gpu_kstep_parity.py's CASES
(variants 31 and 44: odd and even K-steps per tile, more than one tile per
workgroup; id-31 takes its identity as the fp32 epilogue residual, read as
fp16), tests/test_gpu_l2conv_loop.py's FORMS x SHAPES (variant 41, and the same
output shapes for variant 43's 64 -> 128 stride-2 conv),
tests/test_gpu_l1block_loop.py's SHAPES (the fused layer1 block, variant 40), and
one implicit-GEMM case, 3x3 s1 on a 5 x 9 map with Cout 64 as in
tests/test_gpu_conv_igemm.py (conv2d's kernel and block_conv's variant 9), and
tests/test_gpu_blockconv.py's layer1 / layer2 shapes for halo.hip's variants 25
and 20 / 21 / 22.

Per case:
  exact      integer operands (x in 0..3, weights in {-1, 0, 1} with at most 16
             non-zeros per output row, integer biases and shortcut sources):
             every operand, product, partial sum and output is exact in bf16,
             fp16 and fp32, so the fp16 output must EQUAL the float64 reference
             and the bf16 kernel's output, value for value (tolerance zero: any
             indexing, layout or unpacking slip shows); >= 25 % non-zero outputs.
  rounding   random fp16-exact operands in fp16's normal range under fp16_ref's
             bar, 2^-11 |ref| + 4 sqrt(K) 2^-24 max|ref|.
  position   one more image in front leaves images 1..N bit-identical.
The fused layer1 block rounds its intermediate to fp16 inside the kernel; its
rounding case makes conv1 exact (x = k/4, w1 = +-{1/2, 1, 2} sparse, b1 = k/8:
the intermediate is a multiple of 1/8 below 2^11 / 8, one well-defined fp16
value), so the bar applies to conv2 + identity with random fp16 weights.
Then the stem against tests/stem_ref.py's float64 reference under its bf16 bar
formula with u = 2^-11 (fp16_ref.stem_reference), and the saturation contract.
"""
import ctypes
import zlib

import pytest
import torch

import fp16_ref as R16
import stem_ref as S
import test_gpu_kstep_parity as KP
import test_gpu_l1block_loop as L1
import test_gpu_l2conv_loop as L2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F16, BF16 = torch.float16, torch.bfloat16


# name -> (N, H, W (output), Cin, Cout, stride, form, Cin1, variant)
#   form: None | 'res' (epilogue residual) | 'ds' (1x1/2 of a 2x source as K columns)
def _cases():
    c = {}
    for name, (N, H, Cin, Cout, stride, sc, v) in KP.CASES.items():
        Ho = H // stride
        form, cin1 = (None, 0) if sc is None else ('res', 0) if sc == 'id' else ('ds', sc[1])
        c[name] = (N, Ho, Ho, Cin, Cout, stride, form, cin1, v)
    for form in L2.FORMS:
        for (N, H, W) in L2.SHAPES:
            f = None if form == 'plain' else form
            c[f'{form}-41-{N}x{H}x{W}'] = (N, H, W, 128, 128, 1, f, 64 if form == 'ds' else 0, 41)
    for (N, H, W) in L2.SHAPES:
        c[f's2-43-{N}x{H}x{W}'] = (N, H, W, 64, 128, 2, None, 0, 43)
    c['igemm-9-2x5x9'] = (2, 5, 9, 64, 64, 1, None, 0, 9)
    # the halo kernels of halo.hip: variant 25 (64 -> 64 resident weights: the deep Bottleneck plans' layer1
    # conv2, unfused layer1) with 320 tiles on 256 workgroups and with few, variants 20 / 21 / 22
    # (weight ring; 22: register epilogue), plain and with the epilogue residual -- shapes of
    # tests/test_gpu_blockconv.py's l1-res, l1-plain, l2-res and l2-plain-halo cases
    c['l1-res-25'] = (5, 128, 128, 64, 64, 1, 'res', 0, 25)
    c['l1-plain-25'] = (2, 48, 48, 64, 64, 1, None, 0, 25)
    for v in (20, 21, 22):
        c[f'l2-res-{v}'] = (2, 32, 32, 128, 128, 1, 'res', 0, v)
    c['l2-plain-20'] = (3, 32, 32, 128, 128, 1, None, 0, 20)
    c['l2-plain-22'] = (3, 32, 32, 128, 128, 1, None, 0, 22)
    return c


CASES = _cases()


def test_case_table():
    assert [n for n in CASES if n in KP.CASES] == ['c192-31', 'ds64-31', 'l2ds-31', 'c192-44', 'id-31', 'l4-44']
    assert CASES['id-31'][6] == 'res' and len(CASES) == 6 + 18 + 6 + 1 + 7


def _launch(case, x, w, bias, sc, res, dtype, relu=True):
    from sad.engine import block_conv
    N, Ho, Wo, Cin, Cout, stride, form, cin1, v = case
    dev = lambda t: None if t is None else t.to(dtype).to(DEV).contiguous()
    out = block_conv(dev(x), dev(w), bias.to(DEV), stride, 1, sc=dev(sc), sc_stride=2 if sc is not None else 1,
                     relu=relu, variant=v, res=dev(res))
    torch.cuda.synchronize()
    return out.cpu()


def _geometry(case, extra=0):
    N, Ho, Wo, Cin, Cout, stride, form, cin1, v = case
    return N + extra, Ho * stride, Wo * stride, (2 * Ho, 2 * Wo) if form == 'ds' else None


# ------------------------------------------------------------------- exact --
@pytest.mark.parametrize('name', list(CASES))
def test_exact(name):
    case = CASES[name]
    N, Ho, Wo, Cin, Cout, stride, form, cin1, v = case
    n, H, W, sc_hw = _geometry(case)
    g = torch.Generator().manual_seed(zlib.crc32(('exact-' + name).encode()))
    x = torch.randint(0, 4, (n, H, W, Cin), generator=g).float()
    K = 9 * Cin + cin1
    w = torch.zeros(Cout, K)
    cols = torch.rand(Cout, K, generator=g).argsort(1)[:, :16]
    w.scatter_(1, cols, torch.randint(0, 2, (Cout, 16), generator=g).float() * 2.0 - 1.0)
    bias = torch.randint(-4, 9, (Cout,), generator=g).float()
    sc = torch.randint(0, 4, (n, *sc_hw, cin1), generator=g).float() if form == 'ds' else None
    res = torch.randint(0, 4, (n, Ho, Wo, Cout), generator=g).float() if form == 'res' else None
    ref = R16.conv_ref(x, w, bias, stride, sc, 2, res)
    assert torch.equal(ref, ref.round()) and ref.max().item() < 256
    out = _launch(case, x, w, bias, sc, res, F16)
    twin = _launch(case, x, w, bias, sc, res, BF16)
    nz = (ref != 0).double().mean().item()
    print(f'{name}: {nz:.2f} of the outputs non-zero, max {ref.max().item():.0f}')
    assert nz >= 0.25
    assert torch.equal(out.double(), ref), f'{(out.double() != ref).sum().item()} of {ref.numel()} values differ'
    assert torch.equal(out.double(), twin.double()), 'fp16 and bf16 kernels differ on exact operands'


# ---------------------------------------------------- rounding and position --
def _random_run(name):
    """(K, reference of images 1..N, output of images 1..N alone, output of images 0..N)"""
    case = CASES[name]
    N, Ho, Wo, Cin, Cout, stride, form, cin1, v = case
    n, H, W, sc_hw = _geometry(case, extra=1)
    g = torch.Generator().manual_seed(zlib.crc32(('round-' + name).encode()))
    x = R16.rand_f16(g, n, H, W, Cin)
    K = 9 * Cin + cin1
    w = R16.rand_f16(g, Cout, K)
    bias = torch.randn(Cout, generator=g)
    sc = R16.rand_f16(g, n, *sc_hw, cin1) if form == 'ds' else None
    res = R16.rand_f16(g, n, Ho, Wo, Cout) if form == 'res' else None
    cut = lambda t, lo: None if t is None else t[lo:]
    ref = R16.conv_ref(x[1:], w, bias, stride, cut(sc, 1), 2, cut(res, 1))
    outs = [_launch(case, x[lo:], w, bias, cut(sc, lo), cut(res, lo), F16) for lo in (1, 0)]
    return K + (1 if form == 'res' else 0), ref, outs[0], outs[1]


@pytest.mark.parametrize('name', list(CASES))
def test_rounding_and_position(name):
    K, ref, out, shifted = _random_run(name)
    assert (ref > 0).any() and ref.max().item() < R16.F16_MAX
    frac, worst = R16.over_bar(out, ref, K)
    same = (out.view(torch.int16) == shifted[1:].view(torch.int16)).flatten(1).all(1)
    print(f'RATIO fp16 {name}: worst |d|/bar {worst:.3f} (K {K}, max |ref| {ref.max().item():.1f}); '
          f'{int((~same).sum())} images differ after the shift')
    assert frac == 0.0, f'{frac:.2e} of the elements over the bar, worst |d|/bar {worst:.3f}'
    assert bool(same.all()), f'images that differ after the shift: {(~same).nonzero().flatten().tolist()[:20]}'


def test_conv2d_igemm_case():
    """conv.hip's implicit GEMM (sad_conv2d_run) on tests/test_gpu_conv_igemm.py's
    '3x3 s1 p1 Cout64' shape, with its residual: exact, then under the bar."""
    from sad.engine import conv2d
    import test_gpu_conv_igemm as CI
    N, H, W, ks, Cout, k, s, p, has_res, relu = CI.SHAPES['3x3 s1 p1 Cout64']
    Cin = ks * CI.KSTEP['bf16']
    g = torch.Generator().manual_seed(77)
    x, w, bias, _, r = R16.exact_operands(g, N, H, W, Cin, Cout, res=True)
    run = lambda dt, x, w, r: conv2d(x.to(dt).to(DEV), w.reshape(Cout, 3, 3, Cin).to(dt).to(DEV).contiguous(),
                                     bias.to(DEV), s, p, r.to(dt).to(DEV), relu).cpu()
    ref = R16.conv_ref(x, w, bias, s, res=r, relu=relu)
    out, twin = run(F16, x, w, r), run(BF16, x, w, r)
    torch.cuda.synchronize()
    assert (ref != 0).double().mean().item() >= 0.25
    assert torch.equal(out.double(), ref) and torch.equal(out.double(), twin.double())
    x, w, r = R16.rand_f16(g, N, H, W, Cin), R16.rand_f16(g, Cout, 9 * Cin), R16.rand_f16(g, N, H, W, Cout)
    ref = R16.conv_ref(x, w, bias, s, res=r, relu=relu)
    frac, worst = R16.over_bar(run(F16, x, w, r), ref, 9 * Cin + 1)
    print(f'RATIO fp16 conv2d igemm: worst |d|/bar {worst:.3f}')
    assert frac == 0.0


# ---------------------------------------------------- the fused layer1 block --
def _l1_ref(x, w1, b1, w2, b2):
    mid = R16.f16(R16.conv_ref(x, w1[:, :576], b1))
    return mid, R16.conv_ref(mid, w2[:, :576], b2, res=x)


def _l1_run(x, w1, b1, w2, b2, dtype):
    from sad.engine import l1_block
    dev = lambda t: t.to(dtype).to(DEV).contiguous()
    out = l1_block(dev(x), dev(w1), b1.to(DEV), dev(w2), b2.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


def _l1_w2(w576):
    """the engine's layout: 64 identity K columns after the taps (not read)"""
    w2 = torch.zeros(64, 640)
    w2[:, :576] = w576
    w2[:, 576:] = torch.eye(64)
    return w2


@pytest.mark.parametrize('N,H,W', L1.SHAPES)
def test_l1_block_exact(N, H, W):
    g = torch.Generator().manual_seed(31 * N + H + 7 * W)
    x, w1, b1, _, _ = R16.exact_operands(g, N, H, W, 64, 64)
    _, w2, b2, _, _ = R16.exact_operands(g, 1, 16, 16, 64, 64, nnz=4)  # (outputs stay below 256: exact in bf16 too)
    w2 = _l1_w2(w2)
    mid, ref = _l1_ref(x, w1, b1, w2, b2)
    assert torch.equal(ref, ref.round()) and ref.max().item() < 256 and mid.max().item() < 256
    out, twin = _l1_run(x, w1, b1, w2, b2, F16), _l1_run(x, w1, b1, w2, b2, BF16)
    assert (ref != 0).double().mean().item() >= 0.25
    assert torch.equal(out.double(), ref), f'{(out.double() != ref).sum().item()} of {ref.numel()} values differ'
    assert torch.equal(out.double(), twin.double())


def _l1_random(N, H, W):
    g = torch.Generator().manual_seed(131 * N + H + 7 * W)
    n = N + 1
    x = torch.randint(-8, 9, (n, H, W, 64), generator=g).float() / 4.0
    _, w1, _, _, _ = R16.exact_operands(g, 1, 16, 16, 64, 64)
    w1 = w1 * 2.0 ** torch.randint(-1, 2, w1.shape, generator=g).float()
    b1 = torch.randint(-16, 33, (64,), generator=g).float() / 8.0
    w2 = _l1_w2(R16.rand_f16(g, 64, 576).float())
    b2 = torch.randn(64, generator=g)
    mid, ref = _l1_ref(x[1:], w1, b1, w2, b2)
    assert torch.equal(mid * 8, (mid * 8).round()) and mid.max().item() < 256   # the intermediate is exact in fp16
    outs = [_l1_run(x[lo:], w1, b1, w2, b2, F16) for lo in (1, 0)]
    return ref, outs[0], outs[1]


@pytest.mark.parametrize('N,H,W', L1.SHAPES)
def test_l1_block_rounding_and_position(N, H, W):
    ref, out, shifted = _l1_random(N, H, W)
    frac, worst = R16.over_bar(out, ref, 577)
    print(f'RATIO fp16 l1block {N}x{H}x{W}: worst |d|/bar {worst:.3f} (max |ref| {ref.max().item():.1f})')
    assert frac == 0.0, f'{frac:.2e} of the elements over the bar, worst |d|/bar {worst:.3f}'
    same = (out.view(torch.int16) == shifted[1:].view(torch.int16)).flatten(1).all(1)
    assert bool(same.all()), f'images that differ after the shift: {(~same).nonzero().flatten().tolist()[:20]}'


def test_l1_block_wrapper_refuses_fp32():
    from sad.engine import l1_block
    x = torch.zeros(1, 16, 16, 64, device=DEV)
    with pytest.raises(ValueError, match='bfloat16 or float16'):
        l1_block(x, x, x, x, x)


# -------------------------------------------------------------------- stem --
def _stem_arrays(params, edit=None):
    from sad import weights as sw
    from sad.engine import _backbone_arrays
    sd = dict(sw.backbone_state_dict(0))
    W, gamma, beta, mean, var = params
    sd['conv1.weight'], sd['bn1.weight'], sd['bn1.bias'] = W, gamma, beta
    sd['bn1.running_mean'], sd['bn1.running_var'] = mean, var
    if edit:
        edit(sd)
    return _backbone_arrays(sd, sw.backbone_param_shapes())


@pytest.fixture(scope='module')
def stem_params():
    return S.random_stem_params(torch.Generator().manual_seed(31))


def _plan(arrays, mh, mw):
    from sad import _lib
    p = _lib.P()
    rc = _lib.load().sad_backbone_plan_create(_lib.pointer_array(arrays), len(arrays), _lib.SAD_F16, mh, mw,
                                              ctypes.byref(p))
    return rc, p


@pytest.mark.parametrize('shape', [(1, 1), (128, 251), (512, 512)], ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('src', ['map', 'img'])
def test_stem(stem_params, shape, src):
    from sad import _lib
    mh, mw = shape
    fd = S.fold(*stem_params)
    g = torch.Generator().manual_seed(100 + mh * 513 + mw)
    rc, plan = _plan(_stem_arrays(stem_params), mh, mw)
    assert rc == 0, _lib.load().sad_last_error()
    out = torch.empty(2, 128, 128, 64, dtype=F16, device=DEV)
    s = _lib.stream_handle(torch.device(DEV))
    try:
        if src == 'map':
            m = S.exact_map(g, 2, mh, mw)
            if torch.equal(m[0], m[1]):
                m[1, 0, 0] = m[0, 0, 0] + 0.25
            assert S.resize_is_exact(m)
            ref, bar = R16.stem_reference(fd, map=m)
            _lib.call('sad_backbone_stem_run', plan, _lib.ptr(m.to(DEV)), 2, _lib.ptr(out), s)
        else:
            img = S.adversarial_image(g, 2)
            ref, bar = R16.stem_reference(fd, img=img)
            _lib.call('sad_backbone_stem_run_img', plan, _lib.ptr(img.to(DEV)), None, 2, _lib.ptr(out), s)
        torch.cuda.synchronize()
    finally:
        _lib.load().sad_backbone_plan_destroy(plan)
    r = S.worst_ratio(out.cpu().double(), ref, bar)
    print(f'RATIO fp16 stem {src} {mh}x{mw}: worst |d|/bar {r:.3f} (max |ref| {ref.max().item():.3f})')
    assert r <= 1.0


# -------------------------------------------------------------- saturation --
@pytest.mark.parametrize('variant,Cin,Cout,H', [(9, 256, 64, 16), (31, 256, 256, 16)], ids=['generic-9', 'variant-31'])
def test_stores_saturate(variant, Cin, Cout, H):
    """Channels 0 / 1 carry weights of +-8 on every tap: over pixels of 8s their
    sums pass +-1e5.  Those outputs must be exactly +-65504, every value finite,
    and the rest within the bar (its floor from the unsaturated values)."""
    g = torch.Generator().manual_seed(variant)
    N, K = 2, 9 * Cin
    x = R16.rand_f16(g, N, H, H, Cin).float()
    x[0, 4:12, 4:12] = 8.0
    w = R16.rand_f16(g, Cout, K).float() / 16.0
    w[0], w[1] = 8.0, -8.0
    bias = torch.randn(Cout, generator=g)
    ref = R16.conv_ref(x, w, bias, relu=False)
    hot = ref.abs() > 1e5
    assert hot[..., 0].any() and hot[..., 1].any() and not hot[..., 2:].any()
    out = _launch((N, H, H, Cin, Cout, 1, None, 0, variant), x, w, bias, None, None, F16, relu=False).double()
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out[hot], torch.sign(ref[hot]) * R16.F16_MAX)
    cold = ref.abs() < R16.F16_MAX
    d = (out - ref).abs()
    bar = R16.U16 * ref.abs() + 4.0 * K ** 0.5 * R16.U32 * ref[cold].abs().max()
    assert bool((d[cold] <= bar[cold]).all())
    between = ~cold & ~hot          # past fp16's range but not past 1e5: saturated too
    assert torch.equal(out[between], torch.sign(ref[between]) * R16.F16_MAX)


def test_plan_refuses_weights_beyond_fp16(stem_params):
    from sad import _lib

    def huge(sd):
        sd['layer2.0.conv1.weight'] = sd['layer2.0.conv1.weight'].clone()
        sd['layer2.0.conv1.weight'][3, 5, 1, 1] = 1e6

    def huge_last(sd):  # the plan's last conv: everything before it (21 MB of fp16 weights) is uploaded by then
        sd['layer4.1.conv2.weight'] = sd['layer4.1.conv2.weight'].clone()
        sd['layer4.1.conv2.weight'][500, 7, 2, 0] = -1e6

    def nan_bias(sd):
        sd['layer3.1.bn2.bias'] = sd['layer3.1.bn2.bias'].clone()
        sd['layer3.1.bn2.bias'][7] = float('nan')

    torch.cuda.synchronize()
    free = [torch.cuda.mem_get_info(torch.device(DEV))[0]]    # the baseline, before the first refusal
    for edit, where in ((huge_last, b'layer4.1.conv2'), (huge, b'layer2.0.conv1'), (nan_bias, b'layer3.1.conv2'),
                        (huge_last, b'layer4.1.conv2'), (huge_last, b'layer4.1.conv2')):
        arrays = _stem_arrays(stem_params, edit)
        rc, p = _plan(arrays, 128, 251)
        msg = _lib.load().sad_last_error()
        assert rc == -1 and p.value is None, (rc, msg)       # SAD_ERR_ARG, *out untouched
        assert where in msg and b'fp16' in msg, msg
        free.append(torch.cuda.mem_get_info(torch.device(DEV))[0])
    # nothing stays allocated: a refusal at the last conv comes after ~21 MB of uploads, and three
    # of them leave the device's free memory where it was before the first (the allocator's
    # granule aside: 2 MB)
    print(f'free memory before / after each refusal (MiB): {[f >> 20 for f in free]}')
    assert free[0] - min(free[1:]) < (2 << 20), free
    # the same weights are a valid bf16 plan
    arrays = _stem_arrays(stem_params, huge)
    p = _lib.P()
    _lib.call('sad_backbone_plan_create', _lib.pointer_array(arrays), len(arrays), _lib.SAD_BF16, 128, 251,
              ctypes.byref(p))
    _lib.load().sad_backbone_plan_destroy(p)
