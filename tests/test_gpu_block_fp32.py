"""GPU: the fp32 block-conv kernel, launch_block_v<float> (csrc/block.hip,
variants 9..19 and 0 = the library's choice) -- what every conv of an 'fp32'
backbone and of the fp32 trainer forward runs on -- one variant at a time through
block_conv(..., variant=v) on float32 tensors, element for element against the
float64 contract of tests/parity_ref.py:

  rounding  a quiet image with large border pixels (a padding slip is far over
            the bar) under (K + 8) 2^-24 S per element, exact zeros under ReLU
            where the float64 pre-activation is <= -bar;
  exact     integer operands (fp16_ref.exact_operands): every product and partial
            sum is exact, the output must EQUAL the reference, tolerance zero;
  bits      every variant walks K in the same order (K-step by K-step, chunk fg
            then fg + 4 inside a step, in both wave-tile code paths, and an fp32
            chunk is the same four 16x16x4 MFMAs everywhere), so all accepted
            variants agree bit for bit, as tests/test_gpu_blockconv.py asserts for
            bf16;
  guards    4 KiB of fill before and behind `out` stay untouched;
  refusals  a channel tile that does not divide Cout, `res` on any variant but
            13: the library's RuntimeError, `out` untouched.

Shapes (parity_ref.GEMM_SHAPES; the fp32 K-step is 32 channels): 1, 2 and 3
K-steps, M = 15, M one past 128 / 256 / 512, 3x3 stride 1 and 2 on 5 x 9 and
9 x 5, 1x1 stride 1 and 2, identity and downsample K columns, variant 13's
epilogue residual and its downsample-columns form, Cout 64 / 128 / 192 / 256,
ReLU on and off, N = 0.

The fused average pool of variants 13 and 15 is not reachable through
block_conv; the backbone tests (test_gpu_parity.py) cover it.
"""
import pytest
import torch

import parity_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 4096
FILL = 0xFF


def launch(c, ops, v, split=False, four=False):
    """One block_conv launch into a guarded buffer -> (out on the CPU, the raw
    buffer).  ops: fp32 CPU tensors (x, w, bias, sc, res); split: sent in the
    split-bf16 layout.  A refusal raises before anything is written."""
    from sad.engine import block_conv, to_split
    x, w, bias, sc, res = ops
    w = P.sent_weights(c, w)
    dev = lambda t: None if t is None else (to_split(t) if split else t).to(DEV).contiguous()  # noqa: E731
    Ho, Wo = P.out_hw(c)
    dt = torch.bfloat16 if split else torch.float32
    C = 2 * c.cout if split else c.cout
    nbytes = x.shape[0] * Ho * Wo * C * (2 if split else 4)
    raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)
    out = raw[GUARD:GUARD + nbytes].view(dt).view(x.shape[0], Ho, Wo, C)
    try:
        block_conv(dev(x), dev(w), bias.to(DEV), c.stride, c.pad, sc=dev(sc), sc_stride=P.sc_stride(c), relu=c.relu,
                   variant=v, out=out, res=dev(res), k=c.k, split=split, four=four)
    finally:
        torch.cuda.synchronize()
    return out.cpu(), raw


def guards_ok(raw):
    return bool((raw[:GUARD] == FILL).all() and (raw[-GUARD:] == FILL).all())


def refused(c, ops, v, why, **kw):
    """the launch raises the library's error and leaves the whole buffer as it was"""
    from sad.engine import block_conv, to_split
    split = kw.get('split', False)
    x, w, bias, sc, res = ops
    w = P.sent_weights(c, w)
    dev = lambda t: None if t is None else (to_split(t) if split else t).to(DEV).contiguous()  # noqa: E731
    Ho, Wo = P.out_hw(c)
    out = torch.full((x.shape[0], Ho, Wo, 2 * c.cout if split else c.cout), 7.0,
                     dtype=torch.bfloat16 if split else torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match=why):
        block_conv(dev(x), dev(w), bias.to(DEV), c.stride, c.pad, sc=dev(sc), sc_stride=P.sc_stride(c), relu=c.relu,
                   variant=v, out=out, res=dev(res), k=c.k, **kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), f'variant {v}: a refused launch wrote to out'


def _all_variants(name, ops, check):
    """every variant on one shape: refusals asserted, check(v, out) on the rest,
    guards, then bit equality across the accepted variants"""
    c = P.GEMM_SHAPES[name]
    outs = {}
    for v in P.GEMM_VARIANTS:
        why = P.gemm_refusal(v, c)
        if why:
            refused(c, ops, v, why)
            continue
        out, raw = launch(c, ops, v)
        assert guards_ok(raw), f'variant {v}: guard bytes around out'
        check(v, out)
        outs[v] = out
    assert len(outs) >= 2
    for v, out in outs.items():
        assert torch.equal(out.view(torch.int32), outs[0].view(torch.int32)), \
            f'variant {v} differs from the default choice in some bit'
    return outs


@pytest.mark.parametrize('name', list(P.GEMM_SHAPES))
def test_rounding(name):
    c = P.GEMM_SHAPES[name]
    ops = P.random_operands(P.generator('random32', name), c, post_relu=False)
    ref, bar, zero = P.fp32_contract(c, *ops)
    assert ref.numel() > 0 and (not c.relu or ((ref == 0).any() and (ref > 0).any()))
    ratios = {}

    def check(v, out):
        ratios[v] = P.worst_ratio(out, ref, bar, zero)

    _all_variants(name, ops, check)
    print(f'RATIO block fp32 {name}: ' + ', '.join(f'v{v} {q:.3g}' for v, q in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize('name', list(P.GEMM_SHAPES))
def test_exact(name):
    c = P.GEMM_SHAPES[name]
    ops = P.exact_operands_f32(P.generator('exact32', name), c)
    ref, _, _ = P.fp32_contract(c, *ops)
    assert torch.equal(ref, ref.round()) and (ref != 0).double().mean().item() >= 0.25

    def check(v, out):
        bad = int((out.double() != ref).sum())
        assert bad == 0, f'variant {v}: {bad} of {ref.numel()} values differ'

    _all_variants(name, ops, check)


def test_empty_batch_writes_nothing():
    """N = 0 with valid pointers: accepted by every variant, nothing is written."""
    from sad import _lib
    c = P.GEMM_SHAPES['3x3 s1 5x9']
    x, w, bias, _, _ = P.random_operands(P.generator('random32', 'empty'), c, post_relu=False)
    dx, dw, db = x.to(DEV), w.to(DEV), bias.to(DEV)
    out = torch.full((GUARD,), FILL, dtype=torch.uint8, device=DEV)
    for v in P.GEMM_VARIANTS:
        with torch.cuda.device(DEV):
            _lib.call('sad_block_conv_run', dx.data_ptr(), 0, c.H, c.W, c.cin, None, 0, 0, 0, 1, dw.data_ptr(),
                      w.shape[1], db.data_ptr(), None, out.data_ptr(), c.cout, c.k, c.stride, c.pad, 1,
                      _lib.DTYPES['fp32'], v, _lib.stream_handle(torch.device(DEV)))
        torch.cuda.synchronize()
        assert bool((out == FILL).all()), v
