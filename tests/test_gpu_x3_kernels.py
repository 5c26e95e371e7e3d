"""GPU: the split-bf16 ('bf16x3') form of every block-conv kernel, one kernel at
a time through block_conv(..., split=True, variant=v), against the float64
contract of tests/parity_ref.py -- the net tests/test_gpu_fp16_kernels.py gives
bf16 and fp16, for the parity mode.

Variants: the implicit GEMM 9..19 and 0 (launch_block_v<u16, true>) on
parity_ref.GEMM_SHAPES -- the fp32 file's shape classes, 32 logical channels per
K-step, any H and W, identity and downsample columns, `res` on 13, 3x3 stride 2
and 1x1 --, its four-product form (four=True) on 9, 13 and 15 on the same shapes
and on the shape classes of test_gpu_x3.py's test_block_conv_four_products
(parity_ref.FOUR_SHAPES); and the 16 x 16-tiled kernels 42, 26, 20, 30, 31
(128- and 256-channel tiles) and 44 (parity_ref.TILED_FORMS) on the maps
(1,16,16), (1,16,32), (1,32,16), (2,48,32) and on 257 one-tile images (more tiles
than workgroups; five distinct images in a seeded order, the reference computed
for five).  Variants 31 and 44 run 18, 20, 36 and 40 K-steps per tile: the split
form's step count is always even (whole 64-channel multiples), what alternates
is the number of step pairs.  Each tiled kernel also runs once without ReLU
(negative stored pairs), and every `res` launch gets the engine's weight layout
(the identity's unread K columns behind the taps: rows longer than K).

Per case:
  (a) exact     operands whose lo halves are non-zero and whose products and
                partial sums are all exact in fp32 (parity_ref docstring): the
                output BYTES equal to_split(ref.float()) under the form the
                launch asked for, and differ from the other form's expectation;
  (b) rounding  random post-ReLU activations and He-scaled weights: per element
                |hi + lo - ref| <= (P K + 8) 2^-24 S3 + 2^-16 (|ref| + ...) against
                the contract of the stored operands, exact zeros under ReLU in
                both halves, |lo| <= 2^-8 |hi|;
  (c) position  one more image in front leaves images 1..N identical byte for
                byte;
  (d) guards    4 KiB of fill before and behind `out` stay untouched.

The fused average pool of variants 13, 15, 30 and 31 is not reachable through
block_conv; the backbone tests of test_gpu_x3.py cover it.
"""
import pytest
import torch

import parity_ref as P
from test_gpu_block_fp32 import guards_ok, launch, refused

pytestmark = pytest.mark.gpu
TILED = P.tiled_cases()
I16 = torch.int16


def _take(ops, idx):
    """the launch's images: rows idx of the per-image operands"""
    x, w, bias, sc, res = ops
    pick = lambda t: None if t is None else t[idx]  # noqa: E731
    return pick(x), w, bias, pick(sc), pick(res)


def _exact(tag, name, c, runs, slots=None):
    """(a) + (d) for each (variant, four) of runs on one case's exact operands"""
    ops = P.exact_operands_split(P.generator('exact', f'{tag} {name}'), c)
    fig, e3, e4 = P.exact_conditions(c, *ops)
    P.check_conditions(fig)
    idx = torch.arange(c.N) if slots is None else slots
    sent = _take(ops, idx)
    for v, four in runs:
        out, raw = launch(c, sent, v, split=True, four=four)
        assert guards_ok(raw), f'variant {v}: guard bytes around out'
        want, other = ((e4, e3) if four else (e3, e4))
        bad = int(P.differing(out, want[idx]).sum())
        assert bad == 0, f'variant {v} four={four}: {bad} of {out.numel() // 2} stored outputs differ'
        assert torch.equal(out.view(I16), want[idx].view(I16))
        assert int(P.differing(out, other[idx]).sum()) > 0


def _rounding_position(tag, name, c, runs, slots=None):
    """(b) + (c) + (d); image 0 of the operands is the extra one in front"""
    ops = P.random_operands(P.generator('random', f'{tag} {name}'), c, post_relu=True, extra=1)
    idx = 1 + (torch.arange(c.N) if slots is None else slots)
    sent = _take(ops, idx)
    shifted = _take(ops, torch.cat([torch.zeros(1, dtype=torch.long), idx]))
    own = _take(ops, torch.arange(1, c.N + 1))
    refs = {four: P.split_contract(c, *own, four=four)[:3] for four in {f for _, f in runs}}
    ratios = {}
    for v, four in runs:
        out, raw = launch(c, sent, v, split=True, four=four)
        assert guards_ok(raw), f'variant {v}: guard bytes around out'
        ref, bar, zero = (None if t is None else t[idx - 1] for t in refs[four])
        ratios[f'v{v}{"x4" if four else ""}'] = P.split_ratio(out, ref, bar, zero)
        out1, raw = launch(c, shifted, v, split=True, four=four)
        assert guards_ok(raw)
        same = (out.view(I16) == out1[1:].view(I16)).flatten(1).all(1)
        assert bool(same.all()), f'variant {v}: images that differ after the shift: ' \
                                 f'{(~same).nonzero().flatten().tolist()[:20]}'
    print(f'RATIO x3 {tag} {name}: ' + ', '.join(f'{k} {q:.3g}' for k, q in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def _gemm_runs(c):
    runs = [(v, False) for v in P.GEMM_VARIANTS if P.gemm_refusal(v, c) is None]
    return runs + [(v, True) for v in P.FOUR_VARIANTS if P.gemm_refusal(v, c) is None]


# ------------------------------------------------ the implicit GEMM, 9..19 --
@pytest.mark.parametrize('name', list(P.GEMM_SHAPES))
def test_gemm_exact(name):
    _exact('gemm', name, P.GEMM_SHAPES[name], _gemm_runs(P.GEMM_SHAPES[name]))


@pytest.mark.parametrize('name', list(P.GEMM_SHAPES))
def test_gemm_rounding_position(name):
    _rounding_position('gemm', name, P.GEMM_SHAPES[name], _gemm_runs(P.GEMM_SHAPES[name]))


@pytest.mark.parametrize('name', list(P.GEMM_SHAPES))
def test_gemm_refusals(name):
    c = P.GEMM_SHAPES[name]
    ops = P.exact_operands_split(P.generator('exact', f'gemm {name}'), c)
    for v in P.GEMM_VARIANTS:
        why = P.gemm_refusal(v, c)
        if why:
            refused(c, ops, v, why, split=True)
            if v in P.FOUR_VARIANTS:
                refused(c, ops, v, why, split=True, four=True)


@pytest.mark.parametrize('name', list(P.FOUR_SHAPES))
def test_four_product_shapes(name):
    c, v = P.FOUR_SHAPES[name]
    _exact('four', name, c, [(v, False), (v, True)])
    _rounding_position('four', name, c, [(v, False), (v, True)])


def test_four_products_refused_off_the_gemm():
    c, v, _ = TILED['42 plain 1x16x16']
    ops = P.exact_operands_split(P.generator('exact', 'four refused'), c)
    refused(c, ops, v, 'four-product', split=True, four=True)
    refused(c, ops, 11, 'four-product', split=True, four=True)


# ------------------------------------------------- the 16 x 16-tiled kernels --
@pytest.mark.parametrize('name', list(TILED))
def test_tiled_exact(name):
    c, v, slots = TILED[name]
    _exact('tiled', name, c, [(v, False)], slots)


@pytest.mark.parametrize('name', list(TILED))
def test_tiled_rounding_position(name):
    c, v, slots = TILED[name]
    _rounding_position('tiled', name, c, [(v, False)], slots)


def test_tiled_variants_refuse_half_a_chunk_pair():
    """Cin = 32 (one 128-B chunk of the split layout) and a 32-channel shortcut
    source: halo256_ok, halo31_ok and halo256rs2_ok ask for 64-channel multiples,
    which is why the tables above have no odd K-step count for 30, 31 and 44."""
    for form, why in (('30 c64 plain', 'variant 30'), ('31 t128 c64 plain', 'variant 31'),
                      ('44 c64-128', 'variant 44')):
        c, v, _ = TILED[f'{form} 1x16x16']
        c = c._replace(cin=32)
        refused(c, P.exact_operands_split(P.generator('exact', f'half {form}'), c), v, why, split=True)
    c, v, _ = TILED['31 t128 c64 ds 1x16x16']
    c = c._replace(cin1=32)
    refused(c, P.exact_operands_split(P.generator('exact', 'half ds'), c), v, 'variant 31', split=True)


def test_defaults_are_the_tiled_variants():
    """variant 0 picks 42 (64 -> 64), 31 (Cout 128), 30 (Cout % 256) and 44
    (stride 2, Cout % 256): the default's bytes are that variant's bytes."""
    for form in ('42 plain', '31 t128 c64 plain', '30 c64 plain', '44 c128-256'):
        c, v, _ = TILED[f'{form} 1x16x32']
        assert v in P.SPLIT_DEFAULTS
        ops = P.random_operands(P.generator('random', f'default {form}'), c, post_relu=True)
        a, _ = launch(c, ops, 0, split=True)
        b, _ = launch(c, ops, v, split=True)
        assert torch.equal(a.view(I16), b.view(I16)), form
