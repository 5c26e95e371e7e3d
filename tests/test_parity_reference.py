"""CPU checks of tests/parity_ref.py (no GPU): the case tables' helper
conditions, a CPU fp32 emulation of each contract under its own bar, and the
sharpness of the two checks the GPU tests make.

Mutants (plausible kernel slips, parity_ref.MUTANTS) and what catches them:
  exact   every mutant changes the stored bytes on the exact operands (asserted
          for each, in the three- and the four-product form);
  bar     random operands under the rounding bar.  A mutant whose float64 effect
          passes 2 x bar somewhere MUST fail (the emulation's own error is at most
          one bar); that is asserted for whichever mutants reach it, and always
          for the hi/lo swap, which leaves hi + lo unchanged and is caught by the
          pair rule |lo| <= 2^-8 |hi|.  A truncated lo and the other number of
          products sit inside the bar at every K -- only the exact check catches
          them; the three dropped-term mutants pass the bar where K is small (a
          1x1 conv) and sit inside it at 3x3 x 128 channels.
"""
import pytest
import torch

import parity_ref as P

TILED = P.tiled_cases()
SPLIT_TABLE = {**{f'gemm {n}': c for n, c in P.GEMM_SHAPES.items()},
               **{f'four {n}': c for n, (c, _) in P.FOUR_SHAPES.items()},
               **{f'tiled {n}': c for n, (c, _, _) in TILED.items()}}


def test_layout_helpers_match_the_engine():
    from sad.engine import from_split, to_split
    g = torch.Generator().manual_seed(1)
    t = torch.randn(3, 5, 96, generator=g)
    hi, lo = P.parts(t)
    assert torch.equal(P.interleave(hi, lo).view(torch.int16), to_split(t).view(torch.int16))
    assert torch.equal(hi + lo, from_split(to_split(t)))
    h2, l2 = P.halves(to_split(t))
    assert torch.equal(h2.float(), hi) and torch.equal(l2.float(), lo)


def test_tables_cover_every_split_variant():
    tiled = {v for (_, v, _) in TILED.values()}
    assert tiled == {20, 26, 30, 31, 42, 44} and set(P.SPLIT_DEFAULTS) <= tiled
    assert set(P.GEMM_VARIANTS) == {0, *range(9, 20)}
    assert {v for (_, v) in P.FOUR_SHAPES.values()} == set(P.FOUR_VARIANTS)
    assert len(TILED) == len(P.TILED_FORMS) * len(P.TILED_MAPS) + len(P.MANY_FORMS)
    for name, c in P.GEMM_SHAPES.items():      # every shape runs on some variant and variant 13 takes every res
        ok = [v for v in P.GEMM_VARIANTS if P.gemm_refusal(v, c) is None]
        assert len(ok) >= 2, name
    for v in range(9, 20):
        assert any(P.gemm_refusal(v, c) is None for c in P.GEMM_SHAPES.values())
        assert any(P.gemm_refusal(v, c) is not None for c in P.GEMM_SHAPES.values())


@pytest.mark.parametrize('name', list(P.GEMM_SHAPES))
def test_fp32_exact_operands(name):
    c = P.GEMM_SHAPES[name]
    x, w, bias, sc, res = P.exact_operands_f32(P.generator('exact32', name), c)
    ref, _, _ = P.fp32_contract(c, x, w, bias, sc, res)
    nz = (ref != 0).double().mean().item()
    print(f'CONDITIONS fp32 {name}: non-zero {nz:.2f}, max |ref| {ref.abs().max().item():.0f}')
    assert torch.equal(ref, ref.round()) and ref.abs().max().item() < 2 ** 24 and nz >= 0.25
    assert torch.equal(P.emulate_fp32(c, x, w, bias, sc, res).double(), ref)


@pytest.mark.parametrize('name', list(SPLIT_TABLE))
def test_split_exact_operands(name):
    c = SPLIT_TABLE[name]
    ops = P.exact_operands_split(P.generator('exact', name), c)
    fig, e3, e4 = P.exact_conditions(c, *ops)
    print(f'CONDITIONS split {name}: ' + ', '.join(f'{k} {v:.3g}' if isinstance(v, float) else f'{k} {v}'
                                                  for k, v in fig.items()))
    P.check_conditions(fig)
    # the term-by-term fp32 emulation reproduces both expectations bit for bit
    for four, e in ((False, e3), (True, e4)):
        assert not P.differing(P.emulate_split(c, *ops, four=four), e).any()


EMU_CASES = {**{f'gemm {n}': c for n, c in P.GEMM_SHAPES.items()},
             **{f'four {n}': c for n, (c, _) in P.FOUR_SHAPES.items()},
             **{f'tiled {n}': c for n, (c, _, s) in TILED.items() if n.endswith('1x16x32')}}


@pytest.mark.parametrize('name', list(EMU_CASES))
def test_emulations_sit_under_their_bars(name):
    c = EMU_CASES[name]
    ratios = {}
    if name.startswith('gemm'):
        ops = P.random_operands(P.generator('random32', name), c, post_relu=False)
        ref, bar, zero = P.fp32_contract(c, *ops)
        ratios['fp32'] = P.worst_ratio(P.emulate_fp32(c, *ops), ref, bar, zero)
    ops = P.random_operands(P.generator('random', name), c, post_relu=True)
    for four in (False, True):
        ref, bar, zero, _ = P.split_contract(c, *ops, four=four)
        ratios['four' if four else 'three'] = P.split_ratio(P.emulate_split(c, *ops, four=four), ref, bar, zero)
    print(f'RATIO emulation {name}: ' + ', '.join(f'{k} {v:.3g}' for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


MUTANT_CASES = {'four c3 1x1 res 128-256 v13': P.FOUR_SHAPES['c3 1x1 res 128-256 v13'][0],
                'tiled 20 c128 res 1x16x32': TILED['20 c128 res 1x16x32'][0]}


@pytest.mark.parametrize('four', [False, True], ids=['three', 'four'])
@pytest.mark.parametrize('name', list(MUTANT_CASES))
def test_every_mutant_is_caught(name, four):
    c = MUTANT_CASES[name]
    exact = P.exact_operands_split(P.generator('exact', name), c)
    _, e3, e4 = P.exact_conditions(c, *exact)
    want = e4 if four else e3
    rnd = P.random_operands(P.generator('random', name), c, post_relu=True)
    ref, bar, zero, _ = P.split_contract(c, *rnd, four=four)
    for m in P.MUTANTS:
        n_exact = int(P.differing(P.emulate_split(c, *exact, four=four, mutant=m), want).sum())
        r32 = P.split_ratio(P.emulate_split(c, *rnd, four=four, mutant=m), ref, bar, zero)
        effect = P.split_ratio(P.emulate_split(c, *rnd, four=four, mutant=m, dtype=torch.float64), ref, bar, zero)
        by = [k for k, hit in (('exact', n_exact > 0), ('bar', r32 > 1.0)) if hit]
        print(f'MUTANT {name} {"four" if four else "three"} | {m}: {n_exact} stored outputs differ on the exact '
              f'operands; random operands |d|/bar {r32:.3g} (float64 effect {effect:.3g}) -> caught by '
              f'{" and ".join(by) or "NOTHING"}')
        assert n_exact > 0, m
        if effect > 2.0 or m == P.MUTANTS[5]:
            assert r32 > 1.0, m
