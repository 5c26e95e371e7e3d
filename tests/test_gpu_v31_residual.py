"""Variant 31 (halo256r.hip): the identity shortcut as an fp32 epilogue residual.

The bf16 identity blocks of layer3/4 hand the block input to variant 31 as
``res``: the epilogue adds it in fp32 to the accumulators the wave holds,
out = bf16(relu(acc + x)) (the pooled form sums relu(acc + x)), instead of
multiplying it by an identity matrix as K columns.  A residual tile is one
16-B load per lane for two tile rows of a 16-channel group, in the store
layout, addressed through the tile's pixel and the wave's channels.

Every case has more tiles than workgroups (some workgroups run two tiles, so
the accumulator re-initialisation and the residual addressing cross a tile
boundary):

  res-l3    N = 70, 32 x 32, 256 -> 256: 280 pixel tiles over 256 workgroups
  res-2tc   N = 140, 16 x 16, 256 -> 512: two channel tiles (the residual's
            channel offset is not 0), 140 pixel tiles over 128 workgroup pairs
  res-c128  N = 20, 64 x 64, 128 -> 128: the 128-channel tile form (two pixel
            halves per channel group), 320 tiles
  res-l3 also runs with relu=False.

Checks:
  * values: |out - ref| <= 2^-8 |ref| + 1e-2 against F.conv2d on the
    bf16-rounded operands in fp32, + bias + res, clamped
    (tests/test_gpu_kstep_parity.py's bar);
  * position invariance: one more image in front, images 1..N bit for bit;
  * against the K-column form of the same kernel (sc=res, weights with an
    appended identity): both are one bf16 rounding of fp32 sums that differ at
    most in their last bits, so |a - b| <= 2^-7 max(|a|, |b|) + 1e-5 (one bf16
    ulp); the share of elements that differ at all is printed;
  * pooled form: the features of the backbone run (fused pool with the
    residual) against the debug run's (layer4 map stored as bf16, then the pool
    kernel) on 3 seeded maps: |d| <= 2^-8 feature + 1e-6 (each pooled value
    rounded once to bf16 is 2^-9 relative; the factor 2 covers summation order);
  * the split-bf16 form with ``res`` on variant 31 is an argument error and
    launches nothing;
  * past the 2 GiB buffer range: 4,200 images of 32 x 32 x 256 (input, residual
    and output 2.2 GB each) run as image-range launches, each with its own
    residual base and ``res_bytes``; the result equals, bit for bit, the two
    halves run on their own (tests/test_gpu_large_batch.py's check), on the
    default variant for this shape, which must be 31.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from conftest import merged_sd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# name: N, H, Cin, Cout, relu
CASES = {
    'res-l3': (70, 32, 256, 256, True),
    'res-2tc': (140, 16, 256, 512, True),
    'res-c128': (20, 64, 128, 128, True),
    'res-l3-norelu': (70, 32, 256, 256, False),
}


def test_case_table_has_more_tiles_than_workgroups():
    for name, (N, H, _, Cout, _) in CASES.items():
        n_tc = max(1, Cout // 256)
        tiles, groups = N * (H // 16) ** 2, 256 // n_tc
        assert groups < tiles < 2 * groups, name


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """N + 1 images (image 0 is the extra one in front), residual, weights
    [Cout, 9 Cin + Cout] with the identity appended, bias -- fp32 on the CPU.
    The relu=False case shares res-l3's tensors."""
    N, H, Cin, Cout, _ = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.split('-norelu')[0].encode()))
    x = torch.randn(N + 1, H, H, Cin, generator=g)
    res = torch.randn(N + 1, H, H, Cout, generator=g)
    K = 9 * Cin + Cout
    w = torch.randn(Cout, K, generator=g) * (2.0 / K) ** 0.5
    w[:, 9 * Cin:] = torch.eye(Cout)
    bias = torch.randn(Cout, generator=g) * 0.1
    return x, res, w, bias


@functools.lru_cache(maxsize=None)
def _preact(base):
    """conv + bias + res of images 1..N before the activation (computed once per
    tensor set, never changed)"""
    _, _, Cin, Cout, _ = CASES[base]
    x, res, w, bias = _inputs(base)
    xb, rb, wb = x.to(torch.bfloat16), res.to(torch.bfloat16), w.to(torch.bfloat16)
    wc = wb[:, :9 * Cin].float().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    return F.conv2d(xb[1:].float().permute(0, 3, 1, 2), wc, padding=1).permute(0, 2, 3, 1) + bias + rb[1:].float()


@functools.lru_cache(maxsize=None)
def _run(name):
    """(reference of images 1..N, residual-form output of images 1..N alone, of
    images 0..N, K-column-form output of images 1..N)"""
    from sad.engine import block_conv
    relu = CASES[name][4]
    x, res, w, bias = _inputs(name)
    xb, rb, wb = x.to(torch.bfloat16), res.to(torch.bfloat16), w.to(torch.bfloat16)
    ref = _preact(name.split('-norelu')[0])
    if relu:
        ref = ref.clamp_min(0)
    xd, rd, wd, bd = xb.to(DEV), rb.to(DEV), wb.to(DEV), bias.to(DEV)
    outs = []
    for lo in (1, 0):
        out = block_conv(xd[lo:].contiguous(), wd, bd, 1, 1, res=rd[lo:].contiguous(), relu=relu, variant=31)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    kcol = block_conv(xd[1:].contiguous(), wd, bd, 1, 1, sc=rd[1:].contiguous(), sc_stride=1, relu=relu, variant=31)
    torch.cuda.synchronize()
    return ref, outs[0], outs[1], kcol.cpu()


@pytest.mark.parametrize('name', list(CASES))
def test_values(name):
    ref, out, _, _ = _run(name)
    d = (out.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-2
    print(f'{name}: max |d| {d.max().item():.3g}, worst excess {(d - bound).max().item():.3g}')
    assert bool((d <= bound).all()), f'max |d| {d.max().item():.3g}, worst excess {(d - bound).max().item():.3g}'


@pytest.mark.parametrize('name', list(CASES))
def test_position_invariance(name):
    _, out, shifted, _ = _run(name)
    same = (out.view(torch.int16) == shifted[1:].view(torch.int16)).flatten(1).all(1)
    assert bool(same.all()), f'images that differ after the shift: {(~same).nonzero().flatten().tolist()[:20]}'


@pytest.mark.parametrize('name', list(CASES))
def test_matches_k_column_form(name):
    _, out, _, kcol = _run(name)
    a, b = out.float(), kcol.float()
    d = (a - b).abs()
    bound = torch.maximum(a.abs(), b.abs()) * 2.0 ** -7 + 1e-5
    share = (out.view(torch.int16) != kcol.view(torch.int16)).float().mean().item()
    print(f'{name}: residual vs K-column form: {share:.3e} of the elements differ, max |d| {d.max().item():.3g}')
    assert bool((d <= bound).all()), f'max |d| {d.max().item():.3g}, worst excess {(d - bound).max().item():.3g}'


def test_pooled_form_matches_stored_map_then_pool():
    from sad.engine import MAP_H, MAP_W, Backbone, split_merged_state
    _, bases, _ = split_merged_state(merged_sd('n6'))
    bb = Backbone(bases[0], DEV, 'bf16')
    maps = torch.randn(3, MAP_H, MAP_W, generator=torch.Generator().manual_seed(31)).to(DEV)
    fused = bb(maps)
    sep, _ = bb.debug(maps)
    torch.cuda.synchronize()
    fused, sep = fused.cpu(), sep.cpu()
    d = (fused - sep).abs()
    bound = fused.abs() * 2.0 ** -8 + 1e-6
    print(f'pooled: max |d| {d.max().item():.3g}, max feature {fused.abs().max().item():.3g}, '
          f'worst excess {(d - bound).max().item():.3g}')
    assert float(fused.abs().max()) > 0
    assert bool((d <= bound).all()), f'max |d| {d.max().item():.3g}, worst excess {(d - bound).max().item():.3g}'


def test_split_form_with_residual_is_an_argument_error():
    from sad.engine import block_conv, to_split
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 16, 16, 256, generator=g)
    res = torch.randn(2, 16, 16, 256, generator=g)
    w = torch.randn(256, 9 * 256, generator=g) * 0.02
    bias = torch.zeros(256)
    out = torch.full((2, 16, 16, 512), 7.0, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r'\(-1\).*variant 31'):
        block_conv(to_split(x).to(DEV), to_split(w).to(DEV), bias.to(DEV), 1, 1, res=to_split(res).to(DEV),
                   variant=31, split=True, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), 'the rejected call wrote to its output'


def test_residual_follows_image_range_launches():
    from sad.engine import block_conv
    N, H, C = 4200, 32, 256

    def rand(shape, seed, scale=1.0):
        g = torch.Generator(device=DEV).manual_seed(seed)
        return (torch.randn(shape, generator=g, device=DEV) * scale).to(torch.bfloat16)

    x, res = rand((N, H, H, C), 1), rand((N, H, H, C), 2)
    assert x.numel() * 2 > 2 ** 31
    w = rand((C, 9 * C), 3, (2.0 / (9 * C)) ** 0.5)
    b = torch.randn(C, device=DEV) * 0.1
    big = block_conv(x, w, b, 1, 1, res=res)
    half = N // 2
    parts = [block_conv(x[lo:hi], w, b, 1, 1, res=res[lo:hi], variant=31) for lo, hi in ((0, half), (half, N))]
    torch.cuda.synchronize()
    assert torch.equal(big, torch.cat(parts))
    assert big.float().abs().sum() > 0
