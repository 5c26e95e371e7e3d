"""Variants 31 / 44 (halo256r.hip, halo256rs2.hip): K-step state carried across
chunks and tiles.

Both kernels use two weight register sets in turn and two patch buffers (31) /
four parity planes (44), and a persistent workgroup runs its tiles back to
back, so whatever the K loop carries from one chunk to the next -- which set
holds the next step's weights, which buffer the next patch -- also crosses tile
boundaries.  tests/test_gpu_blockconv.py never combines an ODD number of K-steps
per tile with SEVERAL tiles per workgroup, the combination in which a carried
parity differs from tile to tile.  Every case here has more than 256 tiles (some
workgroups run two, some one); steps per tile = 9 per 64-channel conv chunk + 1
per 64-channel shortcut chunk:

  odd:   c192-31 27, ds64-31 37, l2ds-31 19 (128-channel tiles), c192-44 27
  even:  id-31 40, l4-44 36 (two channel tiles per pixel range)

Checks per case:
  * values: |out - ref| <= 2^-8 |ref| + 1e-2 against F.conv2d on the bf16-rounded
    operands (tests/test_gpu_blockconv.py's bar: one bf16 rounding of an fp32
    accumulation, plus the floor for summation order near zero);
  * position invariance: the same batch with one more random image in front
    gives, for images 1..N, the first run's output bit for bit -- every image
    then sits at another place of its workgroup's tile sequence and meets the
    other parity.
The split-bf16 form of c192-31 and l2ds-31 runs against a float64 conv with
tests/test_gpu_x3.py's bar (1e-4 of the output scale), and the same invariance.

The fused average pool of variant 31 (POOL) is not reachable through
block_conv; the backbone tests (test_gpu_parity.py, test_gpu_x3.py) cover it.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# name: N, H (input), Cin, Cout, stride, shortcut (None | 'id' | ('ds', channels of the 2x source)), variant
CASES = {
    'c192-31': (70, 32, 192, 256, 1, None, 31),
    'ds64-31': (70, 32, 256, 256, 1, ('ds', 64), 31),
    'l2ds-31': (20, 64, 128, 128, 1, ('ds', 64), 31),
    'c192-44': (70, 64, 192, 256, 2, None, 44),
    'id-31': (70, 32, 256, 256, 1, 'id', 31),
    'l4-44': (300, 32, 256, 512, 2, None, 44),
}
SPLIT_CASES = ['c192-31', 'l2ds-31']


def _steps(name):
    N, H, Cin, Cout, stride, sc, _ = CASES[name]
    cin1 = Cout if sc == 'id' else sc[1] if sc else 0
    return 9 * (Cin // 64) + cin1 // 64, N * (H // stride // 16) ** 2


def test_case_table_matches_its_description():
    want = {'c192-31': (27, 280), 'ds64-31': (37, 280), 'l2ds-31': (19, 320), 'c192-44': (27, 280),
            'id-31': (40, 280), 'l4-44': (36, 300)}
    assert {n: _steps(n) for n in CASES} == want


@functools.lru_cache(maxsize=None)
def _inputs(name, relu_in):
    """N + 1 images (image 0 is the extra one in front), shortcut source,
    weights [Cout, 9 Cin + Cin1], bias -- fp32 on the CPU."""
    N, H, Cin, Cout, stride, sc, _ = CASES[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    Ho = H // stride
    post = (lambda t: t.clamp_min(0)) if relu_in else (lambda t: t)
    x = post(torch.randn(N + 1, H, H, Cin, generator=g))
    scx, cin1, ss = None, 0, 1
    if sc == 'id':
        scx, cin1 = post(torch.randn(N + 1, Ho, Ho, Cout, generator=g)), Cout
    elif sc is not None:
        scx, cin1, ss = post(torch.randn(N + 1, 2 * Ho, 2 * Ho, sc[1], generator=g)), sc[1], 2
    K = 9 * Cin + cin1
    w = torch.randn(Cout, K, generator=g) * (2.0 / K) ** 0.5
    if sc == 'id':
        w[:, 9 * Cin:] = torch.eye(Cout)
    bias = torch.randn(Cout, generator=g) * 0.1
    return x, scx, ss, w, bias


def _conv_ref(x, scx, ss, w, bias, stride, dtype):
    cin = x.shape[3]
    wc = w[:, :9 * cin].to(dtype).reshape(w.shape[0], 3, 3, cin).permute(0, 3, 1, 2)
    y = F.conv2d(x.to(dtype).permute(0, 3, 1, 2), wc, stride=stride, padding=1)
    if scx is not None:
        w1 = w[:, 9 * cin:].to(dtype)
        y = y + F.conv2d(scx.to(dtype).permute(0, 3, 1, 2), w1[:, :, None, None], stride=ss)
    return (y + bias.to(dtype).view(1, -1, 1, 1)).clamp_min(0).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def _bf16_run(name):
    """(reference of images 1..N, output of images 1..N alone, output of images 0..N)"""
    from sad.engine import block_conv
    _, _, _, _, stride, _, variant = CASES[name]
    x, scx, ss, w, bias = _inputs(name, False)
    xb, wb = x.to(torch.bfloat16), w.to(torch.bfloat16)
    sb = scx.to(torch.bfloat16) if scx is not None else None
    ref = _conv_ref(xb[1:], sb[1:] if sb is not None else None, ss, wb, bias, stride, torch.float32)
    xd, wd, bd = xb.to(DEV), wb.to(DEV), bias.to(DEV)
    sd = sb.to(DEV) if sb is not None else None
    outs = []
    for lo in (1, 0):
        out = block_conv(xd[lo:].contiguous(), wd, bd, stride, 1, sc=sd[lo:].contiguous() if sd is not None else None,
                         sc_stride=ss, relu=True, variant=variant)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    return ref, outs[0], outs[1]


@pytest.mark.parametrize('name', list(CASES))
def test_values(name):
    ref, out, _ = _bf16_run(name)
    d = (out.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-2
    print(f'{name}: max |d| {d.max().item():.3g}, worst excess {(d - bound).max().item():.3g}')
    assert bool((d <= bound).all()), f'max |d| {d.max().item():.3g}, worst excess {(d - bound).max().item():.3g}'


@pytest.mark.parametrize('name', list(CASES))
def test_position_invariance(name):
    _, out, shifted = _bf16_run(name)
    same = (out.view(torch.int16) == shifted[1:].view(torch.int16)).flatten(1).all(1)
    assert bool(same.all()), f'images that differ after the shift: {(~same).nonzero().flatten().tolist()[:20]}'


@functools.lru_cache(maxsize=None)
def _split_run(name):
    from sad.engine import block_conv, from_split, to_split
    _, _, _, _, stride, _, variant = CASES[name]
    x, scx, ss, w, bias = _inputs(name, True)
    ref = _conv_ref(x[1:], scx[1:] if scx is not None else None, ss, w, bias, stride, torch.float64)
    wd, bd = to_split(w).to(DEV), bias.to(DEV)
    outs = []
    for lo in (1, 0):
        out = block_conv(to_split(x[lo:]).to(DEV), wd, bd, stride=stride, pad=1,
                         sc=to_split(scx[lo:]).to(DEV) if scx is not None else None, sc_stride=ss,
                         variant=variant, split=True)
        torch.cuda.synchronize()
        outs.append(out.cpu())
    return ref, from_split(outs[0]).double(), outs[0], outs[1]


@pytest.mark.parametrize('name', SPLIT_CASES)
def test_split_values(name):
    ref, got, _, _ = _split_run(name)
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f'{name} split: rel err {err:.3e}')
    assert err <= 1e-4, err


@pytest.mark.parametrize('name', SPLIT_CASES)
def test_split_position_invariance(name):
    _, _, out, shifted = _split_run(name)
    same = (out.view(torch.int16) == shifted[1:].view(torch.int16)).flatten(1).all(1)
    assert bool(same.all()), f'images that differ after the shift: {(~same).nonzero().flatten().tolist()[:20]}'
