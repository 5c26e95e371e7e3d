"""GPU: the layer2 resident-weight conv's tile loop (csrc/l2conv.hip, variant
41) -- the stepped tile origin, the tabled patch pieces and their edge masks,
the one-constant residual / downsample pieces and the kernel dispatch.

Operands, the fp32 torch reference and the bar are tests/test_gpu_blockconv.py's:
|out - ref| <= 2^-8 |ref| + 1e-2 on every element (fp32 accumulation, one
rounding to bf16, summation-order noise near zero).

* walk and edges: the three forms (plain, epilogue residual, downsample) at
  (N, H, W) = (1,16,16) one tile with all four edges; (1,16,64) and (1,64,16)
  one tile row / column; (3,48,32) every edge class, ranges that end mid-row;
  (257,16,16) one tile per image and more tiles than workgroups, so every step
  changes image; (5,48,48) 45 tiles on 256 workgroups.  (3,48,32) also without
  the ReLU, which the kernel applies as a floor decided once per launch;
* position invariance: an image gives the same bytes inside a batch as alone;
* dispatch: launches of the timing-ablation kernels (variant | ablate << 8)
  return without error, and ablate = 0 launches before and after them give
  identical bytes.
"""
import functools
import zlib

import pytest
import torch

from test_gpu_blockconv import _check, _ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMS = ('plain', 'res', 'ds')
SHAPES = [(1, 16, 16), (1, 16, 64), (1, 64, 16), (3, 48, 32), (257, 16, 16), (5, 48, 48)]


@functools.lru_cache(maxsize=None)
def operands(form, N, H, W):
    """(x, w, bias, sc, res) on the host, bf16 (bias fp32), seeded by the case"""
    g = torch.Generator().manual_seed(zlib.crc32(f'{form}-{N}-{H}-{W}'.encode()))
    sc = res = None
    cin1 = 0
    if form == 'ds':
        sc = torch.randn(N, 2 * H, 2 * W, 64, generator=g).to(torch.bfloat16)
        cin1 = 64
    elif form == 'res':
        res = torch.randn(N, H, W, 128, generator=g).to(torch.bfloat16)
    x = torch.randn(N, H, W, 128, generator=g).to(torch.bfloat16)
    K = 9 * 128 + cin1
    w = (torch.randn(128, K, generator=g) * (2.0 / K) ** 0.5).to(torch.bfloat16)
    bias = torch.randn(128, generator=g) * 0.1
    return x, w, bias, sc, res


@functools.lru_cache(maxsize=None)
def reference(form, N, H, W, relu):
    x, w, bias, sc, res = operands(form, N, H, W)
    return _ref(x, w, bias, 1, sc, 2, res, relu)


def launch(form, N, H, W, relu=True, variant=41, images=None):
    """variant 41 on the case's operands (images: a subset of the batch)"""
    from sad.engine import block_conv
    x, w, bias, sc, res = operands(form, N, H, W)
    pick = (lambda t: t) if images is None else (lambda t: t[images].contiguous())
    out = block_conv(pick(x).to(DEV), w.to(DEV), bias.to(DEV), 1, 1, sc=pick(sc).to(DEV) if sc is not None else None,
                     sc_stride=2 if sc is not None else 1, relu=relu, variant=variant,
                     res=pick(res).to(DEV) if res is not None else None)
    torch.cuda.synchronize()
    return out


def cases():
    """(form, N, H, W, relu) of the walk-and-edges cases (tools/l2bench.py --digest hashes their outputs)"""
    out = [(f, *s, True) for f in FORMS for s in SHAPES]
    return out + [(f, 3, 48, 32, False) for f in FORMS]


@pytest.mark.parametrize('form,N,H,W,relu', cases(), ids=[f'{c[0]}-{c[1]}x{c[2]}x{c[3]}{"" if c[4] else "-norelu"}'
                                                          for c in cases()])
def test_walk_and_edges(form, N, H, W, relu):
    out = launch(form, N, H, W, relu)
    _check(out.cpu(), reference(form, N, H, W, relu))


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('N,H,W,images', [(37, 64, 64, (0, 17, 36)), (5, 48, 32, (0, 2, 4))],
                         ids=['37x64x64', '5x48x32'])
def test_position_invariance(form, N, H, W, images):
    batch = launch(form, N, H, W)
    for b in images:
        alone = launch(form, N, H, W, images=[b])
        assert torch.equal(alone[0].view(torch.int16), batch[b].view(torch.int16)), f'image {b}'


@pytest.mark.parametrize('form', FORMS)
def test_ablation_dispatch(form):
    N, H, W = 3, 48, 32
    before = launch(form, N, H, W)
    for ab in (8, 32, 40):
        launch(form, N, H, W, variant=41 | (ab << 8))  # returns without error; the values are not looked at
    after = launch(form, N, H, W)
    fresh = launch(form, N, H, W)
    assert torch.equal(before.view(torch.int16), after.view(torch.int16))
    assert torch.equal(before.view(torch.int16), fresh.view(torch.int16))
    _check(after.cpu(), reference(form, N, H, W, True))
