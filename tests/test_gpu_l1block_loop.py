"""GPU: the fused layer1 block's tile loop (csrc/l1block.hip, variant 40) --
the incremental tile walk, the tabled patch pieces and the two kernel
instantiations (production / timing ablations).  Operands and bars as
tests/test_gpu_l1block.py.

* walk and edges: against the unfused variant-25 path (1 bf16 ulp of |ref| +
  1e-2, at most 1 % of the outputs differing at all) and the torch fp32
  reference (same bar), on shapes where no tile continues a strip, every tile
  but the first does, workgroups hold 1 or 2 tiles with every piece partly
  outside the image, and ranges start and end mid-strip;
* position invariance: an image gives the same bytes inside a batch as alone.
  Whether a tile's top halo is computed (strip start, workgroup range start)
  or copied from the tile above depends on where the workgroup ranges fall;
  both forms sum a fragment's K-steps in the same order, so the bits must not
  depend on it;
* dispatch: ablate = 0 runs the production kernel and is unaffected by
  ablated launches around it (their values are wrong by design and not
  looked at).
"""
import pytest
import torch

from test_gpu_l1block import DEV, _fused, _operands, _torch_ref, _unfused

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 64), (1, 256, 16), (257, 16, 16), (3, 48, 32), (37, 128, 128)]
_cache = {}


def _case(N, H, W):
    """operands and the fused output of a shape, computed once"""
    k = (N, H, W)
    if k not in _cache:
        ops = _operands(N, H, W, 31 * N + H + 7 * W)
        out = _fused(*ops)
        torch.cuda.synchronize()
        _cache[k] = (ops, out)
    return _cache[k]


@pytest.mark.parametrize('N,H,W', SHAPES)
def test_walk_matches_unfused(N, H, W):
    ops, out = _case(N, H, W)
    ref = _unfused(*ops)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    d = (out.float() - ref.float()).abs()
    bound = ref.float().abs() * 2.0 ** -8 + 1e-2
    nd = (out != ref).sum().item()
    print(f'{N}x{H}x{W}: max |d| {d.max().item():.3g}, {nd} of {out.numel()} differ')
    assert bool((d <= bound).all()), f'max |d| {d.max().item():.3g}'
    assert nd <= out.numel() // 100, f'{nd} of {out.numel()} outputs differ'


@pytest.mark.parametrize('N,H,W', SHAPES)
def test_walk_vs_torch_fp32(N, H, W):
    ops, out = _case(N, H, W)
    ref = _torch_ref(*ops)
    d = (out.float() - ref).abs()
    bound = ref.abs() * 2.0 ** -8 + 1e-2
    print(f'{N}x{H}x{W}: max |d| {d.max().item():.3g}')
    assert bool((d <= bound).all()), f'max |d| {d.max().item():.3g}'


@pytest.mark.parametrize('N,H,W,picks', [(37, 128, 128, (0, 17, 36)), (5, 64, 80, (0, 2, 4))])
def test_position_invariance_bit_for_bit(N, H, W, picks):
    (x, w1, b1, w2, b2), out = _case(N, H, W)
    for i in picks:
        alone = _fused(x[i:i + 1].contiguous(), w1, b1, w2, b2)
        torch.cuda.synchronize()
        assert torch.equal(alone[0].view(torch.int16), out[i].view(torch.int16)), f'image {i}'


def test_instantiation_dispatch():
    from sad import _lib
    x, w1, b1, w2, b2 = _operands(2, 48, 32, 99)
    N, H, W, _ = x.shape
    s = _lib.stream_handle(torch.device(DEV))
    buf = torch.empty_like(x)
    zeros = []
    for ab in (0, 1, 2, 4, 7, 0):
        # (_lib.call raises on any status but SAD_OK)
        _lib.call('sad_l1_block_run', _lib.ptr(x), N, H, W, _lib.ptr(w1), 576, _lib.ptr(b1), _lib.ptr(w2), 640,
                  _lib.ptr(b2), _lib.ptr(buf), ab, s)
        torch.cuda.synchronize()
        if ab == 0:
            zeros.append(buf.clone())
    fresh = _fused(x, w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert torch.equal(zeros[0].view(torch.int16), zeros[1].view(torch.int16))
    assert torch.equal(zeros[0].view(torch.int16), fresh.view(torch.int16))
