"""GPU: the tuned ResNet-18 plan and the generic BasicBlock plan run the same
blocks.  Both fold a BasicBlock with fold_basic_block and issue its launches
with run_basic_block (csrc/basicblock.hip), so the generic plan built as
'resnet18' must give the ResNet-18 plan's pooled features bit for bit.

The ResNet-18 side is the debug entry: like the generic plan it ends in the
plain average pool (the normal run fuses the pool into the last conv and sums
in another order, so it is not part of this test).

Weights: the hash PRNG's 'n6' backbone with tests/golden/bn_stats_n6.npz;
inputs: seeded normal maps [B, 128, 251]."""
import pytest
import torch

from conftest import merged_sd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = ['fp32', 'bf16', 'bf16x3']


@pytest.fixture(scope='module')
def base_sd():
    from sad.engine import split_merged_state
    return split_merged_state(merged_sd('n6'))[1][0]


@pytest.fixture(scope='module')
def maps5():
    g = torch.Generator().manual_seed(11)
    return torch.randn(5, 128, 251, generator=g).to(DEV).contiguous()


@pytest.mark.parametrize('dtype', DTYPES)
def test_generic_plan_equals_resnet18_plan(base_sd, maps5, dtype):
    from sad.engine import Backbone, ResNetBackbone
    tuned = Backbone(base_sd, DEV, dtype)
    # B = 3: one chunk on both sides
    ref3 = tuned.debug(maps5[:3])[0]
    got3 = ResNetBackbone(base_sd, 'resnet18', DEV, dtype, micro_batch=3)(maps5[:3])
    # B = 5: the generic plan in chunks of 2 + 2 + 1 against one debug run of 5
    # (no launch's result depends on an image's neighbours in the batch)
    ref5 = tuned.debug(maps5)[0]
    got5 = ResNetBackbone(base_sd, 'resnet18', DEV, dtype, micro_batch=2)(maps5)
    torch.cuda.synchronize()
    assert torch.isfinite(ref5).all() and ref5.abs().max() > 0
    assert not torch.equal(ref5[0], ref5[1])
    assert torch.equal(got3, ref3), (got3 - ref3).abs().max().item()
    assert torch.equal(got5, ref5), (got5 - ref5).abs().max().item()
