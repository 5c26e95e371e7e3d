"""GPU: ``submodel_trainer.py --trunk CHECKPOINT`` (sad.train.FrozenTrunkNet).

conv1, bn1 and layer1-3 come from CHECKPOINT and run in eval mode on the
inference plan's trunk entry; layer4 trains on the existing kernels.  The
reference of a step is oracle.train.build's model with those modules put in
``.eval()`` (running statistics normalise, nothing in them is updated), under
the bars tests/test_gpu_train.py applies to the ordinary step:

  loss relative <= 1e-4; total grad norm relative <= 1e-3; clipped layer4
  gradients per tensor norm-relative <= ``_bar`` (5e-3, BN biases 8e-3);
  parameters after AdamW |d| <= 1e-6 + 1e-2 * lr where the oracle's gradient is
  not negligible; layer4 BN running statistics relative <= 1e-4;
  bf16: finite loss, layer4 gradient cosine vs the fp32 oracle >= 0.98.

The trunk's parameters, running statistics and counters must come out of the
step, and of ``unfreeze_layer3()``, bit for bit as CHECKPOINT has them.  End to
end: two sub-models trained from one trunk, merged with ``--keep-backbone``,
load as one trunk under two tails and match the oracle within 1e-3."""
import csv
import logging
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from test_gpu_train import _bar, _oracle_inputs, _rel, _waves

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TRUNK_MODULES = ('conv1', 'bn1', 'layer1', 'layer2', 'layer3')


@pytest.fixture(scope='module')
def setup():
    """(initial backbone, head, trunk CHECKPOINT state dict): the trunk is the
    'n6d' fixture's sub-model 0 (seed 2, calibrated BN statistics), counters set
    to a value a trained checkpoint would carry."""
    from sad import train as st
    from sad import weights as sw
    base = sw.backbone_state_dict(7)
    _, head = st.init_state_dict(42)
    sd = sw.merged_state_dict(2, 1, True, bn_stats=sw.load_bn_stats(os.path.join(GOLDEN, 'bn_stats_n6d.npz')))
    ck = {k[len('sub_models.0.base.'):]: v.clone() for k, v in sd.items() if k.startswith('sub_models.0.base.')}
    for k in ck:
        if k.endswith('num_batches_tracked'):
            ck[k] = torch.tensor(11, dtype=torch.long)
    return base, head, ck


def _oracle(base, head, ck, lr):
    from oracle import train as otr
    from sad import train as st
    both = dict(base)
    for k in st.trunk_keys(base):
        both[k] = ck[k]
    return otr.build(both, head, lr=lr)


def _oracle_step(m, opt, x, targets):
    """oracle.train.train_step with the trunk modules in eval mode."""
    m.train()
    for name in TRUNK_MODULES:
        getattr(m.base, name).eval()
    opt.zero_grad()
    loss = torch.nn.CrossEntropyLoss()(m(x), targets)
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(m.parameters(), max_norm=0.5)
    opt.step()
    return loss.detach(), norm


def _assert_trunk_is(net, ck):
    from sad import train as st
    sd = net.base_state_dict()
    keys = st.trunk_keys(sd)
    assert len(keys) == len([k for k in sd if not k.startswith('layer4.')]) > 0
    for k in keys:
        assert sd[k].dtype == ck[k].dtype and torch.equal(sd[k], ck[k]), k


def test_frozen_trunk_step_fp32(setup):
    from sad.train import FrozenTrunkNet, Trainer, TrainFrontEnd
    base, head, ck = setup
    lr, n = 1e-3, 4
    img = TrainFrontEnd(DEV, 'fp32')(_waves(n).to(DEV))
    targets = torch.tensor([0, 1, 1, 0])
    tr = Trainer(base, head, DEV, 'fp32', lr=lr, trunk_sd=ck)
    assert isinstance(tr.net, FrozenTrunkNet)
    _assert_trunk_is(tr.net, ck)
    l4_before = {k: v.clone() for k, v in tr.net.base_state_dict().items() if k.startswith('layer4.')}
    for k, v in l4_before.items():  # layer4 is the seeded init's, not CHECKPOINT's
        assert torch.equal(v, base[k]), k
    m, opt = _oracle(base, head, ck, lr)
    loss, correct, tot, ok = tr.train_step(img, targets, n)
    torch.cuda.synchronize()
    assert ok and tot == n
    rloss, rnorm = _oracle_step(m, opt, _oracle_inputs(img), targets)
    norm = tr.last_norm.cpu()[0].item()
    print(f'frozen trunk fp32: loss {loss:.6f} vs {rloss.item():.6f}; norm {norm:.6f} vs {rnorm.item():.6f}')
    assert abs(loss - rloss.item()) <= 1e-4 * abs(rloss.item())
    assert abs(norm - rnorm.item()) <= 1e-3 * rnorm.item()
    for name, p in m.base.named_parameters():
        if not name.startswith('layer4.'):
            assert p.grad is None
            continue
        r = _rel(tr.net.grads[name].cpu(), p.grad)
        d = (tr.net.params[name].cpu() - p.detach()).abs()
        big = p.grad.abs() > 1e-3 * p.grad.abs().max()
        frac_bad = (d[big] > 1e-6 + 1e-2 * lr).float().mean().item() if big.any() else 0.0
        print(f'{name:32s} grad rel {r:.2e}  param mismatch frac {frac_bad:.2e}')
        assert r <= _bar(name), (name, r)
        assert frac_bad <= 1e-3, (name, frac_bad, d.max().item())
    sd = tr.net.base_state_dict()
    for k in ('layer4.0.bn1', 'layer4.0.downsample.1', 'layer4.1.bn2'):
        bn = m.base.get_submodule(k)
        r1, r2 = _rel(sd[f'{k}.running_mean'], bn.running_mean), _rel(sd[f'{k}.running_var'], bn.running_var)
        assert r1 <= 1e-4 and r2 <= 1e-4, (k, r1, r2)
        assert int(sd[f'{k}.num_batches_tracked']) == int(bn.num_batches_tracked) == 1
    for name in TRUNK_MODULES:  # the oracle's eval-mode trunk did not move either
        for k, v in getattr(m.base, name).state_dict().items():
            assert torch.equal(v, ck[f'{name}.{k}']), (name, k)
    _assert_trunk_is(tr.net, ck)
    # the epochs // 3 unfreeze has nothing to unfreeze; a further step leaves the trunk alone too
    assert tr.unfreeze_layer3() is False and not tr.layer3_unfrozen and tr.grads3 is None
    _assert_trunk_is(tr.net, ck)
    _, _, _, ok = tr.train_step(img, targets, n)
    assert ok
    _assert_trunk_is(tr.net, ck)
    full = tr.net.state_dict()  # the usual checkpoint format
    assert [k for k in full if k.startswith('head.')] and 'layer4.1.bn2.running_var' in full


def test_frozen_trunk_step_bf16(setup):
    from sad.train import Trainer, TrainFrontEnd
    base, head, ck = setup
    n = 4
    img = TrainFrontEnd(DEV, 'fp32')(_waves(n).to(DEV))  # the trunk plan reads fp32 images
    targets = torch.tensor([0, 1, 1, 0])
    tr = Trainer(base, head, DEV, 'bf16', trunk_sd=ck)
    m, opt = _oracle(base, head, ck, 1e-3)
    loss, _, _, ok = tr.train_step(img, targets, n)
    torch.cuda.synchronize()
    rloss, _ = _oracle_step(m, opt, _oracle_inputs(img), targets)
    assert ok and np.isfinite(loss)
    g = torch.cat([tr.net.grads[k].cpu().flatten() for k in tr.l4_names])
    gr = torch.cat([p.grad.flatten() for k, p in m.base.named_parameters() if k.startswith('layer4.')])
    cos = torch.nn.functional.cosine_similarity(g.double(), gr.double(), dim=0).item()
    print(f'frozen trunk bf16: loss {loss:.5f} vs {rloss.item():.5f}; layer4 gradient cosine {cos:.5f}')
    assert cos >= 0.98
    _assert_trunk_is(tr.net, ck)


def test_frozen_trunk_refuses_other_nets(setup):
    from sad.train import Trainer
    base, head, ck = setup
    with pytest.raises(ValueError, match='frozen trunk'):
        Trainer(base, head, DEV, 'mixed', trunk_sd=ck)
    cut = {k: v for k, v in ck.items() if k != 'layer2.0.bn1.running_mean'}
    with pytest.raises(KeyError, match='layer2.0.bn1.running_mean'):
        Trainer(base, head, DEV, 'fp32', trunk_sd=cut)


def _dataset(root):
    from sad import audio as sa
    from sad.synth import synth_labelled_clip
    k = 0
    for mode, n in (('train', 2), ('test', 1)):
        for label, cls in enumerate(('Real', 'Class1')):
            d = os.path.join(root, mode, cls)
            os.makedirs(d, exist_ok=True)
            for i in range(n):
                k += 1
                sa.save_pcm16(os.path.join(d, f'{cls}_{i}.wav'), synth_labelled_clip(3, k, label))


def test_two_submodels_on_one_trunk_merge_and_infer(tmp_path, monkeypatch, caplog, golden_frontend):
    import inference_runner as ir
    import model_merger as mm
    import submodel_trainer as smt
    from oracle import frontend as ofe
    from oracle import resnet as ores
    from sad import train as st
    monkeypatch.chdir(tmp_path)
    fe = st.TrainFrontEnd(DEV, 'fp32')
    img = fe(_waves(4).to(DEV))
    targets = torch.tensor([0, 1, 1, 0])

    def train(seed, trunk_sd, name):
        base, head = st.init_state_dict(seed)  # as submodel_trainer.main
        tr = st.Trainer(base, head, DEV, 'fp32', seed=seed, trunk_sd=trunk_sd)
        for _ in range(2):
            assert tr.train_step(img, targets, 4)[3]
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(tr.optimizer, mode='min', factor=0.5, patience=2)
        smt.save_checkpoint(str(tmp_path / 'ck' / name), 0, tr, sched, 50.0, 2)
        return torch.load(tmp_path / 'ck' / name, map_location='cpu', weights_only=True)['state_dict']

    first = train(42, None, 'first.pth')  # trained as today: its BN statistics moved
    assert int(first['layer2.0.bn1.num_batches_tracked']) == 2
    subs = [train(s, first, f'sub{s}.pth') for s in (1, 2)]
    for sd in subs:
        assert list(sd) == list(first)
        for k in st.trunk_keys(first):
            assert torch.equal(sd[k], first[k]), k
    assert not torch.equal(subs[0]['layer4.0.conv1.weight'], subs[1]['layer4.0.conv1.weight'])

    # the CLI path: --trunk through main(), across the epochs // 3 unfreeze
    _dataset(str(tmp_path / 'ds'))
    with caplog.at_level(logging.INFO):
        smt.main(['--data-dir', str(tmp_path / 'ds'), '--epochs', '3', '--batch-size', '2', '--workers', '0',
                  '--max-steps', '1', '--checkpoint-dir', str(tmp_path / 'cli'), '--precision', 'fp32',
                  '--trunk', str(tmp_path / 'ck' / 'first.pth'), '--seed', '5'])
    assert 'Skipped: layer3 belongs to the frozen trunk' in caplog.text
    cli = tmp_path / 'cli' / 'model_best.pth'
    if cli.exists():  # written only when the validation accuracy rose above 0
        sd = torch.load(cli, map_location='cpu', weights_only=True)['state_dict']
        for k in st.trunk_keys(first):
            assert torch.equal(sd[k], first[k]), k

    with open(tmp_path / 'm.csv', 'w', newline='') as f:
        wr = csv.writer(f)
        wr.writerow(['model_filename', 'synthetic_class', 'real_class'])
        wr.writerows([['sub1.pth', 'SynA', 'Real'], ['sub2.pth', 'SynB', 'Real']])
    merged = str(tmp_path / 'merged.pth')
    assert mm.main(['--submodels-folder', str(tmp_path / 'ck'), '--csv-file', str(tmp_path / 'm.csv'),
                    '--output-path', merged, '--keep-backbone']) == ['SynA', 'SynB', 'Real']
    model, meta = ir.load_merged_model(merged, torch.device(DEV), precision='fp32')
    g = model.engine.grouping
    assert (g.n_trunks, g.n_backbones) == (1, 2) and model.engine.shared_groups == [[0, 1]]
    assert g.describe() == '2 sub-models: 1 trunk, 2 tails'
    pcm = golden_frontend['pcm']
    out = model.forward_pcm(torch.from_numpy(pcm)).cpu()
    ref_model = ores.load_merged_state(torch.load(merged, map_location='cpu', weights_only=True)['state_dict'])
    with torch.no_grad():
        imgs = torch.cat([ofe.waveform_to_spectrogram(torch.from_numpy(pcm[i].astype(np.float32) / 32768.0), 32000,
                                                      ofe.SpectrogramConfig()) for i in range(4)])
        ref = ref_model(imgs)
    d = (out - ref).abs().max().item()
    print(f'two tails on one trained trunk, fp32: max|dlogit| vs oracle {d:.3e}')
    assert out.shape == (4, 3) and d <= 1e-3
