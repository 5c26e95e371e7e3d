"""CPU: the host side of shared-trunk ensembles -- ``model_merger.py
--keep-backbone`` (strict load of the trained backbone instead of quirk C2),
the engine's trunk/tail grouping on fabricated state dicts, and the argument
checks of the new libsad entries (no device work)."""
import csv

import pytest
import torch


def _trainer_checkpoints(tmp_path, name, files):
    """Trainer-format checkpoints: unprefixed timm keys + head.* (as tests/test_merger.py)."""
    from oracle import resnet as ores
    torch.manual_seed(321)
    sds = {}
    for fn in files:
        tr = ores.create_model(name)
        tr.head = ores.make_head(tr.num_features)
        for m in tr.modules():  # non-trivial BN buffers, counters included
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.running_mean.normal_()
                m.running_var.uniform_(0.5, 2.0)
                m.num_batches_tracked.fill_(7)
        sds[fn] = {k: v.detach().clone() for k, v in tr.state_dict().items()}
        torch.save({'epoch': 0, 'state_dict': tr.state_dict(), 'best_acc': 50.0}, tmp_path / fn)
    with open(tmp_path / 'm.csv', 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(['model_filename', 'synthetic_class', 'real_class'])
        w.writerows([(fn, f'Syn{i}', 'Real') for i, fn in enumerate(files)])
    return sds


def _merge(tmp_path, *extra):
    import model_merger as mm
    out = tmp_path / 'merged.pth'
    names = mm.main(['--submodels-folder', str(tmp_path), '--csv-file', str(tmp_path / 'm.csv'),
                     '--output-path', str(out), *extra])
    return names, torch.load(out, map_location='cpu', weights_only=True)


@pytest.mark.parametrize('name', ['resnet18', 'resnet50'])
def test_keep_backbone_keeps_every_trained_tensor(tmp_path, name):
    files = ['m1.pth', 'm2.pth']
    sds = _trainer_checkpoints(tmp_path, name, files)
    names, ck = _merge(tmp_path, '--keep-backbone', '--model-name', name)
    assert names == ['Syn0', 'Syn1', 'Real']
    assert sorted(ck.keys()) == ['metadata', 'state_dict'] and ck['metadata'] == {'class_names': names}
    sd = ck['state_dict']
    n_base = 0
    for i, fn in enumerate(files):
        for k, v in sds[fn].items():
            big = f'sub_models.{i}.' + (k if k.startswith('head.') else f'base.{k}')
            assert torch.equal(sd[big], v) and sd[big].dtype == v.dtype, big
            n_base += not k.startswith('head.')
    assert len(sd) == sum(len(s) for s in sds.values()) and n_base > 0
    assert int(sd['sub_models.1.base.layer3.0.bn1.num_batches_tracked']) == 7


def test_keep_backbone_output_format_equals_default(tmp_path):
    """Same keys, shapes and dtypes with and without the flag; the default is
    still quirk C2 (heads from the checkpoints, one constructor backbone)."""
    files = ['m1.pth', 'm2.pth']
    sds = _trainer_checkpoints(tmp_path, 'resnet18', files)
    _, ck0 = _merge(tmp_path)
    _, ck1 = _merge(tmp_path, '--keep-backbone')
    assert list(ck0['state_dict']) == list(ck1['state_dict'])
    for k, v in ck0['state_dict'].items():
        assert v.shape == ck1['state_dict'][k].shape and v.dtype == ck1['state_dict'][k].dtype, k
    sd0 = ck0['state_dict']
    assert torch.equal(sd0['sub_models.1.head.10.bias'], sds['m2.pth']['head.10.bias'])
    assert not torch.equal(sd0['sub_models.0.base.conv1.weight'], sds['m1.pth']['conv1.weight'])
    assert torch.equal(sd0['sub_models.0.base.conv1.weight'], sd0['sub_models.1.base.conv1.weight'])


def test_keep_backbone_loads_base_form_as_it_is(tmp_path):
    import model_merger as mm
    sds = _trainer_checkpoints(tmp_path, 'resnet18', ['m1.pth'])
    based = mm.to_base_keys(sds['m1.pth'])
    assert 'base.conv1.weight' in based and 'head.2.weight' in based
    torch.save({'state_dict': based}, tmp_path / 'b.pth')
    got = mm.load_sub_model(str(tmp_path / 'b.pth'), 'cpu', keep_backbone=True).state_dict()
    assert set(got) == set(based)
    for k, v in based.items():
        assert torch.equal(got[k], v), k


@pytest.mark.parametrize('drop', ['layer3.0.bn1.running_var', 'layer2.1.bn2.num_batches_tracked', 'head.7.bias'])
def test_keep_backbone_names_a_missing_key(tmp_path, drop):
    import model_merger as mm
    sds = _trainer_checkpoints(tmp_path, 'resnet18', ['m1.pth'])
    sd = dict(sds['m1.pth'])
    del sd[drop]
    torch.save({'state_dict': sd}, tmp_path / 'cut.pth')
    want = drop if drop.startswith('head.') else f'base.{drop}'
    with pytest.raises(RuntimeError, match=want.replace('.', r'\.')):
        mm.load_sub_model(str(tmp_path / 'cut.pth'), 'cpu', keep_backbone=True)
    mm.load_sub_model(str(tmp_path / 'cut.pth'), 'cpu')  # the default (strict=False) still loads it


def test_merger_arguments_without_the_flag(tmp_path, capsys):
    import model_merger as mm
    with pytest.raises(SystemExit):
        mm.main(['--csv-file', 'x.csv', '--output-path', 'y.pth'])  # --submodels-folder is required
    with pytest.raises(SystemExit):
        mm.main(['--submodels-folder', '.', '--csv-file', 'x.csv', '--output-path', 'y.pth', '--keep-backbones'])
    capsys.readouterr()
    (tmp_path / 'e.csv').write_text('model_filename,synthetic_class,real_class\n')
    assert mm.main(['--submodels-folder', str(tmp_path), '--csv-file', str(tmp_path / 'e.csv'),
                    '--output-path', str(tmp_path / 'x.pth')]) is None


# ---------------------------------------------------------------- grouping ----
def _base(seed):
    from sad import weights as sw
    return {k: v.clone() for k, v in sw.backbone_state_dict(seed).items()}


def _with_tail(trunk, tail):
    return {k: (tail[k] if k.startswith('layer4.') else trunk[k]).clone() for k in trunk}


def test_grouping_all_identical():
    from sad.engine import group_backbones
    g = group_backbones([_base(0) for _ in range(4)])
    assert g.feat_index == [0, 0, 0, 0] and g.first == [0] and g.trunk_of == [0] and g.shared == []
    assert (g.n_backbones, g.n_trunks) == (1, 1)


def test_grouping_all_distinct():
    from sad.engine import group_backbones
    g = group_backbones([_base(s) for s in range(4)])
    assert g.feat_index == [0, 1, 2, 3] and g.first == [0, 1, 2, 3] and g.trunk_of == [0, 1, 2, 3]
    assert g.shared == [] and (g.n_backbones, g.n_trunks) == (4, 4)


def test_grouping_one_trunk_three_tails_one_duplicated():
    from sad.engine import group_backbones
    a, b = _base(0), _base(1)
    subs = [a, _with_tail(a, b), a]  # sub-model 2 duplicates sub-model 0's tail
    g = group_backbones(subs)
    assert g.feat_index == [0, 1, 0] and g.first == [0, 1] and g.trunk_of == [0, 0] and g.shared == [[0, 1]]
    assert g.describe() == '3 sub-models: 1 trunk, 2 tails'
    # a fully distinct sub-model in the middle keeps first-appearance order
    g = group_backbones([a, b, _with_tail(a, b), a])
    assert g.feat_index == [0, 1, 2, 0] and g.first == [0, 1, 2] and g.trunk_of == [0, 1, 0]
    assert g.shared == [[0, 2]] and g.describe() == '4 sub-models: 2 trunks, 3 tails'


def test_grouping_running_var_splits_and_counter_does_not():
    from sad.engine import group_backbones
    a, b = _base(0), _base(1)
    other = _with_tail(a, b)
    g = group_backbones([a, other])
    assert g.shared == [[0, 1]] and g.n_trunks == 1
    moved = {k: v.clone() for k, v in other.items()}
    moved['layer3.1.bn2.running_var'][5] += 1e-3
    g = group_backbones([a, moved])
    assert g.shared == [] and g.n_trunks == 2 and g.feat_index == [0, 1]
    counted = {k: v.clone() for k, v in other.items()}
    for k in counted:
        if k.endswith('num_batches_tracked'):
            counted[k] = torch.tensor(123, dtype=torch.long)
    g = group_backbones([a, counted])
    assert g.shared == [[0, 1]] and g.n_trunks == 1
    g = group_backbones([other, counted])  # counters alone: one backbone
    assert g.feat_index == [0, 0] and g.shared == []


# ------------------------------------------------------------------- ABI ----
def test_new_entries_reject_null_arguments_without_gpu():
    from sad import _lib
    lib = _lib.load()
    sz = _lib.SZ()
    assert lib.sad_backbone_trunk_run(None, None, None, 1, 1, None, None, 0, None) == -1
    assert b'null' in lib.sad_last_error()
    assert lib.sad_backbone_tail_run(None, None, 1, 1, None, None, 0, None) == -1
    assert b'null' in lib.sad_last_error()
    assert lib.sad_backbone_shared_workspace_size(None, 1, _lib.ctypes.byref(sz)) == -1
    assert lib.sad_backbone_shared_run(None, None, 0, None, None, 1, 1, None, None, 0, None) == -1
    assert b'null' in lib.sad_last_error()
    with pytest.raises(RuntimeError, match='libsad'):
        _lib.call('sad_backbone_tail_run', None, None, 1, 1, None, None, 0, None)
