"""CPU: ``submodel_trainer.py --trunk CHECKPOINT`` is accepted for resnet18 in
bf16 or fp32 and refused, at argument time and with a message that says why,
for any other backbone or ``--precision mixed``; the frozen trunk's key set is
everything outside layer4."""
import pytest


def test_trunk_parses_and_defaults_off():
    import submodel_trainer as tr
    assert tr.parse_args([]).trunk == ''
    a = tr.parse_args(['--trunk', 'first/model_best.pth'])
    assert a.trunk == 'first/model_best.pth' and a.precision == 'bf16' and a.model_name == 'resnet18'
    a = tr.parse_args(['--trunk', 't.pth', '--precision', 'fp32', '--head-loss', '--seed', '7'])
    assert a.trunk == 't.pth' and a.precision == 'fp32' and a.head_loss and a.seed == 7


@pytest.mark.parametrize('extra,word', [(['--precision', 'mixed'], 'mixed'), (['--model-name', 'resnet34'], 'resnet34'),
                                        (['--model-name', 'resnet50'], 'resnet50')])
def test_trunk_refuses_what_the_plan_cannot_run(extra, word, capsys):
    import submodel_trainer as tr
    with pytest.raises(SystemExit) as e:
        tr.parse_args(['--trunk', 't.pth'] + extra)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert '--trunk needs' in err and word in err
    tr.parse_args(extra)  # fine without --trunk


def test_trunk_keys_are_everything_outside_layer4():
    from sad import train as st
    from sad import weights as sw
    sd = sw.backbone_state_dict(0)
    keys = st.trunk_keys(sd)
    assert set(keys) == {k for k in sd if not k.startswith('layer4.')}
    assert 'bn1.num_batches_tracked' in keys and 'layer3.1.bn2.running_var' in keys and 'conv1.weight' in keys


def test_trainer_docs_name_the_bottleneck_nets():
    import submodel_trainer as tr
    assert 'resnet50' in tr.__doc__ and 'Bottleneck' in tr.__doc__
