"""CPU: the fp16 mode's names and command-line choices (no device work)."""
import os
import re

import pytest

from conftest import ROOT


def test_header_and_binding_agree_on_sad_f16():
    from sad import _lib
    src = open(os.path.join(ROOT, 'include', 'sad.h')).read()
    body = re.search(r'enum sad_dtype \{(.*?)\n\};', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    vals = {k: int(v) for k, v in re.findall(r'(SAD_\w+)\s*=\s*(\d+)', body)}
    assert vals == {'SAD_F32': 0, 'SAD_BF16': 1, 'SAD_BF16X3': 2, 'SAD_F16': 3}
    assert _lib.SAD_F16 == 3 and _lib.DTYPES == {'fp32': 0, 'bf16': 1, 'bf16x3': 2, 'fp16': 3}
    flag = int(re.search(r'#define SAD_L1_BLOCK_F16 (0x[0-9a-fA-F]+)', src).group(1), 16)
    assert flag == _lib.SAD_L1_BLOCK_F16
    assert 'SILENTLY' in src  # the saturation's documentation


def test_runners_parse_precision_fp16():
    import catalog_runner
    import inference_runner
    a = inference_runner.build_parser().parse_args(['--merged-model', 'm.pth', '--audio', 'a.wav', '--precision', 'fp16'])
    assert a.precision == 'fp16'
    c = catalog_runner.build_parser()
    args = c.parse_args(['--merged-model', 'm.pth', '--audio-dir', 'd', '--precision', 'fp16', '--gpus', '2'])
    assert args.precision == 'fp16' and args.gpus == 2
    assert catalog_runner.DEFAULT_BATCH['fp16'] == catalog_runner.DEFAULT_BATCH['bf16']
    for parser in (inference_runner.build_parser(), c):
        act = next(x for x in parser._actions if x.dest == 'precision')
        assert list(act.choices) == ['fp32', 'bf16x3', 'bf16', 'fp16'] and act.default == 'fp32'
    with pytest.raises(SystemExit):
        inference_runner.build_parser().parse_args(['--merged-model', 'm', '--audio', 'a', '--precision', 'fp8'])


def test_trainer_precision_choices_unchanged():
    import submodel_trainer
    src = open(submodel_trainer.__file__).read()
    m = re.search(r"add_argument\('--precision', default='bf16', choices=\[([^\]]*)\]", src)
    assert m and [c.strip(" '") for c in m.group(1).split(',')] == ['bf16', 'mixed', 'fp32']


def test_engine_names_four_precisions_when_it_refuses_one():
    from sad.engine import _dtype_code
    with pytest.raises(ValueError) as e:
        _dtype_code('fp8')
    assert re.findall(r"'(\w+)'", str(e.value).split('(got')[0]) == ['bf16', 'bf16x3', 'fp16', 'fp32']
    assert _dtype_code('fp16') == 3


def test_engine_refuses_unknown_dtype_before_device_work(monkeypatch):
    """Engine(..., dtype='fp8') raises the same error (the plan builder checks the
    name first), with the four names in its message."""
    from sad import engine
    monkeypatch.setattr(engine, '_dev', lambda d: d)  # no device here
    from conftest import merged_sd
    with pytest.raises(ValueError, match=r"\['bf16', 'bf16x3', 'fp16', 'fp32'\]"):
        engine.Engine(merged_sd('n6'), 'cuda:0', dtype='fp8')
