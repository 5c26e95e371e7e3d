"""GPU: the fp16 (SAD_F16) plans end to end.

* split-plan equality (B = 3, micro-batch 2): trunk + tail equals Backbone(...)
  bit for bit for maps and img; three tails on one trunk through Engine.features
  equal the per-backbone loop (tests/test_gpu_shared_trunk.py's shared_sd); a
  bf16 tail under an fp16 trunk is refused before any launch; B = 5 at
  micro-batch 2 equals micro-batch 5;
* launch census: one forward of B = 4 inside sad_profile_begin / end in bf16 and
  in fp16 launches the same number of kernels of every variant id -- "same
  kernels", which no value test can pin;
  the same for resnet50's Bottleneck plan
  (its three 64 -> 64 3x3 convs on variant 25, not on the implicit GEMM);
* accuracy gate on tests/test_gpu_accuracy_gate.py's workload against the fp32
  device path.  Bars from the bf16 gate's by the ratio of the unit roundoffs,
  2^-11 / 2^-8 = 1/8: max|dlogit| <= 0.15 / 8 = 0.01875, identical decisions
  >= 1 - 0.05 / 8 = 0.99375, and d_fp16 <= d_bf16 / 4 (expected ratio 8; the
  factor 2 is for the different mix of weight and activation error);
* the deep plans (resnet34, resnet50) against tests/golden/golden_deep.npz as
  tests/test_gpu_deep_golden.py runs them: finite, d_fp16 <= d_bf16 / 4, and the
  fixture's decisions wherever bf16 has them;
* the command lines: inference_runner --precision fp16 writes the fp32 run's
  JSON keys and segment labels; catalog_runner --precision fp16 on two files
  equals the single-file runs.

Measured values (MI355X) are in profiles/fp16_tests_ratios.txt.
"""
import json
import os

import numpy as np
import pytest
import torch

import scan_catalogue as cat
import test_gpu_accuracy_gate as AG
import test_gpu_deep_golden as DG
import test_gpu_shared_trunk as ST
from conftest import GOLDEN, merged_sd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.fixture(scope='module')
def maps5(golden_frontend):
    m = torch.from_numpy(golden_frontend['std_map'])
    return torch.cat([m[:4], m[1:2] * 0.5 + m[2:3] * 0.5]).to(DEV).contiguous()


# ------------------------------------------------------ split-plan equality --
@pytest.mark.parametrize('kind', ['maps', 'img'])
def test_trunk_then_tail_equals_backbone_run(maps5, kind):
    from sad.engine import Backbone, resize, split_merged_state
    _, bases, _ = split_merged_state(ST.n6d_sd(1))
    bb = Backbone(bases[0], DEV, 'fp16', micro_batch=2)
    x = maps5[:3].contiguous() if kind == 'maps' else resize(maps5[:3].contiguous()).contiguous()
    ref = bb(x) if kind == 'maps' else bb.forward_images(x)
    l3 = bb.trunk(x, kind)
    assert l3.shape == (3, 32, 32, 256) and l3.dtype == torch.float16
    before = _bits(l3).clone()
    feats = bb.tail(l3)
    torch.cuda.synchronize()
    assert torch.equal(_bits(l3), before)
    assert torch.equal(_bits(feats), _bits(ref)), (feats - ref).abs().max().item()
    assert torch.isfinite(feats).all() and feats.abs().max() > 0 and torch.isfinite(l3.float()).all()


def test_three_tails_on_one_trunk_equal_the_per_backbone_loop(maps5):
    from sad.engine import Engine
    eng = Engine(ST.shared_sd(3), DEV, dtype='fp16', micro_batch=2)
    assert eng.grouping.n_trunks == 1 and eng.grouping.n_backbones == 3 and eng.shared_groups == [[0, 1, 2]]
    x = maps5[:3].contiguous()
    shared = eng.features(x)
    loop = [bb(x) for bb in eng.backbones]
    torch.cuda.synchronize()
    for a, b in zip(shared, loop):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(shared[0], shared[1])


def test_bf16_tail_under_fp16_trunk_is_refused_before_any_launch(maps5):
    from sad import _lib
    from sad.engine import Backbone, split_merged_state
    _, bases, _ = split_merged_state(ST.n6d_sd(1))
    trunk = Backbone(bases[0], DEV, 'fp16', micro_batch=2)
    tail = Backbone(bases[0], DEV, 'bf16', micro_batch=2)
    x = maps5[:3].contiguous()
    with pytest.raises(RuntimeError, match='dtype'):
        trunk.shared([trunk, tail], x)
    # through the C entry with sentinels: neither the features nor the workspace
    # (every launch's output lies in it) is written
    sz = _lib.SZ()
    _lib.call('sad_backbone_shared_workspace_size', trunk._plan, 2, _lib.ctypes.byref(sz))
    ws = torch.full((sz.value,), 0xA5, dtype=torch.uint8, device=DEV)
    feats = torch.full((2, 3, 512), 7.0, device=DEV)
    plans = (_lib.ctypes.c_void_p * 2)(trunk._plan.value, tail._plan.value)
    fp = (_lib.ctypes.c_void_p * 2)(feats[0].data_ptr(), feats[1].data_ptr())
    rc = _lib.load().sad_backbone_shared_run(trunk._plan, plans, 2, _lib.ptr(x), None, 3, 2, fp, _lib.ptr(ws),
                                             ws.numel(), _lib.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == -1 and b'dtype' in _lib.load().sad_last_error()
    assert bool((feats == 7.0).all()) and bool((ws == 0xA5).all())
    with pytest.raises(AssertionError):
        tail.tail(trunk.trunk(x))              # the wrapper checks the activation's dtype


def test_micro_batch_does_not_change_the_features(maps5):
    from sad.engine import Backbone, split_merged_state
    _, bases, _ = split_merged_state(ST.n6d_sd(1))
    a = Backbone(bases[0], DEV, 'fp16', micro_batch=2)(maps5)
    b = Backbone(bases[0], DEV, 'fp16', micro_batch=5)(maps5)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------ launch census --
# every variant id a bf16 / fp16 plan can reach: the implicit GEMMs 9-19, the halo kernels 20-22 and 25,
# the patch-resident 30-32, the fused layer1 block 40, the resident-weight convs 41 / 43, and 44
VARIANT_IDS = list(range(9, 20)) + [20, 21, 22, 25, 30, 31, 32, 40, 41, 43, 44]


def _census(bb, maps):
    """{variant id: kernel launches} of one forward of backbone `bb` (a bracket answers for one id)"""
    from sad import _lib
    bb(maps)
    torch.cuda.synchronize()
    counts, total = {}, 0
    for v in [0] + VARIANT_IDS:
        _lib.call('sad_profile_begin')
        bb(maps)
        ms, n, fl = _lib.ctypes.c_double(), _lib.I64(), _lib.ctypes.c_double()
        _lib.call('sad_profile_end', v, _lib.ctypes.byref(ms), _lib.ctypes.byref(n), _lib.ctypes.byref(fl))
        if v == 0:
            total = n.value
        elif n.value:
            counts[v] = n.value
    assert sum(counts.values()) == total, (counts, total)     # no launch under an id outside the list
    return counts


def test_launch_census_equals_bf16s(maps5):
    from sad.engine import Backbone, split_merged_state
    _, bases, _ = split_merged_state(ST.n6d_sd(1))
    maps = maps5[:4].contiguous()
    cb, ch = (_census(Backbone(bases[0], DEV, dt, micro_batch=4), maps) for dt in ('bf16', 'fp16'))
    print(f'launches per variant: bf16 {cb}, fp16 {ch}')
    assert ch == cb
    assert cb == {40: 2, 43: 1, 41: 3, 44: 2, 31: 6}      # the bf16 plan's kernels (layer1 .. layer4)


def test_bottleneck_plan_launch_census_equals_bf16s(maps5):
    """The deep Bottleneck plans (resnet50: 3 + 4 + 6 + 3 blocks): fp16 runs every conv on
    the variant bf16 runs it on -- layer1's three 64 -> 64 3x3 convs at 128 x 128 on the
    resident-weight halo kernel (variant 25), not on the implicit GEMM."""
    from sad.engine import Engine
    maps = maps5[:2].contiguous()
    cb, ch = (_census(Engine(DG._sd('resnet50'), DEV, dtype=dt, micro_batch=2).backbones[0], maps)
              for dt in ('bf16', 'fp16'))
    print(f'resnet50 launches per variant: bf16 {cb}, fp16 {ch}')
    assert ch == cb
    assert cb[25] == 3 and sum(cb.values()) == 48      # 16 blocks x 3 convs (a downsample rides in its conv3)


# ------------------------------------------------------------ accuracy gate --
@pytest.fixture(scope='module')
def batch():
    """tests/test_gpu_accuracy_gate.py's workload (B = 2,048 synthesised segments,
    seed 0, the n6 model) and its fp32 device reference, once per module."""
    from sad import _lib
    from sad.engine import Engine
    sd = merged_sd('n6')
    pcm = torch.empty(AG.B, 128000, dtype=torch.int16, device=DEV)
    _lib.call('sad_synth_pcm', 0, 0, AG.B, 128000, _lib.ptr(pcm), _lib.stream_handle(torch.device(DEV)))
    _, m32 = Engine(sd, DEV, dtype='fp32', micro_batch=128).forward_pcm(pcm)
    torch.cuda.synchronize()
    return sd, pcm, m32.cpu()


def test_accuracy_gate(batch):
    from sad.engine import Engine
    sd, pcm, m32 = batch
    l32 = AG._decisions(m32)
    got = {}
    for dtype in ('fp16', 'bf16'):
        _, m = Engine(sd, DEV, dtype=dtype, micro_batch=2048).forward_pcm(pcm)
        torch.cuda.synchronize()
        m = m.cpu()
        assert torch.isfinite(m).all()
        agree = sum(a == b for a, b in zip(AG._decisions(m), l32)) / AG.B
        got[dtype] = ((m - m32).abs().max().item(), agree)
    (d16, a16), (db, ab) = got['fp16'], got['bf16']
    line = (f'accuracy gate (B 2048, n6, micro-batch 2048, vs fp32 device): fp16 max|dlogit| {d16:.3e}, decisions '
            f'identical {a16:.5f} ({round((1 - a16) * AG.B)} flips); bf16 {db:.3e}, {ab:.5f} '
            f'({round((1 - ab) * AG.B)} flips); ratio {db / d16:.2f}')
    print(line)
    assert d16 <= 0.15 / 8, d16
    assert a16 >= 1 - 0.05 / 8, a16
    assert d16 <= db / 4, (d16, db)


# --------------------------------------------------------------- deep plans --
@pytest.mark.parametrize('name', ['resnet34', 'resnet50'])
def test_deep_plans(golden_frontend, name):
    from oracle.decision import interpret_multihead_logits
    from sad.engine import Engine
    fx = dict(np.load(os.path.join(GOLDEN, 'golden_deep.npz')))
    pcm = torch.from_numpy(golden_frontend['pcm']).to(DEV)
    ref = torch.from_numpy(fx[f'{name}_merged'])
    dec = lambda rows: [interpret_multihead_logits(r, 0.5, ['A', 'B'])[0] for r in rows]
    out = {}
    for dtype in ('fp16', 'bf16'):
        logits, merged = Engine(DG._sd(name), DEV, dtype=dtype, micro_batch=3).forward_pcm(pcm)
        torch.cuda.synchronize()
        assert torch.isfinite(merged).all() and torch.isfinite(logits).all()
        d = max(np.abs(merged.cpu().numpy() - fx[f'{name}_merged']).max(),
                np.abs(logits.cpu().numpy() - fx[f'{name}_per_head']).max())
        out[dtype] = (float(d), dec(merged.cpu()))
    (d16, dec16), (db, decb) = out['fp16'], out['bf16']
    line = f'deep {name} vs golden_deep: fp16 max|dlogit| {d16:.3e}, bf16 {db:.3e}, ratio {db / d16:.2f}'
    print(line)
    assert d16 <= db / 4, (d16, db)
    for a, b, r in zip(dec16, decb, dec(ref)):
        if b == r:
            assert a == r


# ------------------------------------------------------------ command lines --
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp('fp16cli')
    folder = root / 'wavs'
    folder.mkdir()
    from sad.audio import save_pcm16
    pcm = np.load(os.path.join(GOLDEN, 'golden_frontend.npz'))['pcm']
    four = str(root / 'four.wav')
    save_pcm16(four, np.concatenate([pcm[0], pcm[1], pcm[2], pcm[3]]))
    a, b = str(folder / 'a.wav'), str(folder / 'b.wav')
    save_pcm16(a, np.concatenate([pcm[0], pcm[1], pcm[2]]))
    save_pcm16(b, np.concatenate([pcm[3], pcm[0][:77777]]))
    return {'model': cat.write_model(root / 'merged_n6.pth'), 'four': four, 'folder': str(folder), 'ab': [a, b],
            'root': root}


def test_inference_runner_precision_fp16(files):
    import inference_runner as ir
    out = {}
    for prec in ('fp32', 'fp16'):
        o = str(files['root'] / f'{prec}.json')
        js = ir.main(['--merged-model', files['model'], '--audio', files['four'], '--output-json', o, '--precision',
                      prec])
        assert json.load(open(o)) == js
        out[prec] = js
    assert list(out['fp16']) == list(out['fp32']) and len(out['fp32']['segments']) == 4
    assert list(out['fp16']['percentages']) == list(out['fp32']['percentages'])
    assert out['fp16']['segments'] == out['fp32']['segments']       # start, end and label of every window
    model, _ = ir.load_merged_model(files['model'], torch.device(DEV), precision='fp16')
    assert model.precision == 'fp16' and model.engine.dtype == 'fp16'


def test_catalog_runner_precision_fp16_equals_single_file_runs(files):
    import catalog_runner as cr
    import inference_runner as ir
    o = str(files['root'] / 'scan.json')
    recs = cr.main(['--merged-model', files['model'], '--audio-dir', files['folder'], '--output-json', o,
                    '--precision', 'fp16', '--batch-size', '4'])
    assert [r['filename'] for r in recs] == files['ab']
    for rec, p in zip(recs, files['ab']):
        single = ir.main(['--merged-model', files['model'], '--audio', p, '--output-json',
                          str(files['root'] / 'single.json'), '--precision', 'fp16'])
        assert rec['segments'] == single['segments'] and len(rec['segments']) >= 1
        assert list(rec['percentages']) == list(single['percentages'])
