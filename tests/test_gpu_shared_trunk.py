"""GPU: shared-trunk ensembles.  The ResNet-18 plan split after layer3
(sad_backbone_trunk_run / _tail_run / _shared_run) must equal the unsplit run
bit for bit -- the entries issue the same launches on the same micro-batch --
and an ensemble whose sub-models differ in layer4 alone must run one trunk,
give the features of the per-backbone loop exactly, and stay within the
north-star bar (|dlogit| <= 1e-3, identical decisions) of the CPU oracle.

Weights: the hash PRNG's 'n6d' model (seed 2, tests/golden/bn_stats_n6d.npz),
first sub-models, with sub-model 0's trunk copied into the others."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = ['fp32', 'bf16', 'bf16x3']


def n6d_sd(n=3):
    from sad import weights as sw
    sd = sw.merged_state_dict(2, 6, True, bn_stats=sw.load_bn_stats(os.path.join(GOLDEN, 'bn_stats_n6d.npz')))
    return {k: v for k, v in sd.items() if int(k.split('.')[1]) < n}


def share_trunk(sd, subs, src=0):
    """Copy sub-model src's non-layer4 backbone tensors into sub-models `subs`."""
    out = dict(sd)
    pre = f'sub_models.{src}.base.'
    for k, v in sd.items():
        if k.startswith(pre) and not k[len(pre):].startswith('layer4.'):
            for i in subs:
                out[f'sub_models.{i}.base.{k[len(pre):]}'] = v.clone()
    return out


def shared_sd(n=3):
    return share_trunk(n6d_sd(n), range(1, n))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.fixture(scope='module')
def maps3(golden_frontend):
    return torch.from_numpy(golden_frontend['std_map'][:3]).to(DEV).contiguous()


@pytest.fixture(scope='module')
def seg7():
    """7 synthesised segments: (device pcm, device maps, oracle images)."""
    from oracle import frontend as ofe
    from sad import _lib
    from sad.engine import FrontEnd
    pcm = torch.empty(7, 128000, dtype=torch.int16, device=DEV)
    _lib.call('sad_synth_pcm', 5, 0, 7, 128000, _lib.ptr(pcm), _lib.stream_handle(torch.device(DEV)))
    maps = FrontEnd(DEV)(pcm)
    host = pcm.cpu()
    with torch.no_grad():
        imgs = torch.cat([ofe.waveform_to_spectrogram(host[i].to(torch.float32) / 32768.0, 32000,
                                                      ofe.SpectrogramConfig()) for i in range(7)])
    return pcm, maps, imgs


@pytest.fixture(scope='module')
def oracle7(seg7):
    """Oracle merged and per-head logits of the 3-tail shared-trunk model on seg7."""
    from oracle import resnet as ores
    model = ores.load_merged_state(shared_sd(3))
    with torch.no_grad():
        return model(seg7[2]), ores.per_head_logits(model, seg7[2])


# -------------------------------------------------------------- primitives ----
@pytest.mark.parametrize('kind', ['maps', 'img'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_trunk_then_tail_equals_backbone_run(maps3, dtype, kind):
    """B = 3, micro-batch 2 (a ragged second chunk): trunk_run + tail_run ==
    sad_backbone_run / _run_img bit for bit; the tail leaves l3 intact."""
    from sad.engine import Backbone, resize, split_merged_state
    _, bases, _ = split_merged_state(n6d_sd(1))
    bb = Backbone(bases[0], DEV, dtype, micro_batch=2)
    x = maps3 if kind == 'maps' else resize(maps3).contiguous()
    ref = bb(x) if kind == 'maps' else bb.forward_images(x)
    l3 = bb.trunk(x, kind)
    assert l3.shape == (3, 32, 32, 512 if dtype == 'bf16x3' else 256)
    assert l3.dtype == (torch.float32 if dtype == 'fp32' else torch.bfloat16)
    before = _bits(l3).clone()
    feats = bb.tail(l3)
    torch.cuda.synchronize()
    assert torch.equal(_bits(l3), before)
    assert torch.equal(_bits(feats), _bits(ref)), (feats - ref).abs().max().item()
    assert torch.isfinite(feats).all() and feats.abs().max() > 0
    again = bb.tail(l3)  # and a second tail on the same activation
    assert torch.equal(_bits(again), _bits(ref))


def test_l3_is_layer3_output_in_the_documented_layout(maps3):
    """fp32 l3 against the oracle's layer3 output (NHWC).  Bound: 15 fp32 convs
    with K <= 2304 and fp32 accumulation, each ~sqrt(K) * 2^-24 ~ 3e-6 of the
    activation scale -> 1e-4 of max|ref| (the bar test_gpu_parity.py puts on
    the fp32 features).  The split layout decodes (from_split) to the same
    activation; its dropped lo*lo products are 2^-16 per product -> 1e-3."""
    from oracle import frontend as ofe
    from oracle import resnet as ores
    from sad.engine import Backbone, from_split, split_merged_state
    sd = n6d_sd(1)
    _, bases, _ = split_merged_state(sd)
    base = ores.load_merged_state(sd).sub_models[0].base
    with torch.no_grad():
        x = ofe.resize_bilinear(maps3.cpu().unsqueeze(1), (512, 512)).repeat(1, 3, 1, 1)
        x = base.maxpool(base.act1(base.bn1(base.conv1(x))))
        ref = base.layer3(base.layer2(base.layer1(x))).permute(0, 2, 3, 1)
    l3 = Backbone(bases[0], DEV, 'fp32', micro_batch=2).trunk(maps3).cpu()
    e32 = ((l3 - ref).abs().max() / ref.abs().max()).item()
    x3 = from_split(Backbone(bases[0], DEV, 'bf16x3', micro_batch=2).trunk(maps3)).cpu()
    e3 = ((x3 - ref).abs().max() / ref.abs().max()).item()
    print(f'l3 vs oracle layer3, rel. to max: fp32 {e32:.3e}  bf16x3 {e3:.3e}')
    assert e32 <= 1e-4 and e3 <= 1e-3


def test_shared_run_refuses_a_tail_of_another_dtype(maps3):
    from sad import _lib
    from sad.engine import Backbone, split_merged_state
    _, bases, _ = split_merged_state(n6d_sd(1))
    trunk = Backbone(bases[0], DEV, 'bf16', micro_batch=2)
    other = Backbone(bases[0], DEV, 'fp32', micro_batch=2)
    with pytest.raises(RuntimeError, match='dtype'):
        trunk.shared([trunk, other], maps3)
    lib = _lib.load()
    feats = torch.zeros(2, 3, 512, device=DEV)
    ws = trunk.workspace(2)
    plans = (_lib.ctypes.c_void_p * 2)(trunk._plan.value, other._plan.value)
    fp = (_lib.ctypes.c_void_p * 2)(feats[0].data_ptr(), feats[1].data_ptr())
    rc = lib.sad_backbone_shared_run(trunk._plan, plans, 2, _lib.ptr(maps3), None, 3, 2, fp, _lib.ptr(ws),
                                     ws.numel(), _lib.stream_handle(torch.device(DEV)))
    assert rc == -1  # SAD_ERR_ARG, before any launch
    torch.cuda.synchronize()
    assert not feats.any()
    # both inputs, or neither, is an argument error too
    rc = lib.sad_backbone_trunk_run(trunk._plan, _lib.ptr(maps3), _lib.ptr(maps3), 3, 2, _lib.ptr(feats),
                                    _lib.ptr(ws), ws.numel(), None)
    assert rc == -1


# ------------------------------------------------------------------ engine ----
@pytest.mark.parametrize('dtype', DTYPES)
def test_engine_shares_one_trunk_bit_for_bit(seg7, oracle7, dtype):
    """One trunk under three tails, B = 7 with micro-batch 3 (3 + 3 + 1)."""
    from oracle.decision import interpret_multihead_logits
    from sad.engine import Engine
    _, maps, _ = seg7
    eng = Engine(shared_sd(3), DEV, dtype=dtype, micro_batch=3)
    g = eng.grouping
    assert len(eng.backbones) == 3 and g.n_trunks == 1 and g.n_backbones == 3
    assert eng.shared_groups == [[0, 1, 2]] and g.feat_index == [0, 1, 2]
    assert g.describe() == '3 sub-models: 1 trunk, 3 tails'
    shared = eng.features(maps)
    alone = [bb(maps) for bb in eng.backbones]
    torch.cuda.synchronize()
    for j in range(3):
        assert torch.equal(_bits(shared[j]), _bits(alone[j])), (j, (shared[j] - alone[j]).abs().max().item())
    assert not torch.equal(shared[0], shared[1]) and not torch.equal(shared[1], shared[2])
    logits, merged = eng.forward_maps(maps)
    l2, m2 = eng.heads(alone)
    assert torch.equal(logits, l2) and torch.equal(merged, m2)
    if dtype == 'bf16':
        return
    ref_m, ref_h = oracle7
    dm = (merged.cpu() - ref_m).abs().max().item()
    dh = (logits.cpu() - ref_h).abs().max().item()
    print(f'shared trunk {dtype}: max|dlogit| merged {dm:.3e} per-head {dh:.3e}; max|z| {ref_m.abs().max():.2f}')
    assert dm <= 1e-3 and dh <= 1e-3
    names = ['S0', 'S1', 'S2']
    for row, ref in zip(merged.cpu(), ref_m):
        assert interpret_multihead_logits(row, 0.5, names)[0] == interpret_multihead_logits(ref, 0.5, names)[0]


def test_engine_features_from_images_equal_the_unshared_loop(maps3):
    """The img form (ModularMultiHeadClassifier.__call__ with identical channels)."""
    import inference_runner as ir
    from sad.engine import Engine, resize
    sd = shared_sd(3)
    eng = Engine(sd, DEV, dtype='bf16x3', micro_batch=2)
    img = resize(maps3).contiguous()
    shared = eng.features(img, kind='img')
    alone = [bb.forward_images(img) for bb in eng.backbones]
    for a, b in zip(shared, alone):
        assert torch.equal(_bits(a), _bits(b))
    with pytest.raises(ValueError, match='kind'):
        eng.features(img, kind='img3')
    subs = []
    for i in range(3):
        sm = ir.BinaryClassifier(init='empty')
        sm.load_state_dict({k[len(f'sub_models.{i}.'):]: v for k, v in sd.items()
                            if k.startswith(f'sub_models.{i}.')}, strict=True)
        subs.append(sm)
    model = ir.ModularMultiHeadClassifier(subs, DEV, 'bf16x3', micro_batch=2)
    out = model(img.unsqueeze(1).repeat(1, 3, 1, 1))
    assert torch.equal(out, model.engine.heads([bb.forward_images(img) for bb in model.engine.backbones])[1])


def test_mixed_ensemble_keeps_head_order_and_values(maps3):
    """Sub-models 0 and 1 on one trunk, 2 fully distinct, 3 a duplicate of 0."""
    from sad.engine import Engine
    sd = share_trunk(n6d_sd(3), [1])
    for k, v in list(sd.items()):
        if k.startswith('sub_models.0.base.'):
            sd['sub_models.3.' + k[len('sub_models.0.'):]] = v.clone()
        if k.startswith('sub_models.1.head.'):  # its own head: the duplicate is of the backbone
            sd['sub_models.3.' + k[len('sub_models.1.'):]] = v.clone()
    eng = Engine(sd, DEV, dtype='fp32', micro_batch=2)
    g = eng.grouping
    assert g.feat_index == [0, 1, 2, 0] and g.trunk_of == [0, 0, 1] and eng.shared_groups == [[0, 1]]
    assert len(eng.backbones) == 3 and g.describe() == '4 sub-models: 2 trunks, 3 tails'
    feats = eng.features(maps3)
    alone = [bb(maps3) for bb in eng.backbones]
    for a, b in zip(feats, alone):
        assert torch.equal(_bits(a), _bits(b))
    logits, merged = eng.forward_maps(maps3)
    l2, m2 = eng.heads(alone)
    assert torch.equal(logits, l2) and torch.equal(merged, m2)
    assert logits.shape == (3, 4, 2) and merged.shape == (3, 5)
    # head 3 sits on backbone 0's features with head 1's weights
    assert not torch.equal(logits[:, 3], logits[:, 1]) and not torch.equal(logits[:, 3], logits[:, 0])


# -------------------------------------------------------------------- scan ----
def test_catalogue_scan_equals_single_file_runs_on_a_shared_trunk_model(tmp_path, golden_frontend, capsys):
    import catalog_runner as cr
    import inference_runner as ir
    from sad.audio import save_pcm16
    pcm = golden_frontend['pcm']
    folder = tmp_path / 'wavs'
    folder.mkdir()
    paths = [str(folder / 'a_two_windows.wav'), str(folder / 'b_short.wav')]
    save_pcm16(paths[0], np.concatenate([pcm[0], pcm[1]]))
    save_pcm16(paths[1], pcm[2][:77777])
    model = str(tmp_path / 'shared.pth')
    torch.save({'state_dict': shared_sd(3), 'metadata': {'class_names': ['SynA', 'SynB', 'SynC', 'Real']}}, model)
    out = str(tmp_path / 'scan.json')
    recs = cr.main(['--merged-model', model, '--audio-dir', str(folder), '--output-json', out, '--batch-size', '2'])
    assert '3 sub-models: 1 trunk, 3 tails' in capsys.readouterr().out
    assert [r['filename'] for r in recs] == paths
    real_load, cache = ir.load_merged_model, {}

    def load_once(path, device, backbone_name='resnet18', precision='fp32'):
        if path not in cache:
            cache[path] = real_load(path, device, backbone_name=backbone_name, precision=precision)
        return cache[path]

    ir.load_merged_model = load_once
    try:
        for rec, p in zip(recs, paths):
            o = str(tmp_path / 'single.json')
            ir.main(['--merged-model', model, '--audio', p, '--output-json', o])
            ref = json.load(open(o))
            assert list(rec) == list(ref) == ['filename', 'segments', 'percentages']
            assert rec['segments'] == ref['segments'] and len(rec['segments']) >= 1
            assert list(rec['percentages']) == list(ref['percentages'])
            for k, v in ref['percentages'].items():
                assert abs(rec['percentages'][k] - v) <= 1e-3, (p, k, rec['percentages'][k], v)
    finally:
        ir.load_merged_model = real_load
