"""A/B helper (GPU box): the front end's dB + standardised maps, the stem and
the merged logits of one library build (SAD_LIB) on a fixed synthetic batch,
saved to an .npz as SHA-256 digests plus the first 2 segments (the files stay
small) -- two builds' files are then compared bit for bit.  Also digested: an
fp32 engine's merged logits on 32 segments, a resnet34 ResNetBackbone's pooled
features in the three dtypes on 8 segments, and Backbone.shared's per-tail
features for two tails on 8 segments.  The digests are printed, one per line.
    SAD_LIB=tools/_libsad_base.so python tools/lib_bits.py out_base.npz"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'synthetic-audio-detection_amd'), os.path.join(ROOT, 'tests')]

import hashlib  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    from conftest import merged_sd
    from sad import _lib
    from sad.engine import Engine
    dev = torch.device('cuda:0')
    B = 512
    pcm = torch.empty(B, 128000, dtype=torch.int16, device=dev)
    _lib.call('sad_synth_pcm', 7, 0, B, 128000, _lib.ptr(pcm), _lib.stream_handle(dev))
    out = {}
    for dt in ('bf16', 'bf16x3'):
        eng = Engine(merged_sd('n6'), dev, dtype=dt, micro_batch=256)
        maps = eng.frontend(pcm).clone()
        logits, merged = eng.forward_pcm(pcm)
        out[f'{dt}_maps'] = maps.cpu().numpy()
        out[f'{dt}_stem'] = eng.backbones[0].stem(maps[:64]).float().cpu().numpy()
        out[f'{dt}_merged'] = merged.cpu().numpy()
    from sad import weights as sw
    from sad.engine import Backbone, ResNetBackbone, split_merged_state
    eng = Engine(merged_sd('n6'), dev, dtype='fp32', micro_batch=16)
    out['fp32_merged'] = eng.forward_pcm(pcm[:32])[1].cpu().numpy()
    maps8 = maps[:8].contiguous()
    gold = os.path.join(ROOT, 'tests', 'golden')
    r34 = split_merged_state(sw.merged_state_dict(
        0, 1, bn_stats=sw.load_bn_stats(os.path.join(gold, 'bn_stats_resnet34.npz')), model_name='resnet34'))[1][0]
    bases = split_merged_state(merged_sd('n2'))[1]  # two distinct backbones: the second as a tail of the first
    for dt in ('fp32', 'bf16', 'bf16x3'):
        out[f'{dt}_resnet34_feats'] = ResNetBackbone(r34, 'resnet34', dev, dt, micro_batch=4)(maps8).cpu().numpy()
        bbs = [Backbone(b, dev, dt, micro_batch=4) for b in (bases[0], bases[1])]
        for t, f in enumerate(bbs[0].shared(bbs, maps8)):
            out[f'{dt}_shared_tail{t}'] = f.cpu().numpy()
    small = {}
    for k, v in out.items():
        small[k + '_sha256'] = np.frombuffer(hashlib.sha256(np.ascontiguousarray(v).tobytes()).digest(), np.uint8)
        if not k.endswith('_stem'):
            small[k + '_head'] = v[:2]
    for k in sorted(small):
        if k.endswith('_sha256'):
            print(k[:-7], small[k].tobytes().hex())
    np.savez(sys.argv[1], **small)


if __name__ == '__main__':
    main()
