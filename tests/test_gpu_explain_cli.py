"""GPU: inference_runner.py --evidence on a synthesised 10 s WAV (two 4 s
windows at the CLI's hop of one window), fp32, two sub-models on one backbone.

  * the JSON written with and without --evidence is byte-identical;
  * the .npz holds evidence [2, 2, 16, 16] float32, timestamps, names, target,
    col_sec [16], row_hz [16, 2] and timeline [2, 32];
  * timeline equals the host reference (tests/evidence_ref.py) applied to the
    file's evidence;
  * orientation pin.  The WAV is 4 s of low noise played twice; the second
    window adds a 6 kHz tone burst in its last second.  Sub-model 0's head is
    rebuilt so that its gradient is uniform over the channels whatever the
    input (one always-active unit per layer), which makes its map a positive
    multiple of layer4's channel sum -- positive everywhere, so the raw
    centroid says little.  The burst's evidence is the second window's map
    minus the first's (same background); the centroid of its positive part
    must lie in the last column quarter (columns 12..15, the window's last
    second) and in a row whose row_hz band contains 6 kHz.  A transposed or
    flipped axis puts it in another quarter or in a band below 1 kHz.
"""
import os

import numpy as np
import pytest
import torch

import evidence_ref as E
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SR = 32000
TONE_HZ = 6000.0


def _uniform_gradient_head(sd, i):
    """Head i: y1[0] = sum_c f_c / 512 + 1 > 0 (f >= 0 after ReLU and pooling),
    y2[0] = y1[0] + 1 > 0, Synthetic logit = y2[0]; every other weight of the
    path is zero and the BatchNorms are the identity up to eps.  So g is one
    positive constant on every channel for every input."""
    p = f'sub_models.{i}.head.'
    for k in ('2.weight', '2.bias', '6.weight', '6.bias', '10.weight', '10.bias'):
        sd[p + k] = torch.zeros_like(sd[p + k])
    sd[p + '2.weight'][0] = 1.0 / 512
    sd[p + '2.bias'][0] = 1.0
    sd[p + '6.weight'][0, 0] = 1.0
    sd[p + '6.bias'][0] = 1.0
    sd[p + '10.weight'][1, 0] = 1.0
    for idx in ('3', '7'):
        sd[p + idx + '.weight'] = torch.ones_like(sd[p + idx + '.weight'])
        sd[p + idx + '.bias'] = torch.zeros_like(sd[p + idx + '.bias'])
        sd[p + idx + '.running_mean'] = torch.zeros_like(sd[p + idx + '.running_mean'])
        sd[p + idx + '.running_var'] = torch.ones_like(sd[p + idx + '.running_var'])


@pytest.fixture(scope='module')
def run(tmp_path_factory):
    import inference_runner as ir
    from sad import weights as sw
    from sad.audio import save_pcm16
    tmp = tmp_path_factory.mktemp('explain_cli')
    sd = sw.merged_state_dict(0, 2, False, bn_stats=sw.load_bn_stats(os.path.join(GOLDEN, 'bn_stats_n6.npz')))
    _uniform_gradient_head(sd, 0)
    merged = str(tmp / 'merged.pth')
    torch.save({'state_dict': dict(sd), 'metadata': {'class_names': ['SynA', 'SynB', 'Real']}}, merged)
    rng = np.random.default_rng(3)
    noise = 0.01 * rng.standard_normal(4 * SR)
    x = np.concatenate([noise, noise, noise[:2 * SR]])
    t = np.arange(SR) / SR
    x[7 * SR:8 * SR] += 0.5 * np.sin(2 * np.pi * TONE_HZ * t)
    wav = str(tmp / 'clip.wav')
    save_pcm16(wav, np.round(x * 32767).astype(np.int16))
    plain, with_ev, npz = str(tmp / 'plain.json'), str(tmp / 'ev.json'), str(tmp / 'ev.npz')
    ir.main(['--merged-model', merged, '--audio', wav, '--output-json', plain])
    ir.main(['--merged-model', merged, '--audio', wav, '--output-json', with_ev, '--evidence', npz])
    return plain, with_ev, npz


def test_json_is_unchanged_and_npz_is_complete(run):
    plain, with_ev, npz = run
    with open(plain, 'rb') as a, open(with_ev, 'rb') as b:
        assert a.read() == b.read()
    z = np.load(npz)
    assert sorted(z.files) == ['col_sec', 'evidence', 'names', 'row_hz', 'target', 'timeline', 'timestamps']
    assert z['evidence'].shape == (2, 2, 16, 16) and z['evidence'].dtype == np.float32
    assert np.isfinite(z['evidence']).all()
    assert z['timestamps'].tolist() == [0.0, 4.0]
    assert z['names'].tolist() == ['SynA', 'SynB'] and str(z['target']) == 'synthetic'
    assert np.array_equal(z['col_sec'], np.arange(16) * 0.25)
    assert z['row_hz'].shape == (16, 2) and (np.diff(z['row_hz'][:, 0]) > 0).all()
    assert z['timeline'].shape == (2, 32) and z['timeline'].dtype == np.float64
    ref = E.timeline(z['evidence'], z['timestamps'], 4.0)
    assert np.array_equal(z['timeline'], ref)
    # hop = one window: bin 16 w + x is window w's column x
    assert np.allclose(z['timeline'][:, 16:], z['evidence'][1].astype(np.float64).sum(axis=1), rtol=1e-12)


def test_orientation_pin(run):
    z = np.load(run[2])
    ev = z['evidence'].astype(np.float64)
    assert (ev[:, 0] > 0).all()                       # the uniform-gradient head: a positive channel sum
    burst = np.maximum(ev[1, 0] - ev[0, 0], 0.0)      # [rows, cols]
    w = burst / burst.sum()
    row = float((w.sum(axis=1) * np.arange(16)).sum())
    col = float((w.sum(axis=0) * np.arange(16)).sum())
    band = z['row_hz'][int(round(row))]
    print(f'orientation: burst centroid row {row:.2f} col {col:.2f}; row band {band.tolist()} Hz')
    assert 12.0 <= col < 16.0, col
    assert band[0] <= TONE_HZ <= band[1], (row, band)
    assert z['col_sec'][int(col)] >= 3.0
