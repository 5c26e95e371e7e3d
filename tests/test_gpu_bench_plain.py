"""GPU: a plain bench.py run (no --full) prints the headline line only, and
--dump-outputs writes what its last timed step computed.  The PCM and the
weights are seeded, so the dumped arrays must equal, bit for bit, a sequential
forward of the same segments through an engine built here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, merged_sd

pytestmark = pytest.mark.gpu


def test_plain_run_is_lean_and_dumps_last_step(tmp_path):
    import bench
    from sad import _lib
    from sad.engine import Engine
    B, steps, warmup = 64, 3, 1
    d = tmp_path / 'dump'
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--batch', str(B), '--dump-outputs', str(d)],
                       env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [json.loads(s) for s in r.stdout.splitlines() if s.startswith('{')]
    assert len(lines) == 1, r.stdout
    rec = lines[0]
    assert rec['unit'] == 'segments/s' and rec['higher_is_better'] is True and rec['dtype'] == 'bf16'
    assert rec['steps'] == steps and rec['warmup'] == warmup and rec['n_gpus'] == 1
    assert rec['ms_per_step'] > 0
    # value and ms_per_step are the same measurement (both rounded in the line)
    assert rec['value'] == pytest.approx(B * 1e3 / rec['ms_per_step'], rel=1e-2)
    for leg in ('roofline', 'accuracy', 'timed_output_check', 'parity_mode', 'fp32_mode', 'ingest', 'cpu_baseline'):
        assert leg not in rec, leg

    shapes = {'features': (B, 512), 'logits': (B, bench.HEADS, 2), 'merged': (B, bench.HEADS + 1)}
    assert sorted(os.listdir(d)) == sorted(k + '.npy' for k in shapes)
    got = {k: np.load(d / (k + '.npy')) for k in shapes}
    for k, a in got.items():
        assert a.dtype == np.float32 and a.shape == shapes[k] and np.isfinite(a).all(), k

    dev = torch.device('cuda:0')
    eng = Engine(merged_sd('n6'), dev, dtype='bf16', micro_batch=2048)
    pcm = torch.empty(B, bench.SEG, dtype=torch.int16, device=dev)
    _lib.call('sad_synth_pcm', 0, 0, B, bench.SEG, _lib.ptr(pcm), _lib.stream_handle(dev))
    logits, merged = eng.forward_pcm(pcm)
    torch.cuda.synchronize()
    assert np.array_equal(got['logits'], logits.cpu().numpy())
    assert np.array_equal(got['merged'], merged.cpu().numpy())
