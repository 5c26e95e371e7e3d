"""GPU: catalog_runner.py --gpus 2 as 2 ranks on ONE GPU (gloo, --one-device;
started without a launcher, so it spawns the ranks itself through
sad/launch.py): the list is split by file, each rank scans its range, rank 0
gathers -- and writes exactly the one-rank JSON."""
import json
import os
import subprocess
import sys

import pytest

import scan_catalogue as cat
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu


def _run(args, timeout=240):
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(PKG, 'catalog_runner.py')] + args, env=env, capture_output=True,
                       text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_two_ranks_write_the_one_rank_json(tmp_path):
    folder = tmp_path / 'wavs'
    folder.mkdir()
    paths = cat.write_catalogue(folder)
    model = cat.write_model(tmp_path / 'merged_n6.pth')
    common = ['--merged-model', model, '--audio-dir', str(folder), '--batch-size', '4', '--pack-seconds',
              str(cat.PACK_SECONDS), '--smooth']
    one, two = str(tmp_path / 'one.json'), str(tmp_path / 'two.json')
    _run(common + ['--output-json', two, '--gpus', '2', '--backend', 'gloo', '--one-device'])
    import catalog_runner as cr
    cr.main(common + ['--output-json', one])
    a, b = json.load(open(one)), json.load(open(two))
    assert [r['filename'] for r in b] == paths
    assert a == b
    assert open(one).read() == open(two).read()
