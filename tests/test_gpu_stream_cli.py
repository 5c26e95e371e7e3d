"""GPU: stream_runner.py against inference_runner.py on the catalogue's 44.1 kHz
stereo file, each run a fresh child process.

  * --wav in 37 ms chunks writes a JSON file byte-equal to inference_runner.py's
    file for the same path;
  * --raw with the same samples piped to stdin in 1,001-byte writes (an odd
    size, so frames are split between writes) gives the same segments and
    percentages;
  * the event lines on stdout parse and match the record's segments in order.
"""
import json
import os
import subprocess
import sys
import tempfile
import threading

import pytest

import scan_catalogue as cat
from conftest import PKG

pytestmark = pytest.mark.gpu


def _child(script, args, stdin_bytes=None, piece=1001):
    cmd = [sys.executable, os.path.join(PKG, script)] + args
    if stdin_bytes is None:
        r = subprocess.run(cmd, capture_output=True, timeout=300)
        out, err, rc = r.stdout, r.stderr, r.returncode
    else:
        errf = tempfile.TemporaryFile()  # a file, so a full pipe can never block the child
        p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=errf, bufsize=0)

        def feed():
            for i in range(0, len(stdin_bytes), piece):
                p.stdin.write(stdin_bytes[i:i + piece])
            p.stdin.close()

        t = threading.Thread(target=feed)
        t.start()
        out = p.stdout.read()
        t.join()
        rc = p.wait(timeout=300)
        errf.seek(0)
        err = errf.read()
    assert rc == 0, err.decode(errors='replace')[-2000:]
    return out.decode()


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    from sad import audio
    root = tmp_path_factory.mktemp('stream_cli')
    folder = root / 'wavs'
    folder.mkdir()
    wav = [p for p in cat.write_catalogue(folder) if p.endswith('b_44k_stereo.wav')][0]
    model = cat.write_model(root / 'merged_n6.pth')
    samples, ch, sr = audio.read_wav(wav)
    assert (ch, sr, str(samples.dtype)) == (2, 44100, 'int16')
    files = {k: str(root / f'{k}.json') for k in ('file', 'wav', 'raw')}
    _child('inference_runner.py', ['--merged-model', model, '--audio', wav, '--output-json', files['file']])
    out_wav = _child('stream_runner.py', ['--merged-model', model, '--wav', wav, '--chunk-ms', '37',
                                          '--output-json', files['wav']])
    out_raw = _child('stream_runner.py', ['--merged-model', model, '--raw', '-', '--rate', '44100', '--channels', '2',
                                          '--format', 's16le', '--output-json', files['raw']],
                     stdin_bytes=samples.tobytes())
    return files, out_wav, out_raw


def test_wav_stream_writes_the_file_runners_bytes(runs):
    files, _, _ = runs
    with open(files['file'], 'rb') as a, open(files['wav'], 'rb') as b:
        ref, got = a.read(), b.read()
    assert got == ref and len(json.loads(ref)['segments']) == 1


def test_raw_stdin_in_odd_writes_gives_the_same_record(runs):
    files, _, _ = runs
    ref, raw = json.load(open(files['file'])), json.load(open(files['raw']))
    assert raw['segments'] == ref['segments'] and raw['percentages'] == ref['percentages']
    assert raw['filename'] == '-' and list(raw) == list(ref)


def test_event_lines_match_the_record(runs):
    files, out_wav, out_raw = runs
    checked = 0
    for key, out in (('wav', out_wav), ('raw', out_raw)):
        rec = json.load(open(files[key]))
        events = [json.loads(line) for line in out.splitlines()]  # every stdout line is an event
        assert [(e['start_sec'], e['end_sec'], e['label']) for e in events] == \
            [(s['start_sec'], s['end_sec'], s['label']) for s in rec['segments']]
        for e in events:
            assert e['name'] == rec['filename'] and len(e['probs']) == len(e['logits']) == 7 and e['slot'] == 0
        checked += len(events)
    assert checked == 2
