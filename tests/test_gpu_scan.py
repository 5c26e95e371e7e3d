"""GPU: catalog_runner.py end to end on a small folder, fp32, n6 fixture model.

For every readable file the scan's record equals the one inference_runner.main
writes for that file alone (segments identical, percentages within 1e-3), plain
and --smooth, although --batch-size 4 and 30 s packs make batches and packs
straddle files; the garbage file yields an error record, the silent file main's
empty record, and the records come in sorted order.  The merged logits of the
packed run are bit-identical to the single-file path's.
"""
import json

import pytest
import torch

import scan_catalogue as cat

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    root = tmp_path_factory.mktemp('scan')
    folder = root / 'wavs'
    folder.mkdir()
    return {'model': cat.write_model(root / 'merged_n6.pth'), 'paths': cat.write_catalogue(folder),
            'folder': str(folder), 'root': root}


@pytest.fixture(scope='module')
def oracle(setup):
    """inference_runner.main per file, plain and smooth.  The checkpoint is
    loaded once for all of these calls (main is otherwise untouched); the
    scanner under test loads its own."""
    import inference_runner as ir
    real_load, cache = ir.load_merged_model, {}

    def load_once(path, device, backbone_name='resnet18', precision='fp32'):
        key = (path, str(device), backbone_name, precision)
        if key not in cache:
            cache[key] = real_load(path, device, backbone_name=backbone_name, precision=precision)
        return cache[key]

    out = {}
    ir.load_merged_model = load_once
    try:
        for smooth in (False, True):
            for p in setup['paths'][:5]:
                o = str(setup['root'] / 'single.json')
                ir.main(['--merged-model', setup['model'], '--audio', p, '--output-json', o]
                        + (['--smooth'] if smooth else []))
                out[(p, smooth)] = json.load(open(o))
    finally:
        ir.load_merged_model = real_load
    return out


@pytest.mark.parametrize('smooth', [False, True])
def test_catalogue_records_equal_single_file_main(setup, oracle, smooth):
    import catalog_runner as cr
    out = str(setup['root'] / f'scan_{int(smooth)}.json')
    recs = cr.main(['--merged-model', setup['model'], '--audio-dir', setup['folder'], '--output-json', out,
                    '--batch-size', '4', '--pack-seconds', str(cat.PACK_SECONDS)] + (['--smooth'] if smooth else []))
    on_disk = json.load(open(out))
    assert on_disk == recs
    paths = setup['paths']
    assert [r['filename'] for r in on_disk] == paths == sorted(paths)
    for rec, p in zip(on_disk[:4], paths[:4]):
        ref = oracle[(p, smooth)]
        assert list(rec) == list(ref) == ['filename', 'segments', 'percentages']
        assert rec['segments'] == ref['segments'] and len(rec['segments']) >= 1
        assert list(rec['percentages']) == list(ref['percentages'])
        for k, v in ref['percentages'].items():
            assert abs(rec['percentages'][k] - v) <= 1e-3, (p, k, rec['percentages'][k], v)
    # c_16k_gap: the silent window in the middle was dropped on the device
    starts = [s['start_sec'] for s in on_disk[2]['segments']]
    assert 8.0 not in starts and 0.0 in starts and 16.0 in starts
    assert on_disk[4] == oracle[(paths[4], smooth)] == {'filename': paths[4], 'segments': [], 'percentages': {}}
    assert list(on_disk[5]) == ['filename', 'error'] and 'RIFF' in on_disk[5]['error']


def test_packed_logits_are_bit_identical_and_one_wait_per_pack(setup):
    """Segments are independent: a window's merged logits do not depend on which
    other windows share its batch or its pack."""
    import inference_runner as ir
    from sad import ingest
    from sad.scan import Scanner
    model, meta = ir.load_merged_model(setup['model'], torch.device(DEV))
    sc = Scanner(model.engine, meta['class_names'], batch_size=4, pack_seconds=cat.PACK_SECONDS, keep_logits=True)
    recs = sc.scan(setup['paths'])
    assert sc.stats['packs'] == 3 and sc.stats['syncs'] == sc.stats['packs'] + 1  # + the last pack's results
    cfg, spec = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=0.0, silence_threshold=1e-3), \
        ir.SpectrogramConfig()
    total = 0
    for p, rec in zip(setup['paths'][:4], recs):
        wf, sr = ir.preprocess_waveform(p, cfg, DEV)
        starts, _ = ingest.select_windows(wf, sr, cfg.window_size, cfg.overlap, cfg.silence_threshold)
        single = ir.run_windows(model, ingest.Windows(wf, starts, 128000), sr, spec, 128)
        packed = sc.logits[p]
        assert packed.shape == single.shape == (len(rec['segments']), 7)
        assert torch.equal(packed, single), (p, (packed - single).abs().max().item())
        total += len(starts)
    assert sc.stats['segments'] == total and sc.logits[setup['paths'][4]].shape[0] == 0
