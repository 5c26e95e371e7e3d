#!/usr/bin/env python3
"""Golden fixture for the waveform augmentation contract (tests/waveaug_ref.py),
made by calling the REFERENCE's own functions (``modular/source/
audio_augmneter.py:79-137``) and its clip (``:190``) on the CPU.

Run only in the build container (it reads /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_waveaug.py

The reference module imports librosa and soundfile, which are not installed:
empty stub modules are registered (the five kinds that call librosa are out of
scope and are not called), then ``audio_augmneter`` is imported unchanged.  Each
function draws its parameters with ``np.random.uniform(min, max)``; it is
called with min = max, so every parameter is pinned.  The signals are float32,
as ``librosa.load`` hands them over: seeded noise at 8 kHz, an int16-grid signal
at 32 kHz, a full-scale square wave and an impulse at 44.1 kHz, and a
one-sample file.  ``add_white_noise`` is not recorded: its noise is numpy's
generator, which the contract replaces.  Only data is written
(tests/golden/golden_waveaug.npz: inputs, parameters, outputs); no reference
source or bytecode.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF_SRC = '/root/reference/modular/source'

PARAMS = dict(amount=0.3, trem_rate=4.5, trem_depth=0.4, ph_rate=0.7, ph_depth=0.8)
SHIFTS = (0.01, -0.01, 0.0, 1e-6, 0.2, -0.2)


def import_reference():
    for name in ('librosa', 'soundfile', 'tqdm'):
        try:
            __import__(name)
        except Exception:
            mod = types.ModuleType(name)
            if name == 'tqdm':
                mod.tqdm = lambda it, **k: it
            sys.modules[name] = mod
    sys.path.insert(0, REF_SRC)
    import audio_augmneter as ref  # noqa
    sys.path.remove(REF_SRC)
    return ref


def signals():
    rng = np.random.default_rng(20250101)
    sq = np.where((np.arange(4096) // 37) % 2 == 0, 1.0, -1.0)
    imp = np.zeros(2000)
    imp[0] = 1.0
    return {
        'noise8k': (8000, (0.3 * rng.standard_normal(3000)).astype(np.float32)),
        'grid32k': (32000, (rng.integers(-32768, 32768, size=4000) / 32768.0).astype(np.float32)),
        'square44k': (44100, sq.astype(np.float32)),
        'impulse44k': (44100, imp.astype(np.float32)),
        'one32k': (32000, np.array([0.625], np.float32)),
    }


def main():
    ref = import_reference()
    out = {'names': np.array(list(signals())), 'shifts': np.array(SHIFTS),
           **{f'param_{k}': np.float64(v) for k, v in PARAMS.items()}}
    for name, (sr, y) in signals().items():
        out[f'{name}/sr'] = np.int64(sr)
        out[f'{name}/y'] = y
        a = PARAMS['amount']
        out[f'{name}/dynamic_range_compression'] = np.clip(
            ref.augment_dynamic_range_compression(y.copy(), a, a)[0], -1.0, 1.0)
        r, d = PARAMS['trem_rate'], PARAMS['trem_depth']
        out[f'{name}/tremolo'] = np.clip(ref.augment_tremolo(y.copy(), sr, r, r, d, d)[0], -1.0, 1.0)
        r, d = PARAMS['ph_rate'], PARAMS['ph_depth']
        out[f'{name}/phaser'] = np.clip(ref.augment_phaser(y.copy(), sr, r, r, d, d)[0], -1.0, 1.0)
        for k, s in enumerate(SHIFTS):
            out[f'{name}/time_shift{k}'] = np.clip(ref.augment_time_shift(y.copy(), sr, s, s)[0], -1.0, 1.0)
    path = os.path.join(HERE, 'golden_waveaug.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: (v.dtype, v.shape) for k, v in out.items() if '/' in k
                                                   and k.startswith('noise8k')})


if __name__ == '__main__':
    main()
