"""The small WAV folder the catalogue-scan GPU tests share (not a test module)."""
import os

import numpy as np

from conftest import GOLDEN

NAMES = [f'Synthetic{chr(65 + i)}' for i in range(6)] + ['Real']
READABLE = ['a_32k_mono.wav', 'b_44k_stereo.wav', 'c_16k_gap.wav', 'd_short.wav']
SILENT = 'e_silent.wav'
GARBAGE = 'f_garbage.wav'
# 30 s packs: [a (12 s), b (5.8 s)], [c (20 s), d (4 s)], [e (6.25 s)]
PACK_SECONDS = 30


def write_catalogue(folder) -> list:
    """Six files, sorted by name: 32 kHz mono with 3 windows; 44.1 kHz stereo;
    16 kHz mono with 12 s of silence in the middle (the 8-12 s window is silent
    whatever the resampler rings into its neighbours); a clip shorter than 4 s;
    an all-silent file; garbage bytes.  Returns the sorted paths."""
    from sad.audio import save_pcm16
    pcm = np.load(os.path.join(GOLDEN, 'golden_frontend.npz'))['pcm']
    folder = str(folder)
    save_pcm16(os.path.join(folder, READABLE[0]), np.concatenate([pcm[0], pcm[1], pcm[2]]))
    save_pcm16(os.path.join(folder, READABLE[1]), np.stack([np.concatenate([pcm[0], pcm[1]]),
                                                            np.concatenate([pcm[2], pcm[3]])]), 44100)
    save_pcm16(os.path.join(folder, READABLE[2]),
               np.concatenate([pcm[3][:64000], np.zeros(192000, np.int16), pcm[0][:64000]]), 16000)
    save_pcm16(os.path.join(folder, READABLE[3]), pcm[1][:77777])
    save_pcm16(os.path.join(folder, SILENT), np.zeros(200000, np.int16))
    with open(os.path.join(folder, GARBAGE), 'wb') as f:
        f.write(bytes(range(256)) * 40)
    return sorted(os.path.join(folder, n) for n in READABLE + [SILENT, GARBAGE])


def write_model(path) -> str:
    import torch
    from conftest import merged_sd
    torch.save({'state_dict': merged_sd('n6'), 'metadata': {'class_names': NAMES}}, str(path))
    return str(path)
