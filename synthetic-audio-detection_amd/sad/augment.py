"""Host-side sampling of the trainer's random augmentation parameters.

The reference draws these inside ``SpectrogramDataset.__getitem__`` with torch's
global RNG (DataLoader workers): torchaudio ``FrequencyMasking(15)`` /
``TimeMasking(35)`` (``submodel_trainer.py:108-114,195-196``) and torchvision
``RandomResizedCrop(512, scale=(0.8, 1.0))`` (``:465-467``).  Only the integer
parameters are drawn here (same formulas, same RNG calls in the same order);
the masking, standardisation and crop-resize arithmetic run on the device
(``sad_specaug_norm_run`` / ``sad_crop_resize_run``).
"""
from __future__ import annotations

import math

import torch

FREQ_MASK_PARAM = 15
TIME_MASK_PARAM = 35
CROP_SCALE = (0.8, 1.0)
CROP_RATIO = (3.0 / 4.0, 4.0 / 3.0)


def mask_range(axis_len: int, mask_param: int, generator: torch.Generator | None = None):
    """torchaudio.functional.mask_along_axis (p = 1.0): returns the masked
    half-open index range [start, end) along one axis."""
    value = torch.rand(1, generator=generator) * mask_param
    min_value = torch.rand(1, generator=generator) * (axis_len - value)
    start = int(min_value.long().item())
    end = int((min_value.long() + value.long()).item())
    return start, end


def specaug_masks(n_mels: int = 128, n_frames: int = 251, generator: torch.Generator | None = None):
    """(f0, f1, t0, t1): FrequencyMasking then TimeMasking, as applied by the
    reference's nn.Sequential (frequency first)."""
    f0, f1 = mask_range(n_mels, FREQ_MASK_PARAM, generator)
    t0, t1 = mask_range(n_frames, TIME_MASK_PARAM, generator)
    return f0, f1, t0, t1


def random_resized_crop_params(height: int = 512, width: int = 512, scale=CROP_SCALE, ratio=CROP_RATIO,
                               generator: torch.Generator | None = None):
    """torchvision RandomResizedCrop.get_params -> (i, j, h, w)."""
    area = height * width
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1], generator=generator).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0].item(), log_ratio[1].item(),
                                                         generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = int(torch.randint(0, height - h + 1, size=(1,), generator=generator).item())
            j = int(torch.randint(0, width - w + 1, size=(1,), generator=generator).item())
            return i, j, h, w
    # fallback to the central crop
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


FULL_IMAGE = (0, 0, 512, 512)
NO_MASK = (0, 0, 0, 0)


# ------------------------------------------------------- waveform augmentation
# submodel_trainer.py --wave-augment: the reference's audio_augmneter.py writes
# eleven variants of every recording to disk ahead of training; here one kind is
# drawn per file and per visit and applied on the device (csrc/waveaug.hip).  The
# index of a name in WAVE_KINDS is the library's kind code (include/sad.h).
WAVE_KINDS = ('original', 'dynamic_range_compression', 'add_white_noise', 'tremolo', 'phaser', 'time_shift')
# the kinds of librosa's phase vocoder: not kinds of --wave-augment but of --wave-stretch (STRETCH_KINDS below)
WAVE_UNSUPPORTED = ('speed_up', 'slow_down', 'pitch_up', 'pitch_down', 'time_pitch_shift')
WAVE_PHASER_MIN_SR = 5000   # the phaser's 2500 Hz stage leaves the unit circle at and below this rate
WAVE_SHIFT_MARGIN = 0.5     # seconds: the largest |shift| (audio_augmneter.py:129)
# the reference's ranges (audio_augmneter.py:79-129)
WAVE_RANGES = {'amount': (0.01, 0.5), 'vol': (0.001, 0.05), 'trem_rate': (3.0, 6.0), 'trem_depth': (0.2, 0.5),
               'ph_depth': (0.5, 0.9), 'ph_rate': (0.1, 1.0), 'shift': (-0.5, 0.5)}


def parse_wave_kinds(text: str):
    """'all' or comma-separated names out of WAVE_KINDS -> tuple of names, in
    WAVE_KINDS' order, each once.  ValueError names the supported set."""
    supported = ', '.join(WAVE_KINDS)
    names = [n.strip() for n in str(text).split(',') if n.strip()]
    if not names:
        raise ValueError(f'no augmentation kind given; supported: {supported}, or all')
    if names == ['all']:
        return WAVE_KINDS
    for n in names:
        if n in WAVE_UNSUPPORTED:
            raise ValueError(f'{n} is not supported here (it is a kind of --wave-stretch); supported: {supported}')
        if n not in WAVE_KINDS:
            raise ValueError(f'unknown augmentation kind {n!r}; supported: {supported}')
    return tuple(k for k in WAVE_KINDS if k in names)


def _uniform(lo_hi, generator):
    return torch.empty(1).uniform_(lo_hi[0], lo_hi[1], generator=generator).item()


def wave_aug_params(kinds, sr: int, generator: torch.Generator | None = None):
    """One draw for one file: a kind uniformly from `kinds` (a file at or below
    WAVE_PHASER_MIN_SR draws among the others), then that kind's parameters from
    the reference's ranges, in the reference's order -> (kind code, p0, p1, key):
    (amount) | (vol, key) | (rate, depth) | (rate, depth), depth drawn first | (s),
    s = int(shift * sr) frames."""
    cands = [k for k in kinds if k != 'phaser' or sr > WAVE_PHASER_MIN_SR] or ['original']
    # (a single candidate needs no draw: --wave-augment original draws nothing at all)
    kind = cands[int(torch.randint(0, len(cands), (1,), generator=generator).item())] if len(cands) > 1 else cands[0]
    p0 = p1 = 0.0
    key = 0
    if kind == 'dynamic_range_compression':
        p0 = _uniform(WAVE_RANGES['amount'], generator)
    elif kind == 'add_white_noise':
        p0 = _uniform(WAVE_RANGES['vol'], generator)
        key = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64, generator=generator).item())
    elif kind == 'tremolo':
        p0 = _uniform(WAVE_RANGES['trem_rate'], generator)
        p1 = _uniform(WAVE_RANGES['trem_depth'], generator)
    elif kind == 'phaser':
        p1 = _uniform(WAVE_RANGES['ph_depth'], generator)
        p0 = _uniform(WAVE_RANGES['ph_rate'], generator)
    elif kind == 'time_shift':
        p0 = float(int(_uniform(WAVE_RANGES['shift'], generator) * sr))
    return WAVE_KINDS.index(kind), p0, p1, key


# ------------------------------------------------------------ time and pitch
# submodel_trainer.py --wave-stretch: the five kinds that change tempo and pitch
# (csrc/stretch.hip; the float64 contract is tests/stretch_ref.py).  Kind codes
# continue WAVE_KINDS': STRETCH_CODE0 + the index in STRETCH_KINDS.
STRETCH_KINDS = WAVE_UNSUPPORTED
STRETCH_CODE0 = len(WAVE_KINDS)
# the reference's ranges (audio_augmneter.py:55-76, 140-145)
STRETCH_RANGES = {'speed_up': (1.0, 1.5), 'slow_down': (0.5, 1.0), 'pitch_up': (0.0, 2.0), 'pitch_down': (-2.0, 0.0),
                  'tps_rate': (0.8, 1.2), 'tps_steps': (-1.0, 1.0)}


def parse_stretch_kinds(text: str):
    """'all' or comma-separated names out of STRETCH_KINDS -> tuple of names, in
    STRETCH_KINDS' order, each once.  ValueError names the supported set."""
    supported = ', '.join(STRETCH_KINDS)
    names = [n.strip() for n in str(text).split(',') if n.strip()]
    if not names:
        raise ValueError(f'no stretch kind given; supported: {supported}, or all')
    if names == ['all']:
        return STRETCH_KINDS
    for n in names:
        if n in WAVE_KINDS:
            raise ValueError(f'{n} is a kind of --wave-augment; supported here: {supported}')
        if n not in STRETCH_KINDS:
            raise ValueError(f'unknown stretch kind {n!r}; supported: {supported}')
    return tuple(k for k in STRETCH_KINDS if k in names)


def stretch_aug_params(kind: str, generator: torch.Generator | None = None):
    """The parameters of one stretch kind from the reference's ranges, in the
    reference's order -> (kind code, p0, p1, 0): (rate) | (steps) | (rate, steps),
    the rate drawn first."""
    p1 = 0.0
    if kind == 'time_pitch_shift':
        p0 = _uniform(STRETCH_RANGES['tps_rate'], generator)
        p1 = _uniform(STRETCH_RANGES['tps_steps'], generator)
    else:
        p0 = _uniform(STRETCH_RANGES[kind], generator)
    return STRETCH_CODE0 + STRETCH_KINDS.index(kind), p0, p1, 0


def wave_stretch_params(wave_kinds, stretch_kinds, sr: int, generator: torch.Generator | None = None):
    """One draw for one file with --wave-stretch: a kind uniformly from the union
    of both lists (a file at or below WAVE_PHASER_MIN_SR draws among the others),
    then that kind's parameters -> (kind code, p0, p1, key) as wave_aug_params
    gives them.  Without stretch kinds this is wave_aug_params, draw for draw."""
    if not stretch_kinds:
        return wave_aug_params(wave_kinds, sr, generator)
    cands = [k for k in tuple(wave_kinds or ()) if k != 'phaser' or sr > WAVE_PHASER_MIN_SR] + list(stretch_kinds)
    kind = cands[int(torch.randint(0, len(cands), (1,), generator=generator).item())] if len(cands) > 1 else cands[0]
    if kind in STRETCH_KINDS:
        return stretch_aug_params(kind, generator)
    return wave_aug_params((kind,), sr, generator)   # (a one-kind list draws no kind)
