#!/usr/bin/env python3
"""Drop-in replacement for the reference's ``modular/source/submodel_trainer.py``
on MI355X: same CLI flags and defaults, same module symbols, same checkpoint
format (``model_best.pth``: epoch / state_dict / best_acc / optimizer /
scheduler / total_steps); the device work runs on libsad (HIP, gfx950) through
``sad.train``.

Reference map (file:line in modular/source/submodel_trainer.py):
  parse_args / setup_logging     :33-66
  SpectrogramDataset             :69-218  -> file discovery, WAV load, resample and
                                             the 2-segment rules on the host; the
                                             spectrogram chain runs on the device
  custom_collate_fn              :221-238
  train / validate / evaluate    :241-460
  get_dataloaders                :463-511
  initialize_weights, get_model  :514-528
  main                           :531-727

Behaviour kept on purpose: the attached head is never
used, the loss is CrossEntropy over the 512 pooled features (C1); layer3 is
unfrozen at epochs//3 but never optimised, its gradients accumulate and enter
the clip norm (C4); mel norm=None (C3); the epoch loss divides the sum of
loss*2B by the number of FILES (:285,304).

Differences (documented in DESIGN.md / INTEGRATION.md):
  * ``SpectrogramDataset.__getitem__`` returns the two fp32 waveform segments
    and their drawn augmentation parameters instead of finished [3,512,512]
    images: ``(seg1 [128000], target, seg2 [128000], target, aug int32 [2, 8])``
    with aug[k] = (f0, f1, t0, t1, i, j, h, w).  The device builds the images.
  * ``--num_gpus > 1`` = one process per GPU (torchrun) over RCCL instead of
    DataParallel threads: each rank loads ``--batch-size`` files per step;
    per-replica BN statistics as in DP; gradients all-reduced.
  * no CPU fallback; ``--model-name`` must be resnet18 / resnet34 (timm's
    BasicBlock) or resnet50 / resnet101 / resnet152 (Bottleneck): the device
    forward and backward implement those two block types.
  * extra flags: ``--precision {bf16,mixed,fp32}`` (default bf16 = throughput
    mode; mixed = the frozen stem/layers 1-3 in fp32 and layer4 in bf16, whose
    layer4 gradients track fp32 autograd to cosine >= 0.95),
    ``--max-steps`` (stop an epoch early; benchmarking), ``--head-loss``
    (CrossEntropy and accuracy through model.head, trained with layer4: the
    BinaryClassifier the merger and inference use; off by default, so C1 is
    reproduced unless asked for), ``--trunk CHECKPOINT`` (resnet18, bf16 or
    fp32: conv1, bn1 and layer1-3 come from CHECKPOINT and run frozen in eval
    mode on the inference plan's trunk entry; sub-models trained on one trunk
    and merged with ``model_merger.py --keep-backbone`` run it once at
    inference).
  * ``--device-ingest`` (off by default): a second input path.  The default
    path reads, decodes and resamples every whole file in a DataLoader worker
    and ships 2 x 128,000 fp32 values per file through the loader's queue; with
    the flag, ``StoredSampleDataset`` decides the segment rule from the WAV
    header, reads only the frames the two segments need, as stored,
    ``stored_collate_fn`` packs the batch into one byte arena with its file and
    tile tables, and ``sad.ingest.TrainIngest`` turns it into the same
    [2B, 128000] tensor with one upload and one launch (csrc/ingest.hip,
    sad_train_ingest_run).  Same files, segments and augmentation draws;
    an extension over the host path: 2-64 channel files are mixed to mono as
    the inference path does instead of being skipped.  Its workers come from a
    fork server and persist across epochs (get_dataloaders says why).
  * ``--wave-augment LIST`` (with ``--device-ingest``; off by default): the
    reference trains on a tree that ``audio_augmneter.py`` wrote ahead of time,
    eleven variants per recording.  With the flag the train split draws, per
    file and per epoch, one kind out of LIST (original,
    dynamic_range_compression, add_white_noise, tremolo, phaser, time_shift, or
    ``all``) with parameters from the reference's ranges, and the device applies
    it to the stored samples before they are resampled (csrc/waveaug.hip,
    sad_wave_augment_run).  Not reproduced: the tool's resample to 44.1 kHz,
    its 16-bit file round trip, numpy's normal generator; the noise's RMS runs
    over the frames read.
  * ``--wave-stretch LIST`` (with ``--device-ingest``, with or without
    ``--wave-augment``; off by default): the tool's other five kinds, the ones
    that go through librosa (speed_up, slow_down, pitch_up, pitch_down,
    time_pitch_shift, or ``all``).  The kind is drawn from the union of both
    lists; a phase vocoder and a resampler on the device apply it
    (csrc/stretch.hip, sad_wave_stretch_run).  The contract is our own float64
    restatement of librosa's documented algorithm (tests/stretch_ref.py), not
    pinned to librosa; the pitch shift's resampler is the ingestion's windowed
    sinc, not soxr.
  * TensorBoard is optional (not installed here): scalars are logged instead.
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import sys
import warnings
from datetime import datetime

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from sad import audio as _audio  # noqa: E402
from sad import augment as _augment  # noqa: E402

warnings.filterwarnings("ignore")

SEGMENT_LENGTH = 4 * 32000
# timm.list_models('resnet*') is unavailable offline: the choices the reference's
# CLI accepts for --model-name (timm 0.9 names); resnet18 / resnet34 (BasicBlock) and
# resnet50 / resnet101 / resnet152 (Bottleneck) train on the device (sad.weights.ARCHS).
RESNET_MODELS = ['resnet10t', 'resnet14t', 'resnet18', 'resnet18d', 'resnet26', 'resnet26d', 'resnet26t',
                 'resnet32ts', 'resnet33ts', 'resnet34', 'resnet34d', 'resnet50', 'resnet50_gn', 'resnet50d',
                 'resnet50t', 'resnet51q', 'resnet61q', 'resnet101', 'resnet101d', 'resnet152', 'resnet152d',
                 'resnet200', 'resnet200d']


def parse_args(argv=None):
    """Parses command-line arguments (:33-53)."""
    parser = argparse.ArgumentParser(description='Audio Classification Training')
    parser.add_argument('--data-dir', default='./dataset', type=str, help='Path to dataset')
    parser.add_argument('--batch-size', default=32, type=int, help='Batch size per GPU')
    parser.add_argument('--epochs', default=100, type=int, help='Number of total epochs to run')
    parser.add_argument('--lr', default=0.001, type=float, help='Initial learning rate')
    parser.add_argument('--workers', default=20, type=int, help='Number of data loading workers')
    parser.add_argument('--seed', default=42, type=int, help='Seed for initializing training.')
    parser.add_argument('--gpu', default=0, type=int, help='GPU id to use.')
    parser.add_argument('--num_gpus', default=1, type=int, help='Number of GPUs to use')
    parser.add_argument('--checkpoint-dir', default='./checkpoints', type=str, help='Directory to save checkpoints')
    parser.add_argument('--resume', default='', type=str, help='Path to resume checkpoint')
    parser.add_argument('--evaluate', dest='evaluate', action='store_true', help='Evaluate model on validation set')
    parser.add_argument('--Class0', default='Real', type=str, help='Name of Class 0 eg. Real')
    parser.add_argument('--Class1', default='Class1', type=str, help='Name of Class 1 eg. Training platform')
    parser.add_argument('--model-name', default='resnet18', type=str, choices=RESNET_MODELS,
                        help='Name of model to use')
    parser.add_argument('--precision', default='bf16', choices=['bf16', 'mixed', 'fp32'],
                        help='device compute precision (fp32 = the reference arithmetic; mixed = fp32 frozen prefix '
                             '+ bf16 layer4)')
    parser.add_argument('--max-steps', default=0, type=int, help='stop each epoch after this many steps (0 = all)')
    parser.add_argument('--head-loss', action='store_true',
                        help='train through model.head: CrossEntropy and accuracy on the BinaryClassifier head\'s two '
                             'logits (train-mode BN + dropout), the head trained with layer4.  Default off: the '
                             'reference computes them on the 512 pooled features and never calls the head (quirk C1)')
    parser.add_argument('--trunk', default='', type=str, metavar='CHECKPOINT',
                        help='trainer checkpoint whose conv1, bn1 and layer1-3 (parameters and BN statistics) are '
                             'loaded after the seeded init and stay frozen in eval mode; layer4 and the head train as '
                             'usual.  resnet18 with --precision bf16 or fp32 only')
    parser.add_argument('--device-ingest', action='store_true',
                        help='second input path: the DataLoader workers read only the frames of each file that the '
                             'two 4 s segments need, as stored (int16 stays int16); one upload and one kernel launch '
                             'per batch do the mono mix, the resampling to 32 kHz and the segment cut on the device.  '
                             'Same segments and augmentation draws as the default host path (bit-identical for '
                             '32 kHz mono files).  An extension over the host path: files of 2-64 channels are mixed '
                             'to mono as the inference path does, where the host path skips them with a warning')
    parser.add_argument('--wave-augment', default='', type=str, metavar='LIST',
                        help='waveform augmentation of the train split on the device (needs --device-ingest): per file '
                             'and per epoch one kind is drawn uniformly from LIST, with parameters from the ranges of '
                             'the reference\'s audio_augmneter.py, and applied to the stored samples before they are '
                             f'resampled.  LIST: comma-separated names out of {", ".join(_augment.WAVE_KINDS)}, or '
                             f'all.  ({", ".join(_augment.WAVE_UNSUPPORTED)}: see --wave-stretch.)  Validation and '
                             '--evaluate are never augmented')
    parser.add_argument('--wave-stretch', default='', type=str, metavar='LIST',
                        help='time-stretch and pitch-shift augmentation of the train split on the device (needs '
                             '--device-ingest; works with or without --wave-augment): the kind of a file is drawn '
                             'uniformly from the union of both lists, its rate / semitone steps from the ranges of the '
                             f'reference\'s audio_augmneter.py.  LIST: comma-separated names out of '
                             f'{", ".join(_augment.STRETCH_KINDS)}, or all.  Validation and --evaluate are never '
                             'augmented')
    args = parser.parse_args(argv)
    if args.wave_augment:
        if not args.device_ingest:
            parser.error('--wave-augment needs --device-ingest: the augmentation runs on the stored samples that '
                         'the device ingestion uploads')
        try:
            args.wave_augment = _augment.parse_wave_kinds(args.wave_augment)
        except ValueError as e:
            parser.error(f'--wave-augment: {e}')
    else:
        args.wave_augment = None
    if args.wave_stretch:
        if not args.device_ingest:
            parser.error('--wave-stretch needs --device-ingest: the stretch runs on the stored samples that the '
                         'device ingestion uploads')
        try:
            args.wave_stretch = _augment.parse_stretch_kinds(args.wave_stretch)
        except ValueError as e:
            parser.error(f'--wave-stretch: {e}')
    else:
        args.wave_stretch = None
    if args.trunk:
        if args.model_name != 'resnet18':
            parser.error(f'--trunk needs --model-name resnet18 (got {args.model_name}): the frozen trunk runs on '
                         'the tuned ResNet-18 inference plan')
        if args.precision not in ('bf16', 'fp32'):
            parser.error(f'--trunk needs --precision bf16 or fp32 (got {args.precision}): the frozen trunk runs in '
                         'the precision of layer4')
    return args


def setup_logging():
    """Sets up logging configuration (:56-66)."""
    os.makedirs('logs', exist_ok=True)
    logging.basicConfig(
        filename=f'logs/training_{datetime.now().strftime("%Y%m%d-%H%M%S")}.log',
        level=logging.INFO,
        format='%(asctime)s %(message)s',
    )
    console = logging.StreamHandler()
    console.setLevel(logging.INFO)
    logging.getLogger('').addHandler(console)


def segment_waveform(waveform: torch.Tensor, min_length_ratio: float = 0.9):
    """The two training segments of one file (:155-187), or None if too short."""
    seg = SEGMENT_LENGTH
    n = waveform.size(1)
    if n >= 2 * seg:
        return [waveform[:, :seg], waveform[:, seg:2 * seg]]
    if n >= seg:
        first = waveform[:, :seg]
        return [first, first]
    if n >= seg * min_length_ratio:
        padded = torch.nn.functional.pad(waveform, (0, seg - n), mode='constant', value=0)
        return [padded, padded]
    return None


class SpectrogramDataset(Dataset):
    """Dataset of 2-segment training samples (:69-218); see the module docstring
    for what __getitem__ returns."""

    def __init__(self, data_dir, mode, transform=None, class_names=None):
        self.mode = mode
        # 'train' -> RandomResizedCrop(512, scale=(0.8, 1.0)) (:465-467); anything else
        # (the val transform Resize((512,512)), :469-471) -> the full image.
        self.transform = transform
        self.classes = ['Real', 'Class1'] if class_names is None else class_names
        self.class_to_idx = {cls_name: i for i, cls_name in enumerate(self.classes)}
        self.samples = self._make_dataset(data_dir)
        logging.info(f"Found {len(self.samples)} samples for mode {self.mode}")
        logging.info(f"Classes: {self.classes}")
        logging.info(f"Class-to-Index Mapping: {self.class_to_idx}")
        self.augment = self.mode == 'train'
        self.min_length_ratio = 0.9

    def _make_dataset(self, directory):
        """(path, class index) for every .wav under <dir>/<mode>/<class>/ (:118-137)."""
        instances = []
        for target_class in self.classes:
            class_index = self.class_to_idx[target_class]
            target_dir = os.path.join(directory, self.mode, target_class)
            if not os.path.isdir(target_dir):
                logging.warning(f"Directory {target_dir} does not exist. Skipping.")
                continue
            for root, _, fnames in sorted(os.walk(target_dir)):
                for fname in sorted(fnames):
                    if fname.endswith('.wav'):
                        instances.append((os.path.join(root, fname), class_index))
        if not instances:
            raise RuntimeError(f"No wav files found in {directory}/{self.mode}")
        return instances

    def _aug_params(self):
        """Per segment, in the reference's RNG order (:190-206): the SpecAugment
        masks, then self.transform's RandomResizedCrop parameters."""
        rows = []
        for _ in range(2):
            mask = _augment.specaug_masks() if self.augment else _augment.NO_MASK
            box = _augment.random_resized_crop_params() if self.transform == 'train' else _augment.FULL_IMAGE
            rows.append(list(mask) + list(box))
        return torch.tensor(rows, dtype=torch.int32)

    def __getitem__(self, index):
        path, target = self.samples[index]
        try:
            waveform, sample_rate = _audio.load(path)
            if waveform.numel() == 0:
                logging.debug(f"Empty waveform detected at index {index} for path {path}")
                return None
            if sample_rate != 32000:
                waveform = _audio.resample(waveform, sample_rate, 32000)
            if waveform.size(0) != 1:
                # the reference would build a [2C,...] image that the 3-channel model rejects
                raise ValueError(f'expected mono audio, got {waveform.size(0)} channels')
            segs = segment_waveform(waveform, self.min_length_ratio)
            if segs is None:
                logging.debug(f"File too short at index {index}, path {path}. Length: {waveform.size(1)}, "
                              f"Required: {2 * SEGMENT_LENGTH}")
                return None
            aug = self._aug_params()
            return segs[0][0].contiguous(), target, segs[1][0].contiguous(), target, aug
        except Exception as e:
            logging.warning(f"Error processing file at index {index}, path {path}: {str(e)}")
            return None

    def __len__(self):
        return len(self.samples)


class StoredSampleDataset(SpectrogramDataset):
    """``--device-ingest``: the same files, labels, segment rule and
    augmentation draws as SpectrogramDataset, but __getitem__ decides from the
    WAV header alone, reads only the frames the two segments need, as stored,
    and returns a ``sad.ingest.StoredFile`` (or None); the device resamples
    and cuts the segments (``sad.ingest.TrainIngest``).  Unlike the host path
    it takes files of 1-64 channels (mixed to mono as the inference path does).

    ``wave_kinds`` (``--wave-augment``; None = off, and then nothing below
    differs): a tuple of names out of ``sad.augment.WAVE_KINDS``.  Per visit one
    kind and its parameters are drawn AFTER the SpecAugment and crop draws, so
    those read the same as without the flag; with ``time_shift`` in the list the
    worker reads half a second more, the samples a left shift brings in.

    ``stretch_kinds`` (``--wave-stretch``; None = off, and then nothing differs):
    a tuple out of ``sad.augment.STRETCH_KINDS``.  The one kind of a visit is then
    drawn from the union of both tuples, still after the SpecAugment and crop
    draws but BEFORE the read, because a stretch decides how much of the file the
    two segments depend on (``sad.ingest.stretch_need_frames``).  Without the flag
    the draws stay where they were, after the read: a file whose read fails has
    always been dropped without consuming a draw, and moving the draws would
    change the sequence of every later file of that worker.  The segment rule
    (two / first / pad / drop) that decides whether the file is kept is applied to
    the file's own length, before the draw; the device then cuts the segments
    from the stretched length.  A file that speed_up brings below 0.9 segments is
    therefore kept and zero-padded, where a tree written ahead of time by the
    reference's tool would hold a variant that the trainer drops."""
    wave_kinds = None
    stretch_kinds = None

    def __getitem__(self, index):
        from sad import ingest as _ingest
        path, target = self.samples[index]
        try:
            frames, channels, sample_rate, _, _, _ = _audio.wav_header(path)
            if frames == 0:
                logging.debug(f"Empty waveform detected at index {index} for path {path}")
                return None
            if not 1 <= channels <= 64:
                raise ValueError(f'expected 1-64 channels, got {channels}')
            if not _ingest.train_rate_supported(sample_rate, 32000):
                raise ValueError(f'sample rate {sample_rate} Hz is not supported by the device ingestion')
            n = _ingest.train_out_len(frames, sample_rate, 32000)
            if _ingest.train_segment_rule(n, SEGMENT_LENGTH, self.min_length_ratio) is None:
                logging.debug(f"File too short at index {index}, path {path}. Length: {n}, "
                              f"Required: {2 * SEGMENT_LENGTH}")
                return None
            need = _ingest.train_need_frames(sample_rate, SEGMENT_LENGTH, 32000)
            aug = wave = None
            if self.stretch_kinds:  # the draw sets how much is read; without the flag: after the read, as ever
                aug = self._aug_params()
                wave = _augment.wave_stretch_params(self.wave_kinds, self.stretch_kinds, sample_rate)
            if wave is not None and wave[0] >= _ingest.STRETCH_CODE0:
                need = _ingest.stretch_need_frames(wave[0], wave[1], wave[2], need)
            elif self.wave_kinds and 'time_shift' in self.wave_kinds:
                need += int(_augment.WAVE_SHIFT_MARGIN * sample_rate)
            samples, _, _ = _audio.read_wav(path, max_frames=min(frames, need))
            if samples.shape[0] != min(frames, need) * channels:
                raise ValueError('the data chunk is shorter than its header says')
            if not self.stretch_kinds:
                aug = self._aug_params()
                wave = _augment.wave_aug_params(self.wave_kinds, sample_rate) if self.wave_kinds else None
            return _ingest.StoredFile(samples, frames, channels, sample_rate, target, aug, wave)
        except Exception as e:
            logging.warning(f"Error processing file at index {index}, path {path}: {str(e)}")
            return None


def stored_collate_fn(batch):
    """``--device-ingest``: drops None samples as custom_collate_fn does; the
    rest become one ``sad.ingest.StoredBatch`` (one byte arena + tables) or None."""
    from sad import ingest as _ingest
    return _ingest.collate_stored(batch, SEGMENT_LENGTH, 32000)


def custom_collate_fn(batch):
    """Drops None samples (:221-238); returns (wave1 [B,T], target1, wave2,
    target2, aug [B,2,8]) or None."""
    batch = list(filter(lambda x: x is not None, batch))
    if len(batch) == 0:
        return None
    input1, target1, input2, target2, aug = zip(*batch)
    return (torch.stack(input1), torch.tensor(target1), torch.stack(input2), torch.tensor(target2),
            torch.stack(aug))


class _Scalars:
    """Stand-in for torch.utils.tensorboard.SummaryWriter (tensorboard absent)."""

    def __init__(self, log_dir=None):
        self.log_dir = log_dir

    def add_scalar(self, tag, value, step):
        logging.debug(f'{tag} {value} @ {step}')

    def close(self):
        pass


def _summary_writer(log_dir):
    try:
        from torch.utils.tensorboard import SummaryWriter
        return SummaryWriter(log_dir=log_dir)
    except Exception:
        return _Scalars(log_dir)


class DeviceModel:
    """What the reference's ``model`` object is to train()/validate(): the
    device trainer + front end, rank/world of this process."""

    def __init__(self, trainer, frontend, rank=0, world=1, group=None):
        self.trainer, self.frontend = trainer, frontend
        self.rank, self.world, self.group = rank, world, group
        self._ingest = None  # sad.ingest.TrainIngest, made when the first StoredBatch arrives

    def _waves(self, batch):
        """(waves [2B, 128000] fp32 on the device, targets [2B], aug [B, 2, 8]) of
        either batch type, rows in the order first segments, second segments."""
        from sad import ingest as _ingest
        if isinstance(batch, _ingest.StoredBatch):  # --device-ingest
            if self._ingest is None:
                self._ingest = _ingest.TrainIngest(self.trainer.device)
            return self._ingest.segments(batch), torch.cat((batch.targets, batch.targets), dim=0), batch.aug
        input1, target1, input2, target2, aug = batch
        waves = torch.cat((input1, input2), dim=0).to(self.trainer.device, non_blocking=True)
        return waves, torch.cat((target1, target2), dim=0), aug

    def images(self, batch, train: bool):
        waves, targets, aug = self._waves(batch)
        aug = torch.cat((aug[:, 0], aug[:, 1]), dim=0)
        masks = aug[:, :4] if train else None
        boxes = aug[:, 4:] if train else None
        return self.frontend(waves, masks, boxes), targets

    def maps(self, batch):
        waves, targets, _ = self._waves(batch)
        return self.frontend.maps(waves), targets


def _allreduce_sum(values, model):
    if model.world <= 1:
        return values
    import torch.distributed as dist
    dev = 'cpu' if dist.get_backend(model.group) == 'gloo' else model.trainer.device
    t = torch.tensor(values, dtype=torch.float64, device=dev)
    dist.all_reduce(t, group=model.group)
    return t.tolist()


def train(args, train_loader, model, criterion, optimizer, scheduler, epoch, writer, total_steps, device):
    """Performs one epoch of training (:241-313)."""
    running_loss = 0.0
    correct = 0
    total = 0
    tr = model.trainer
    n_files = len(train_loader.dataset)
    for batch_idx, batch in enumerate(train_loader):
        if args.max_steps and batch_idx >= args.max_steps:
            break
        if batch is None:
            continue
        try:
            img, targets = model.images(batch, train=True)
            loss, corr, rows, ok = tr.train_step(img, targets)
            if not ok:
                logging.warning(f'NaN or Inf loss encountered at epoch {epoch}, batch {batch_idx}, skipping step.')
                continue
            total += rows
            correct += corr
            running_loss += loss * rows
            total_steps += 1
            if batch_idx % 10 == 0 and model.rank == 0:
                logging.info(f"Epoch [{epoch}] batch {batch_idx}: loss={loss:.4f} acc={100. * correct / total:.2f}% "
                             f"lr={tr.current_lr:.6f}")
            if total_steps % 100 == 0:
                writer.add_scalar('Loss/train_step', loss, total_steps)
                writer.add_scalar('Accuracy/train_step', 100. * correct / total, total_steps)
                writer.add_scalar('Learning_rate', tr.current_lr, total_steps)
        except Exception as e:
            logging.error(f'Error in training batch {batch_idx}: {str(e)}')
            continue
    # the reference divides by the dataset's file count (each file gave 2 rows, :285,304)
    n_total_files = n_files
    epoch_loss = running_loss / n_total_files if n_total_files > 0 else 0.0
    epoch_acc = 100. * correct / total if total > 0 else 0.0
    if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
        scheduler.step(epoch_loss)
    else:
        scheduler.step()
    return epoch_loss, epoch_acc, total_steps


def _eval_pass(val_loader, model):
    """model.eval() pass: BN folded with the running statistics (the inference
    plan), CE + argmax on the pooled features.  Returns (loss_sum, correct,
    total, predictions, targets) summed over ranks (lists from this rank)."""
    bb = model.trainer.net.eval_backbone()
    from sad.train import ce_loss
    loss_sum = 0.0
    correct = total = 0
    preds, tgts = [], []
    for batch in val_loader:
        if batch is None:
            continue
        maps, targets = model.maps(batch)
        feats = bb(maps)
        if model.trainer.head_loss:  # --head-loss: the head in eval mode on the pooled features
            feats = model.trainer.net.head_forward(feats, train=False)
        _, lc, pred = ce_loss(feats, targets, want_pred=True)
        ls, c = lc.tolist()
        loss_sum += ls
        correct += int(c)
        total += targets.numel()
        preds.extend(pred.cpu().numpy().tolist())
        tgts.extend(targets.numpy().tolist())
    loss_sum, correct, total = _allreduce_sum([loss_sum, correct, total], model)
    preds, tgts = _gather_lists(preds, tgts, model)
    return loss_sum, int(correct), int(total), preds, tgts


def _gather_lists(preds, tgts, model):
    """Every rank's predictions / targets, in rank order (the reference's DP
    evaluates the whole validation set in one process, :354-355)."""
    if model.world <= 1:
        return preds, tgts
    import torch.distributed as dist
    gp, gt = [None] * model.world, [None] * model.world
    dist.all_gather_object(gp, preds, group=model.group)
    dist.all_gather_object(gt, tgts, group=model.group)
    return [p for r in gp for p in r], [t for r in gt for t in r]


def validate(args, val_loader, model, criterion, epoch, device):
    """Performs one epoch of validation (:316-385)."""
    classes = val_loader.dataset.classes
    loss_sum, _, total, preds, tgts = _eval_pass(val_loader, model)
    # the argmax over the 512 pooled features (quirk C1) is clamped to the class
    # range BEFORE it is compared with the target (:345-352), so an index > 1
    # counts as class 1 -- pinned by tests/golden/golden_train.json
    preds = [min(max(p, 0), len(classes) - 1) for p in preds]
    correct = sum(int(p == t) for p, t in zip(preds, tgts))
    epoch_loss = loss_sum / len(val_loader.dataset) if len(val_loader.dataset) > 0 else 0.0
    epoch_acc = 100. * correct / total if total > 0 else 0.0
    logging.info(f"Unique targets in validation: {set(tgts)}")
    logging.info(f"Unique predictions in validation: {set(preds)}")
    try:
        from sklearn.metrics import classification_report
        report = classification_report(tgts, preds, target_names=classes, labels=list(range(len(classes))))
        logging.info(f"\nClassification Report:\n{report}")
    except Exception as e:  # sklearn is reporting only
        logging.info(f'classification report unavailable: {e}')
    return epoch_loss, epoch_acc, preds, tgts


def evaluate(args, model, val_loader, criterion, device):
    """Detailed metrics on the validation set (:388-460)."""
    classes = [args.Class0, args.Class1]
    _, _, _, preds, tgts = _eval_pass(val_loader, model)
    class_correct = [0] * 5
    class_total = [0] * 5
    logging.info("Starting evaluation...")
    for p, t in zip(preds, tgts):
        if t < len(classes):
            class_correct[t] += int(p == t)
            class_total[t] += 1
    accuracy = 100 * sum(class_correct) / sum(class_total) if sum(class_total) > 0 else 0.0
    logging.info("\nEvaluation Results:")
    logging.info(f"Overall Accuracy: {accuracy:.2f}%\n")
    logging.info("Per-class Accuracy:")
    for i in range(len(classes)):
        if class_total[i] > 0:
            logging.info(f"{classes[i]}: {100 * class_correct[i] / class_total[i]:.2f}% "
                         f"({int(class_correct[i])}/{class_total[i]})")
        else:
            logging.info(f"{classes[i]}: No samples.")
    from sklearn.metrics import classification_report, confusion_matrix
    cm = confusion_matrix(tgts, preds, labels=list(range(len(classes))))
    report = classification_report(tgts, preds, target_names=classes, labels=list(range(len(classes))))
    logging.info("\nConfusion Matrix:")
    logging.info(f"{cm}")
    logging.info("\nDetailed Classification Report:")
    logging.info(report)
    return accuracy, cm


def get_dataloaders(args, rank: int = 0, world: int = 1):
    """Creates data loaders for training and validation (:463-511).  With
    world > 1 each rank reads a disjoint shard (DistributedSampler) of
    ``--batch-size`` files per step."""
    stored = getattr(args, 'device_ingest', False)
    dataset_cls = StoredSampleDataset if stored else SpectrogramDataset
    collate = stored_collate_fn if stored else custom_collate_fn
    train_dataset = dataset_cls(args.data_dir, 'train', transform='train', class_names=[args.Class0, args.Class1])
    val_dataset = dataset_cls(args.data_dir, 'test', transform='val', class_names=[args.Class0, args.Class1])
    if stored and getattr(args, 'wave_augment', None):  # the train split only
        train_dataset.wave_kinds = tuple(args.wave_augment)
    if stored and getattr(args, 'wave_stretch', None):  # the train split only
        train_dataset.stretch_kinds = tuple(args.wave_stretch)
    per_rank = args.batch_size if world > 1 else (args.batch_size * args.num_gpus if args.num_gpus > 0
                                                   else args.batch_size)
    logging.info(f"Total batch size: {per_rank * world}")
    tsamp = vsamp = None
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler
        tsamp = DistributedSampler(train_dataset, num_replicas=world, rank=rank, shuffle=True, seed=args.seed)
        vsamp = DistributedSampler(val_dataset, num_replicas=world, rank=rank, shuffle=False)
    # --device-ingest: the workers come from a fork server and live across epochs.
    # Children forked from the process that holds the GPU slow its uploads from
    # pinned memory many times over for as long as they live, and a
    # worker that only reads a few hundred KiB per file is not worth a start per
    # epoch.  The host path keeps the DataLoader defaults it always had.
    extra = dict(multiprocessing_context='forkserver', persistent_workers=True) if stored and args.workers > 0 else {}
    train_loader = DataLoader(train_dataset, batch_size=per_rank, num_workers=args.workers, pin_memory=True,
                              shuffle=tsamp is None, sampler=tsamp, drop_last=False, collate_fn=collate, **extra)
    val_loader = DataLoader(val_dataset, batch_size=per_rank, num_workers=args.workers, pin_memory=True,
                            shuffle=False, sampler=vsamp, drop_last=False, collate_fn=collate, **extra)
    return train_loader, val_loader


def initialize_weights(model):
    """(:514-520) kept for API parity; the reference never calls it."""
    import torch.nn as nn
    import torch.nn.init as init
    for module in model.modules():
        if isinstance(module, (nn.Conv2d, nn.Linear)):
            init.kaiming_normal_(module.weight)
            if module.bias is not None:
                init.constant_(module.bias, 0)


def get_model(model):
    """(:523-528): the underlying model object."""
    return getattr(model, 'module', model)


def save_checkpoint(path, epoch, trainer, scheduler, best_acc, total_steps):
    """model_best.pth in the reference's format (:704-714)."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    torch.save({
        'epoch': epoch,
        'state_dict': trainer.net.state_dict(),
        'best_acc': best_acc,
        'optimizer': trainer.optimizer_state_dict(),
        'scheduler': scheduler.state_dict(),
        'total_steps': total_steps,
    }, path)


def main(argv=None):
    args = parse_args(argv)
    setup_logging()
    logging.info(f"Arguments: {args}")
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world == 1 and args.num_gpus > torch.cuda.device_count():
        logging.error(f"Requested number of GPUs ({args.num_gpus}) is greater than available GPUs "
                      f"({torch.cuda.device_count()})")
        sys.exit(1)
    if not torch.cuda.is_available():
        raise RuntimeError('submodel_trainer runs on MI355X GPUs only (no CPU path)')
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    group = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group('nccl', device_id=device)
        group = dist.group.WORLD
    logging.info(f"Using device: {device}; ranks: {world}")

    torch.manual_seed(args.seed)
    torch.cuda.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)

    from sad import train as st
    logging.info("Creating model with RANDOM weights...")
    base_sd, head_sd = st.init_state_dict(args.seed, args.model_name)
    trunk_sd = None
    if getattr(args, 'trunk', ''):
        logging.info(f"Loading the frozen trunk (conv1, bn1, layer1-3) from '{args.trunk}'")
        trunk_sd = torch.load(args.trunk, map_location='cpu', weights_only=True)['state_dict']
    trainer = st.Trainer(base_sd, head_sd, device, args.precision, lr=args.lr, group=group, world=world,
                         model_name=args.model_name, head_loss=getattr(args, 'head_loss', False), seed=args.seed,
                         trunk_sd=trunk_sd)
    # the frozen trunk is the inference plan's: it reads fp32 images
    frontend = st.TrainFrontEnd(device, 'fp32' if trunk_sd is not None else args.precision)
    model = DeviceModel(trainer, frontend, rank, world, group)

    train_loader, val_loader = get_dataloaders(args, rank, world)
    logging.info(f"Number of training samples: {len(train_loader.dataset)}")
    logging.info(f"Number of validation samples: {len(val_loader.dataset)}")
    optimizer = trainer.optimizer
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.5, patience=2)
    writer = _summary_writer(f'runs/experiment_{datetime.now().strftime("%Y%m%d-%H%M%S")}')

    best_acc = 0.0
    total_steps = 0
    start_epoch = 0
    if args.resume:
        if os.path.isfile(args.resume):
            logging.info(f"Loading checkpoint '{args.resume}'")
            checkpoint = torch.load(args.resume, map_location='cpu', weights_only=True)
            trainer.load_state_dict(checkpoint['state_dict'])
            trainer.load_optimizer_state_dict(checkpoint['optimizer'])
            scheduler.load_state_dict(checkpoint['scheduler'])
            start_epoch = checkpoint['epoch'] + 1
            best_acc = checkpoint['best_acc']
            total_steps = checkpoint.get('total_steps', 0)
            logging.info(f"Loaded checkpoint '{args.resume}' (epoch {checkpoint['epoch']})")
        else:
            logging.error(f"No checkpoint found at '{args.resume}'")

    for epoch in range(start_epoch, args.epochs):
        logging.info(f'\nEpoch: {epoch}/{args.epochs - 1}')
        if epoch == args.epochs // 3:
            logging.info("Unfreezing more layers...")
            if trainer.unfreeze_layer3() is False:
                logging.info("Skipped: layer3 belongs to the frozen trunk (--trunk)")
        if world > 1 and hasattr(train_loader.sampler, 'set_epoch'):
            train_loader.sampler.set_epoch(epoch)
        train_loss, train_acc, total_steps = train(args, train_loader, model, None, optimizer, scheduler, epoch,
                                                   writer, total_steps, device)
        val_loss, val_acc, _, _ = validate(args, val_loader, model, None, epoch, device)
        logging.info(f'epoch {epoch}: train loss {train_loss:.4f} acc {train_acc:.2f}% | '
                     f'val loss {val_loss:.4f} acc {val_acc:.2f}%')
        is_best = val_acc > best_acc
        best_acc = max(val_acc, best_acc)
        if is_best and rank == 0:
            save_checkpoint(os.path.join(args.checkpoint_dir, 'model_best.pth'), epoch, trainer, scheduler,
                            best_acc, total_steps)
            logging.info(f'Saved best model with accuracy: {val_acc:.2f}%')
        writer.add_scalar('Loss/train_epoch', train_loss, epoch)
        writer.add_scalar('Accuracy/train_epoch', train_acc, epoch)
        writer.add_scalar('Loss/val_epoch', val_loss, epoch)
        writer.add_scalar('Accuracy/val_epoch', val_acc, epoch)
    writer.close()
    logging.info('Training completed.')
    logging.info(f'Best validation accuracy: {best_acc:.2f}%')
    if args.evaluate:
        evaluate(args, model, val_loader, None, device)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return best_acc


if __name__ == '__main__':
    main()
