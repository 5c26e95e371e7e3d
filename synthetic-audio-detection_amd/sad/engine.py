"""Device engine: front end, backbone(s) and heads as libsad plans.

This is the MI355X replacement of the reference's device work:
  * ``FrontEnd``  -- torchaudio MelSpectrogram/AmplitudeToDB + standardise
    (inference_runner.py:157-171; trainer norm=None variant
    submodel_trainer.py:97-105,191-199)
  * ``Backbone``  -- timm resnet18 forward_features + AdaptiveAvgPool2d
    (inference_runner.py:35,37,49-51), with Resize((512,512)) + repeat(3)
    (:172-174) fused into the stem
  * ``ResNetBackbone`` -- the deeper timm names (resnet34/50/101/152,
    SURVEY.md 8(f) row 4) on the same kernels (libsad sad_resnet_*)
  * ``Heads``     -- BinaryClassifier.head x N + ModularMultiHeadClassifier
    merge (inference_runner.py:36-48,62-73)
  * ``Engine``    -- a merged checkpoint's state dict -> the three above.
    Sub-models whose ``base.*`` tensors are identical (the reference's quirk
    C2 makes that the normal case) share ONE backbone run.  ResNet-18
    sub-models that differ in ``layer4`` alone (trained on one frozen trunk,
    merged with ``--keep-backbone``) run the trunk once and one layer4 tail
    each (``Engine.features``); the deeper plans run one full backbone per
    distinct sub-model.

Every call is asynchronous on torch's current stream of the engine's device.
"""
from __future__ import annotations

import hashlib
from typing import Dict, List, Sequence

import numpy as np
import torch

from . import _lib
from .weights import arch_of_state, arch_param_shapes, arch_spec, backbone_param_shapes

MAP_H, MAP_W = 128, 251
N_SAMPLES = 128000
HEAD_KEYS = ['2.weight', '2.bias', '3.weight', '3.bias', '3.running_mean', '3.running_var',
             '6.weight', '6.bias', '7.weight', '7.bias', '7.running_mean', '7.running_var',
             '10.weight', '10.bias']


def _dev(device) -> torch.device:
    d = torch.device(device)
    if d.type != 'cuda':
        raise RuntimeError(f'libsad runs on MI355X devices only (got {d}); there is no CPU path')
    return torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())


def _np32(t) -> np.ndarray:
    return np.ascontiguousarray(torch.as_tensor(t).detach().to('cpu', torch.float32).numpy())


def _checked(sd: Dict[str, torch.Tensor], key: str, shape) -> np.ndarray:
    """sd[key] as contiguous fp32, after checking its shape: the C plan builders
    read raw host pointers with the layout's sizes, so a wrong width (e.g. a
    wide_resnet state dict) must fail here, not overrun host memory there."""
    if key not in sd:
        raise KeyError(f'missing tensor {key!r}')
    a = _np32(sd[key])
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f'tensor {key!r} has shape {tuple(a.shape)}, expected {tuple(shape)}')
    return a


def _backbone_arrays(base_sd, shapes) -> list:
    arrays = []
    for key, shape, kind in shapes:
        if kind == 'conv':
            arrays.append(_checked(base_sd, f'{key}.weight', shape))
        else:
            for s in ('weight', 'bias', 'running_mean', 'running_var'):
                arrays.append(_checked(base_sd, f'{key}.{s}', shape))
    return arrays


def _head_arrays(sd, num_features: int) -> list:
    from .weights import head_layout
    shapes = {}
    for idx, kind, shape in head_layout(num_features):
        if kind == 'linear':
            shapes[f'{idx}.weight'], shapes[f'{idx}.bias'] = shape, shape[:1]
        else:
            for s in ('weight', 'bias', 'running_mean', 'running_var'):
                shapes[f'{idx}.{s}'] = shape
    return [_checked(sd, k, shapes[k]) for k in HEAD_KEYS]


class FrontEnd:
    def __init__(self, device='cuda', norm: str | None = 'slaney', n_samples: int = N_SAMPLES,
                 sample_rate: int = 32000, n_fft: int = 2048, hop: int = 512, n_mels: int = 128,
                 f_min: float = 20.0, f_max: float = 12000.0, top_db: float | None = 80.0):
        self.device = _dev(device)
        cfg = _lib.FrontendCfg(sample_rate, n_fft, hop, n_mels, f_min, f_max, 1 if norm == 'slaney' else 0,
                               -1.0 if top_db is None else float(top_db), n_samples)
        self._plan = _lib.P()
        # torchaudio's own fp32 filterbank (sad.audio.melscale_fbanks), not the
        # library's float64 rounding of the same triangles
        from .audio import melscale_fbanks
        fb = melscale_fbanks(n_fft // 2 + 1, float(f_min), float(f_max), n_mels, sample_rate,
                             norm == 'slaney').contiguous()
        # the plan reads a host fp32 [n_freqs, n_mels] array through this pointer
        assert fb.dtype == torch.float32 and fb.device.type == 'cpu' and fb.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.call('sad_frontend_plan_create_fb', _lib.ctypes.byref(cfg), fb.data_ptr(),
                      _lib.ctypes.byref(self._plan))
        nf = _lib.I32()
        _lib.call('sad_frontend_frames', self._plan, _lib.ctypes.byref(nf))
        self.n_frames, self.n_mels, self.n_samples = nf.value, n_mels, n_samples
        self.fbank, self.sample_rate = fb, sample_rate  # the plan's filterbank (sad.evidence.row_hz reads it)

    def __call__(self, pcm: torch.Tensor, want_db: bool = False, out: torch.Tensor | None = None):
        """pcm [n, >=n_samples] int16 (or fp32 waveform in [-1,1)) on device ->
        map [n, n_mels, frames] fp32 (and the clamped dB map if want_db)."""
        assert pcm.dtype in (torch.int16, torch.float32) and pcm.device == self.device and pcm.dim() == 2
        assert pcm.stride(1) == 1 and pcm.shape[1] >= self.n_samples
        n = pcm.shape[0]
        if out is None:
            out = torch.empty(n, self.n_mels, self.n_frames, device=self.device, dtype=torch.float32)
        db = torch.empty_like(out) if want_db else None
        fn = 'sad_frontend_run' if pcm.dtype == torch.int16 else 'sad_frontend_run_f32'
        with torch.cuda.device(self.device):
            _lib.call(fn, self._plan, _lib.ptr(pcm), n, pcm.stride(0), _lib.ptr(db), _lib.ptr(out),
                      _lib.stream_handle(self.device))
        return (out, db) if want_db else out

    def windows(self, wf: torch.Tensor, offsets: torch.Tensor, want_db: bool = False,
                out: torch.Tensor | None = None):
        """Windows of one long fp32 waveform wf [T] on the device, segment i at
        sample offsets[i] (int64 device tensor), read in place
        (sad_frontend_run_windows) -> map [n, n_mels, frames]."""
        assert wf.dtype == torch.float32 and wf.dim() == 1 and wf.is_contiguous() and wf.device == self.device
        assert offsets.dtype == torch.int64 and offsets.dim() == 1 and offsets.is_contiguous()
        assert offsets.device == self.device and wf.shape[0] >= self.n_samples
        n = offsets.shape[0]
        if out is None:
            out = torch.empty(n, self.n_mels, self.n_frames, device=self.device, dtype=torch.float32)
        db = torch.empty_like(out) if want_db else None
        with torch.cuda.device(self.device):
            _lib.call('sad_frontend_run_windows', self._plan, _lib.ptr(wf), wf.shape[0], _lib.ptr(offsets), n,
                      _lib.ptr(db), _lib.ptr(out), _lib.stream_handle(self.device))
        return (out, db) if want_db else out

    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                _lib.load().sad_frontend_plan_destroy(self._plan)
        except Exception:
            pass


def _dtype_code(dtype: str) -> int:
    if dtype not in _lib.DTYPES:
        raise ValueError(f'dtype must be one of {sorted(_lib.DTYPES)} (got {dtype!r})')
    return _lib.DTYPES[dtype]


def _tensor_dtype(dtype: str) -> torch.dtype:
    """torch dtype of a plan's activations (bf16x3: bf16 pairs in the split layout)."""
    return {'fp32': torch.float32, 'fp16': torch.float16}.get(dtype, torch.bfloat16)


def _code_of(t: torch.Tensor) -> int:
    """libsad dtype of an operator wrapper's tensors: fp32, bf16 or fp16."""
    codes = {torch.float32: _lib.SAD_F32, torch.bfloat16: _lib.SAD_BF16, torch.float16: _lib.SAD_F16}
    if t.dtype not in codes:
        raise ValueError(f'tensors must be float32, bfloat16 or float16 (got {t.dtype})')
    return codes[t.dtype]


def to_split(x: torch.Tensor) -> torch.Tensor:
    """fp32 [..., C] -> the split-bf16 layout [..., 2C] bf16 of dtype 'bf16x3':
    per group of 32 channels [hi(32) | lo(32)], hi = bf16(x), lo = bf16(x - hi)."""
    C = x.shape[-1]
    assert C % 32 == 0
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    g = torch.stack([hi.reshape(*x.shape[:-1], C // 32, 32), lo.reshape(*x.shape[:-1], C // 32, 32)], dim=-2)
    return g.reshape(*x.shape[:-1], 2 * C).contiguous()


def from_split(t: torch.Tensor) -> torch.Tensor:
    """The split-bf16 layout [..., 2C] bf16 -> fp32 [..., C] (hi + lo)."""
    C2 = t.shape[-1]
    g = t.reshape(*t.shape[:-1], C2 // 64, 2, 32).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(*t.shape[:-1], C2 // 2)


def _act_channels(dtype: str, c: int) -> int:
    return 2 * c if dtype == 'bf16x3' else c


def resize(map_: torch.Tensor, size=(512, 512), dtype: str = 'fp32') -> torch.Tensor:
    """Device bilinear resize (torchvision Resize semantics) of [n, h, w] fp32."""
    n, h, w = map_.shape
    dt = _lib.SAD_BF16 if dtype == 'bf16' else _lib.SAD_F32  # resize output: fp32 or bf16 image
    out = torch.empty(n, size[0], size[1], device=map_.device,
                      dtype=torch.bfloat16 if dt == _lib.SAD_BF16 else torch.float32)
    with torch.cuda.device(map_.device):
        _lib.call('sad_resize_run', _lib.ptr(map_.contiguous()), n, h, w, size[0], size[1], dt, _lib.ptr(out),
                  _lib.stream_handle(map_.device))
    return out


class Backbone:
    """One ResNet-18 backbone; ``base_sd`` uses timm keys (conv1.weight, ...)."""

    def __init__(self, base_sd: Dict[str, torch.Tensor], device='cuda', dtype: str = 'bf16',
                 micro_batch: int = 64):
        self.device = _dev(device)
        self.dtype = dtype
        self._dt = _dtype_code(dtype)
        self.tdtype = _tensor_dtype(dtype)
        self.micro_batch = micro_batch
        arrays = _backbone_arrays(base_sd, backbone_param_shapes())
        self._plan = _lib.P()
        with torch.cuda.device(self.device):
            # the plan copies (hipMemcpy, synchronous) what it needs; the host arrays die here
            _lib.call('sad_backbone_plan_create', _lib.pointer_array(arrays), len(arrays), self._dt, MAP_H, MAP_W,
                      _lib.ctypes.byref(self._plan))
        self._ws = None

    def workspace(self, mb: int) -> torch.Tensor:
        sz = _lib.SZ()
        _lib.call('sad_backbone_workspace_size', self._plan, mb, _lib.ctypes.byref(sz))
        if self._ws is None or self._ws.numel() < sz.value:
            self._ws = torch.empty(sz.value, dtype=torch.uint8, device=self.device)
        return self._ws

    def __call__(self, maps: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        assert maps.dtype == torch.float32 and maps.shape[1:] == (MAP_H, MAP_W) and maps.is_contiguous()
        B = maps.shape[0]
        feats = out if out is not None else torch.empty(B, 512, device=self.device, dtype=torch.float32)
        mb = max(1, min(self.micro_batch, B))
        ws = self.workspace(mb)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_run', self._plan, _lib.ptr(maps), B, mb, _lib.ptr(feats), _lib.ptr(ws),
                      ws.numel(), _lib.stream_handle(self.device))
        return feats

    def forward_images(self, img: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """img [B,512,512] fp32 (one channel of the reference's identical three) -> feats."""
        assert img.dtype == torch.float32 and img.shape[1:] == (512, 512) and img.is_contiguous()
        B = img.shape[0]
        feats = out if out is not None else torch.empty(B, 512, device=self.device, dtype=torch.float32)
        mb = max(1, min(self.micro_batch, B))
        ws = self.workspace(mb)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_run_img', self._plan, _lib.ptr(img), B, mb, _lib.ptr(feats), _lib.ptr(ws),
                      ws.numel(), _lib.stream_handle(self.device))
        return feats

    def forward_images3(self, img3: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """img3 [B,3,512,512] fp32 with possibly distinct channels -> feats [B,512]."""
        assert img3.dtype == torch.float32 and img3.shape[1:] == (3, 512, 512) and img3.is_contiguous()
        B = img3.shape[0]
        feats = out if out is not None else torch.empty(B, 512, device=self.device, dtype=torch.float32)
        mb = max(1, min(self.micro_batch, B))
        ws = self.workspace(mb)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_run_img3', self._plan, _lib.ptr(img3), B, mb, _lib.ptr(feats), _lib.ptr(ws),
                      ws.numel(), _lib.stream_handle(self.device))
        return feats

    def _input(self, x: torch.Tensor, kind: str):
        """(map pointer, img pointer) of the trunk entries for x of `kind`."""
        if kind not in ('maps', 'img'):
            raise ValueError(f"kind must be 'maps' or 'img' (got {kind!r})")
        shape = (MAP_H, MAP_W) if kind == 'maps' else (512, 512)
        assert x.dtype == torch.float32 and x.shape[1:] == shape and x.is_contiguous() and x.device == self.device
        return (_lib.ptr(x), None) if kind == 'maps' else (None, _lib.ptr(x))

    def trunk(self, x: torch.Tensor, kind: str = 'maps') -> torch.Tensor:
        """Stem, layer1, layer2 and layer3 on maps [B,128,251] or images
        [B,512,512] -> layer3's output NHWC [B,32,32,256] in the plan's
        activation layout (fp16: torch.float16; bf16x3: the split layout, 512
        bf16 per pixel)."""
        mp, ip = self._input(x, kind)
        B = x.shape[0]
        l3 = torch.empty(B, 32, 32, _act_channels(self.dtype, 256), device=self.device, dtype=self.tdtype)
        mb = max(1, min(self.micro_batch, B))
        ws = self.workspace(mb)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_trunk_run', self._plan, mp, ip, B, mb, _lib.ptr(l3), _lib.ptr(ws), ws.numel(),
                      _lib.stream_handle(self.device))
        return l3

    def tail(self, l3: torch.Tensor) -> torch.Tensor:
        """layer4 + average pool on ``trunk``'s output (left intact) -> feats [B,512]."""
        B = l3.shape[0]
        assert l3.shape == (B, 32, 32, _act_channels(self.dtype, 256)) and l3.dtype == self.tdtype
        assert l3.is_contiguous() and l3.device == self.device
        feats = torch.empty(B, 512, device=self.device, dtype=torch.float32)
        mb = max(1, min(self.micro_batch, B))
        ws = self.workspace(mb)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_tail_run', self._plan, _lib.ptr(l3), B, mb, _lib.ptr(feats), _lib.ptr(ws),
                      ws.numel(), _lib.stream_handle(self.device))
        return feats

    def shared(self, tails: Sequence['Backbone'], x: torch.Tensor, kind: str = 'maps') -> List[torch.Tensor]:
        """This backbone's trunk once per micro-batch chunk, then the tail of
        every backbone in `tails` on it (sad_backbone_shared_run) -> one feats
        [B,512] per tail.  The micro-batch is this backbone's."""
        mp, ip = self._input(x, kind)
        B = x.shape[0]
        feats = [torch.empty(B, 512, device=self.device, dtype=torch.float32) for _ in tails]
        mb = max(1, min(self.micro_batch, B))
        sz = _lib.SZ()
        _lib.call('sad_backbone_shared_workspace_size', self._plan, mb, _lib.ctypes.byref(sz))
        if self._ws is None or self._ws.numel() < sz.value:
            self._ws = torch.empty(sz.value, dtype=torch.uint8, device=self.device)
        plans = (_lib.ctypes.c_void_p * len(tails))(*[t._plan.value for t in tails])
        fp = (_lib.ctypes.c_void_p * len(tails))(*[f.data_ptr() for f in feats])
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_shared_run', self._plan, plans, len(tails), mp, ip, B, mb, fp,
                      _lib.ptr(self._ws), self._ws.numel(), _lib.stream_handle(self.device))
        return feats

    def stem(self, maps: torch.Tensor) -> torch.Tensor:
        """NHWC [B,128,128,64] in the plan dtype (bf16x3: fp32 decoded from the split layout)."""
        B = maps.shape[0]
        out = torch.empty(B, 128, 128, _act_channels(self.dtype, 64), device=self.device, dtype=self.tdtype)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_stem_run', self._plan, _lib.ptr(maps.contiguous()), B, _lib.ptr(out),
                      _lib.stream_handle(self.device))
        return from_split(out) if self.dtype == 'bf16x3' else out

    def debug(self, maps: torch.Tensor):
        """(pooled feats [B,512], layer4 map NHWC [B,16,16,512]) for small B."""
        B = maps.shape[0]
        feats = torch.empty(B, 512, device=self.device, dtype=torch.float32)
        l4 = torch.empty(B, 16, 16, _act_channels(self.dtype, 512), device=self.device, dtype=self.tdtype)
        ws = self.workspace(B)
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_run_debug', self._plan, _lib.ptr(maps.contiguous()), B, _lib.ptr(feats),
                      _lib.ptr(l4), _lib.ptr(ws), ws.numel(), _lib.stream_handle(self.device))
        return feats, (from_split(l4) if self.dtype == 'bf16x3' else l4)

    def keep(self, x: torch.Tensor, kind: str = 'maps'):
        """One chunk (B <= micro_batch) with the layer4 activation kept
        (sad_backbone_run_keep): (feats [B,512] fp32, l4 NHWC [B,16,16,512] in
        the plan's activation LAYOUT -- bf16x3: 1024 bf16 per pixel, not
        decoded).  The features are the pool of the stored activation."""
        mp, ip = self._input(x, kind)
        B = x.shape[0]
        if B > self.micro_batch:
            raise ValueError(f'keep takes one chunk of at most micro_batch = {self.micro_batch} windows (got {B})')
        feats = torch.empty(B, 512, device=self.device, dtype=torch.float32)
        l4 = torch.empty(B, 16, 16, _act_channels(self.dtype, 512), device=self.device, dtype=self.tdtype)
        ws = self.workspace(max(1, B))
        with torch.cuda.device(self.device):
            _lib.call('sad_backbone_run_keep', self._plan, mp, ip, B, _lib.ptr(feats), _lib.ptr(l4), _lib.ptr(ws),
                      ws.numel(), _lib.stream_handle(self.device))
        return feats, l4

    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                _lib.load().sad_backbone_plan_destroy(self._plan)
        except Exception:
            pass


class ResNetBackbone:
    """A timm resnet34/50/101/152 backbone (``base_sd`` in timm keys) on the
    generic libsad ResNet plan: map -> pooled [B, num_features] fp32."""

    def __init__(self, base_sd: Dict[str, torch.Tensor], model_name: str, device='cuda', dtype: str = 'bf16',
                 micro_batch: int = 64):
        self.device = _dev(device)
        self.dtype = dtype
        self.model_name = model_name
        block, layers, self.num_features = arch_spec(model_name)
        self._dt = _dtype_code(dtype)
        # operands past the kernels' 2 GiB buffer range run as several launches
        # over image ranges (launch_block_conv), so the micro-batch is free
        self.micro_batch = max(1, micro_batch)
        arrays = _backbone_arrays(base_sd, arch_param_shapes(model_name))
        lay = (_lib.I32 * 4)(*layers)
        self._plan = _lib.P()
        with torch.cuda.device(self.device):
            _lib.call('sad_resnet_plan_create', _lib.pointer_array(arrays), len(arrays),
                      1 if block == 'bottleneck' else 0, lay, self._dt, MAP_H, MAP_W, _lib.ctypes.byref(self._plan))
        self._ws = None

    def _run(self, fn: str, x: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        B = x.shape[0]
        feats = out if out is not None else torch.empty(B, self.num_features, device=self.device,
                                                        dtype=torch.float32)
        mb = max(1, min(self.micro_batch, B))
        sz = _lib.SZ()
        _lib.call('sad_resnet_workspace_size', self._plan, mb, _lib.ctypes.byref(sz))
        if self._ws is None or self._ws.numel() < sz.value:
            self._ws = torch.empty(sz.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.call(fn, self._plan, _lib.ptr(x), B, mb, _lib.ptr(feats), _lib.ptr(self._ws),
                      self._ws.numel(), _lib.stream_handle(self.device))
        return feats

    def __call__(self, maps: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        assert maps.dtype == torch.float32 and maps.shape[1:] == (MAP_H, MAP_W) and maps.is_contiguous()
        return self._run('sad_resnet_run', maps, out)

    def forward_images(self, img: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """img [B,512,512] fp32 (one channel of the reference's identical three) -> feats."""
        assert img.dtype == torch.float32 and img.shape[1:] == (512, 512) and img.is_contiguous()
        return self._run('sad_resnet_run_img', img, out)

    def forward_images3(self, img3: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """img3 [B,3,512,512] fp32 with possibly distinct channels -> feats."""
        assert img3.dtype == torch.float32 and img3.shape[1:] == (3, 512, 512) and img3.is_contiguous()
        return self._run('sad_resnet_run_img3', img3, out)

    def keep(self, x: torch.Tensor, kind: str = 'maps'):
        """One chunk (B <= micro_batch) with the last stage's activation kept
        (sad_resnet_run_keep): (feats [B,num_features] fp32, l4 NHWC
        [B,16,16,num_features] in the plan's activation layout, bf16x3 not
        decoded)."""
        if kind not in ('maps', 'img'):
            raise ValueError(f"kind must be 'maps' or 'img' (got {kind!r})")
        shape = (MAP_H, MAP_W) if kind == 'maps' else (512, 512)
        assert x.dtype == torch.float32 and x.shape[1:] == shape and x.is_contiguous() and x.device == self.device
        B = x.shape[0]
        if B > self.micro_batch:
            raise ValueError(f'keep takes one chunk of at most micro_batch = {self.micro_batch} windows (got {B})')
        nf = self.num_features
        feats = torch.empty(B, nf, device=self.device, dtype=torch.float32)
        l4 = torch.empty(B, 16, 16, _act_channels(self.dtype, nf), device=self.device,
                         dtype=_tensor_dtype(self.dtype))
        sz = _lib.SZ()
        _lib.call('sad_resnet_workspace_size', self._plan, max(1, B), _lib.ctypes.byref(sz))
        if self._ws is None or self._ws.numel() < sz.value:
            self._ws = torch.empty(sz.value, dtype=torch.uint8, device=self.device)
        mp, ip = (_lib.ptr(x), None) if kind == 'maps' else (None, _lib.ptr(x))
        with torch.cuda.device(self.device):
            _lib.call('sad_resnet_run_keep', self._plan, mp, ip, B, _lib.ptr(feats), _lib.ptr(l4),
                      _lib.ptr(self._ws), self._ws.numel(), _lib.stream_handle(self.device))
        return feats, l4

    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                _lib.load().sad_resnet_plan_destroy(self._plan)
        except Exception:
            pass


class Heads:
    """N BinaryClassifier heads (+ merge); ``head_sds[h]`` uses nn.Sequential
    index keys (2.weight, 3.running_mean, ...)."""

    def __init__(self, head_sds: Sequence[Dict[str, torch.Tensor]], feat_index: Sequence[int], n_feat: int,
                 device='cuda', feat_dim: int = 512):
        self.device = _dev(device)
        self.n_heads = len(head_sds)
        arrays = [a for sd in head_sds for a in _head_arrays(sd, feat_dim)]
        fi = (_lib.I32 * self.n_heads)(*feat_index)
        self._plan = _lib.P()
        with torch.cuda.device(self.device):
            _lib.call('sad_heads_plan_create_dim', _lib.pointer_array(arrays), self.n_heads, fi, n_feat,
                      feat_dim, _lib.ctypes.byref(self._plan))
        self.n_feat = n_feat
        self.feat_dim = feat_dim
        self._used = sorted(set(int(f) for f in feat_index))
        self._ws = None

    def _check_feats(self, feats) -> int:
        """The C entry reads raw pointers as [B, feat_dim] fp32 rows on the
        plan's device, so anything else must fail here.  An entry of a feature
        group no head reads may be None."""
        if len(feats) != self.n_feat:
            raise ValueError(f'expected {self.n_feat} feature tensors, got {len(feats)}')
        B = None
        for i, f in enumerate(feats):
            if f is None:
                if i in self._used:
                    raise ValueError(f'features {i} are read by a head and must not be None')
                continue
            if f.dtype != torch.float32:
                raise ValueError(f'features {i} must be float32 (got {f.dtype})')
            if f.device != self.device:
                raise ValueError(f'features {i} are on {f.device}, the plan is on {self.device}')
            if f.dim() != 2 or f.shape[1] != self.feat_dim:
                raise ValueError(f'features {i} must be [B, {self.feat_dim}] (got {tuple(f.shape)})')
            if not f.is_contiguous():
                raise ValueError(f'features {i} must be contiguous')
            if B is not None and f.shape[0] != B:
                raise ValueError(f'features {i} have {f.shape[0]} rows, the others {B}')
            B = f.shape[0]
        return B

    def __call__(self, feats: Sequence[torch.Tensor], logits: torch.Tensor | None = None,
                 merged: torch.Tensor | None = None):
        B = self._check_feats(feats)
        if logits is None:
            logits = torch.empty(B, self.n_heads, 2, device=self.device, dtype=torch.float32)
        if merged is None:
            merged = torch.empty(B, self.n_heads + 1, device=self.device, dtype=torch.float32)
        sz = _lib.SZ()
        _lib.call('sad_heads_workspace_size', self._plan, B, _lib.ctypes.byref(sz))
        if self._ws is None or self._ws.numel() < sz.value:
            self._ws = torch.empty(sz.value, dtype=torch.uint8, device=self.device)
        fp = (_lib.ctypes.c_void_p * self.n_feat)(*[_lib.ptr(f) for f in feats])
        with torch.cuda.device(self.device):
            _lib.call('sad_heads_merge_run', self._plan, fp, B, _lib.ptr(logits), _lib.ptr(merged),
                      _lib.ptr(self._ws), self._ws.numel(), _lib.stream_handle(self.device))
        self._ws_rows = B
        return logits, merged

    def grad(self, B: int, cls: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """d logit[cls] / d features of every head for the B rows of the LAST
        ``__call__`` (sad_heads_grad_run reads the ReLU masks from its
        workspace): [n_heads, B, feat_dim] fp32.  cls: 0 Real, 1 Synthetic."""
        if self._ws is None or getattr(self, '_ws_rows', None) != B:
            raise RuntimeError(f'grad({B}) must follow a forward of the same {B} rows (the masks live in its workspace)')
        if cls not in (0, 1):
            raise ValueError(f'cls must be 0 (Real) or 1 (Synthetic), got {cls!r}')
        g = out if out is not None else torch.empty(self.n_heads, B, self.feat_dim, device=self.device,
                                                    dtype=torch.float32)
        assert g.shape == (self.n_heads, B, self.feat_dim) and g.dtype == torch.float32 and g.is_contiguous()
        with torch.cuda.device(self.device):
            _lib.call('sad_heads_grad_run', self._plan, _lib.ptr(self._ws), B, cls, _lib.ptr(g),
                      _lib.stream_handle(self.device))
        return g

    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                _lib.load().sad_heads_plan_destroy(self._plan)
        except Exception:
            pass


EXPLAIN_TARGETS = ('synthetic', 'real', 'margin')


def evidence(l4: torch.Tensor, dtype: str, g: Sequence[torch.Tensor], out: torch.Tensor | None = None) -> torch.Tensor:
    """sad_evidence_run: l4 NHWC [B, H, W, C'] in the activation layout of
    `dtype` (C' = 2C for 'bf16x3'), g = 1..16 tensors [B, C] fp32 (one per map)
    -> out [B, len(g), H*W] fp32, out[b, m, p] = sum_c g[m][b, c] A[b, p, c] / (H W)."""
    B, hw = l4.shape[0], l4.shape[1] * l4.shape[2]
    C = l4.shape[3] // (2 if dtype == 'bf16x3' else 1)
    if l4.dtype != _tensor_dtype(dtype) or not l4.is_contiguous():
        raise ValueError(f'l4 must be contiguous {_tensor_dtype(dtype)} for dtype {dtype!r}')
    for t in g:
        if t.dtype != torch.float32 or tuple(t.shape) != (B, C) or not t.is_contiguous() or t.device != l4.device:
            raise ValueError(f'every g must be a contiguous fp32 [{B}, {C}] tensor on {l4.device}')
    if out is None:
        out = torch.empty(B, len(g), hw, device=l4.device, dtype=torch.float32)
    gp = (_lib.ctypes.c_void_p * len(g))(*[t.data_ptr() for t in g])
    with torch.cuda.device(l4.device):
        _lib.call('sad_evidence_run', _lib.ptr(l4), _dtype_code(dtype), B, hw, C, gp, len(g), _lib.ptr(out),
                  _lib.stream_handle(l4.device))
    return out


def _arch(base_sd) -> str:
    """Architecture name of a backbone state dict.  A BasicBlock key set that
    matches no depth is treated as resnet18 so that the missing-key check names
    what is absent; a Bottleneck key set (conv3 keys) that matches no depth
    raises -- read as resnet18 its 1x1 convs would be taken for 3x3."""
    if not base_sd:
        return 'resnet18'
    try:
        return arch_of_state(base_sd)
    except ValueError:
        if any('.conv3.' in k for k in base_sd):
            raise
        return 'resnet18'


def _digest(tensors: List[torch.Tensor]) -> str:
    h = hashlib.sha1()
    for t in tensors:
        h.update(_np32(t).tobytes())
    return h.hexdigest()


TAIL_PREFIX = 'layer4.'  # the part reference training changes; everything else is the trunk


class Grouping:
    """How an ensemble's sub-models share backbone work (``group_backbones``).

    feat_index[h]    distinct backbone of sub-model h (order of first appearance)
    first[j]         the first sub-model that uses distinct backbone j
    trunk_of[j]      distinct trunk (stem, layer1-3) of backbone j, by first appearance
    shared           lists of backbone indices: two or more distinct tails
                     (layer4) on one trunk, which run the trunk once
    """

    def __init__(self, feat_index, first, trunk_of, shared):
        self.feat_index, self.first, self.trunk_of, self.shared = feat_index, first, trunk_of, shared
        self.n_backbones = len(first)
        self.n_trunks = len(set(trunk_of))

    def describe(self) -> str:
        n = len(self.feat_index)
        return f'{n} sub-model{"s" if n != 1 else ""}: {self.n_trunks} trunk{"s" if self.n_trunks != 1 else ""}, ' \
               f'{self.n_backbones} tail{"s" if self.n_backbones != 1 else ""}'


def group_backbones(base_sds: Sequence[Dict[str, torch.Tensor]]) -> Grouping:
    """Group sub-model backbones (timm keys) by content, on the host.  Trunk
    tensors (everything outside ``layer4.``) and tail tensors (``layer4.*``)
    are hashed separately; ``num_batches_tracked`` counts for neither.  Two
    sub-models are one backbone when both hashes agree; distinct backbones with
    one trunk hash form a shared group."""
    pairs, trunks, feat_index, first, trunk_of = {}, {}, [], [], []
    for h, sd in enumerate(base_sds):
        keys = [k for k in sorted(sd) if not k.endswith('num_batches_tracked')]
        trunk = _digest([sd[k] for k in keys if not k.startswith(TAIL_PREFIX)])
        tail = _digest([sd[k] for k in keys if k.startswith(TAIL_PREFIX)])
        if (trunk, tail) not in pairs:
            pairs[(trunk, tail)] = len(first)
            first.append(h)
            trunk_of.append(trunks.setdefault(trunk, len(trunks)))
        feat_index.append(pairs[(trunk, tail)])
    shared = [[j for j, t in enumerate(trunk_of) if t == tr] for tr in range(len(trunks))]
    return Grouping(feat_index, first, trunk_of, [g for g in shared if len(g) >= 2])


def split_merged_state(sd: Dict[str, torch.Tensor]):
    """merged state dict -> (sorted sub-model indices, {i: base_sd}, {i: head_sd}).
    Index parsing follows inference_runner.py:88-98 (sorted ints after
    ``sub_models.``)."""
    idx = set()
    for k in sd.keys():
        parts = k.split('.')
        if len(parts) >= 3 and parts[0] == 'sub_models':
            try:
                idx.add(int(parts[1]))
            except ValueError:
                pass
    idx = sorted(idx)
    bases, heads = {}, {}
    for i in idx:
        pre = f'sub_models.{i}.'
        bases[i] = {k[len(pre) + 5:]: v for k, v in sd.items() if k.startswith(pre + 'base.')}
        heads[i] = {k[len(pre) + 5:]: v for k, v in sd.items() if k.startswith(pre + 'head.')}
    return idx, bases, heads


class Engine:
    """Merged checkpoint -> device pipeline  pcm -> (per-head logits, merged)."""

    def __init__(self, merged_sd: Dict[str, torch.Tensor], device='cuda', dtype: str = 'bf16',
                 micro_batch: int = 64, norm: str | None = 'slaney'):
        self.device = _dev(device)
        self.dtype = dtype
        idx, bases, heads = split_merged_state(merged_sd)
        if not idx:
            raise ValueError('state dict has no sub_models.<i>.* keys')
        self.indices = idx
        self.backbones = []
        archs = {_arch(bases[i]) for i in idx}
        if len(archs) != 1:
            raise ValueError(f'sub-models mix backbone architectures {sorted(archs)}')
        self.arch = archs.pop()
        for i in idx:
            keys = [k for k, _, kind in arch_param_shapes(self.arch)]
            missing = [k for k in keys if not any(s.startswith(k + '.') for s in bases[i])]
            if missing:
                raise KeyError(f'sub-model {i} lacks backbone tensors {missing[:3]}...')
        # one plan per distinct full backbone (trunk + tail), each usable alone
        self.grouping = group_backbones([bases[i] for i in idx])
        for h in self.grouping.first:
            if self.arch == 'resnet18':  # the tuned ResNet-18 plan
                self.backbones.append(Backbone(bases[idx[h]], self.device, dtype, micro_batch))
            else:
                self.backbones.append(ResNetBackbone(bases[idx[h]], self.arch, self.device, dtype, micro_batch))
        # distinct tails on one trunk run the trunk once (the tuned ResNet-18
        # plan only: the deeper plans run one full backbone per distinct sub-model)
        self.shared_groups = self.grouping.shared if self.arch == 'resnet18' else []
        self.num_features = arch_spec(self.arch)[2]
        self.heads = Heads([heads[i] for i in idx], self.grouping.feat_index, len(self.backbones), self.device,
                           feat_dim=self.num_features)
        self.frontend = FrontEnd(self.device, norm=norm)
        self.n_heads = len(idx)

    def features(self, x: torch.Tensor, kind: str = 'maps') -> List[torch.Tensor]:
        """Pooled features of every distinct backbone, aligned with
        ``self.backbones``: x is maps [B,128,251] (kind='maps') or one-channel
        images [B,512,512] (kind='img').  Backbones of a shared group run their
        trunk once per micro-batch chunk (the micro-batch of the group's first
        backbone); the values equal ``bb(x)`` / ``bb.forward_images(x)`` bit
        for bit."""
        if kind not in ('maps', 'img'):
            raise ValueError(f"kind must be 'maps' or 'img' (got {kind!r})")
        feats: List[torch.Tensor | None] = [None] * len(self.backbones)
        for group in self.shared_groups:
            bbs = [self.backbones[j] for j in group]
            for j, f in zip(group, bbs[0].shared(bbs, x, kind)):
                feats[j] = f
        for j, bb in enumerate(self.backbones):
            if feats[j] is None:
                feats[j] = bb(x) if kind == 'maps' else bb.forward_images(x)
        return feats

    def forward_maps(self, maps: torch.Tensor):
        return self.heads(self.features(maps))

    def explain(self, x: torch.Tensor, kind: str = 'maps', target: str = 'synthetic', details: list | None = None):
        """Evidence maps (include/sad.h "evidence"): (merged [B, N+1], evidence
        [B, N, 16, 16] fp32), evidence[b, h] = Grad-CAM of head h's target logit
        on its backbone's layer4 activation: signed, unnormalised, rows = mel
        axis (row 0 the lowest bands), columns = time.  target: 'synthetic',
        'real', or 'margin' (synthetic minus real; the two share their masks).

        Runs per micro-batch chunk: keep (every distinct backbone in full, a
        shared trunk included), the heads on the chunk, their gradient, one
        evidence pass per backbone -- a row of the heads does not depend on its
        position in the batch, so the chunks are the whole batch's rows.  Only
        one chunk's activations are alive at a time.  merged comes from the
        keep path (features pooled from the stored activation), which can
        differ from ``forward_maps`` by the activation rounding.
        details (tests): a list that receives per chunk (rows, feats per
        backbone, l4 per backbone, g per class, the heads' y1 | y2 workspace)."""
        if target not in EXPLAIN_TARGETS:
            raise ValueError(f'target must be one of {EXPLAIN_TARGETS} (got {target!r})')
        B, N = x.shape[0], self.n_heads
        merged = torch.empty(B, N + 1, device=self.device, dtype=torch.float32)
        out = torch.empty(B, N, 16, 16, device=self.device, dtype=torch.float32)
        mb = max(1, min(bb.micro_batch for bb in self.backbones))
        readers = [[h for h in range(N) if self.grouping.feat_index[h] == j] for j in range(len(self.backbones))]
        if any(len(r) > 16 for r in readers):
            raise ValueError('explain: more than 16 heads read one backbone (sad_evidence_run takes 1..16 maps)')
        for i in range(0, B, mb):
            xi = x[i:i + mb]
            n = xi.shape[0]
            kept = [bb.keep(xi, kind) for bb in self.backbones]
            self.heads([f for f, _ in kept], merged=merged[i:i + n])
            gs = [self.heads.grad(n, cls) for cls in {'synthetic': (1,), 'real': (0,), 'margin': (1, 0)}[target]]
            for j, (_, l4) in enumerate(kept):
                ev = [evidence(l4, self.dtype, [g[h] for h in readers[j]]) for g in gs]
                e = ev[0] - ev[1] if target == 'margin' else ev[0]
                out[i:i + n, readers[j]] = e.view(n, len(readers[j]), 16, 16)
            if details is not None:
                y = self.heads._ws[:n * N * 768 * 4].view(torch.float32).clone()  # the chunk's y1 | y2
                details.append((slice(i, i + n), [f for f, _ in kept], [a for _, a in kept], gs, y))
        return merged, out

    def explain_pcm(self, pcm: torch.Tensor, target: str = 'synthetic'):
        return self.explain(self.frontend(pcm), 'maps', target)

    def forward_pcm(self, pcm: torch.Tensor):
        return self.forward_maps(self.frontend(pcm))


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stride: int = 1, pad: int = 0,
           res: torch.Tensor | None = None, relu: bool = True, variant: int = 0,
           out: torch.Tensor | None = None) -> torch.Tensor:
    """NHWC conv on the libsad implicit-GEMM kernel.  x [N,H,W,Cin] bf16|fp16|fp32,
    w [Cout,k,k,Cin] same dtype, bias [Cout] fp32, res [N,Ho,Wo,Cout] or None."""
    N, H, W, Cin = x.shape
    Cout, k = w.shape[0], w.shape[1]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dt = _code_of(x)
    if out is None:
        out = torch.empty(N, Ho, Wo, Cout, device=x.device, dtype=x.dtype)
    with torch.cuda.device(x.device):
        _lib.call('sad_conv2d_run', _lib.ptr(x), N, H, W, Cin, _lib.ptr(w), _lib.ptr(bias), _lib.ptr(res),
                  _lib.ptr(out), Cout, k, stride, pad, int(relu), dt, variant, _lib.stream_handle(x.device))
    return out


def block_conv(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stride: int = 1, pad: int = 1,
               sc: torch.Tensor | None = None, sc_stride: int = 1, relu: bool = True, variant: int = 0,
               out: torch.Tensor | None = None, res: torch.Tensor | None = None, k: int = 3,
               split: bool = False, four: bool = False) -> torch.Tensor:
    """conv(x) + 1x1 shortcut(sc) [+ res] as ONE launch (libsad block-conv kernels).
    split=True: every tensor in the split-bf16 layout (``to_split``; dtype 'bf16x3');
    four=True (with split): the four-product form of the deep Bottleneck plans.
    x [N,H,W,Cin], sc [N,H1,W1,Cin1] or None, w [Cout, wt_ld] with the k*k*Cin
    conv taps first and the shortcut's Cin1 columns next (extra columns are
    ignored), bias [Cout] fp32, res [N,Ho,Wo,Cout] (epilogue identity shortcut).
    The tensors' dtype picks the mode: float32, bfloat16 or float16 ('fp16')."""
    N, H, W, Cin = x.shape
    Cout = w.shape[0]
    Cin1 = sc.shape[3] if sc is not None else 0
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dt = _code_of(x)
    if split:  # x, sc, res, out, w in the split-bf16 layout; channel counts are logical
        dt = _lib.SAD_BF16X3
        Cin, Cin1, wt_ld = Cin // 2, Cin1 // 2, w.stride(0) // 2
    else:
        wt_ld = w.stride(0)
    if out is None:
        out = torch.empty(N, Ho, Wo, _act_channels('bf16x3' if split else 'bf16', Cout), device=x.device,
                          dtype=x.dtype)
    H1, W1 = (sc.shape[1], sc.shape[2]) if sc is not None else (0, 0)
    with torch.cuda.device(x.device):
        _lib.call('sad_block_conv_run', _lib.ptr(x), N, H, W, Cin, _lib.ptr(sc), H1, W1, Cin1, sc_stride,
                  _lib.ptr(w), wt_ld, _lib.ptr(bias), _lib.ptr(res), _lib.ptr(out), Cout, k, stride, pad,
                  int(relu), dt, variant | (_lib.SAD_CONV_FOUR_PRODUCTS if four else 0),
                  _lib.stream_handle(x.device))
    return out


def l1_block(x: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """One whole layer1 BasicBlock as the fused kernel (sad_l1_block_run, variant
    40): out = relu(conv3x3(relu(conv3x3(x; w1) + b1); w2) + b2 + x).  x NHWC
    [N,H,W,64] bfloat16 or float16 (H, W multiples of 16); w1, w2 [64, >= 576]
    of x's dtype, k = tap * 64 + ci; b1, b2 [64] fp32."""
    if x.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f'the fused layer1 block runs in bfloat16 or float16 (got {x.dtype})')
    assert w1.dtype == x.dtype and w2.dtype == x.dtype and x.is_contiguous() and x.shape[3] == 64
    assert w1.stride(1) == 1 and w2.stride(1) == 1
    N, H, W, _ = x.shape
    if out is None:
        out = torch.empty_like(x)
    flags = _lib.SAD_L1_BLOCK_F16 if x.dtype == torch.float16 else 0
    with torch.cuda.device(x.device):
        _lib.call('sad_l1_block_run', _lib.ptr(x), N, H, W, _lib.ptr(w1), w1.stride(0), _lib.ptr(b1), _lib.ptr(w2),
                  w2.stride(0), _lib.ptr(b2), _lib.ptr(out), flags, _lib.stream_handle(x.device))
    return out
