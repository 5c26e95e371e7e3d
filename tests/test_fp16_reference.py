"""CPU: tests/fp16_ref.py's bar is sharp.  On variant 31's smallest case of
tests/test_gpu_kstep_parity.py (l2ds-31: 128 -> 128 channels on a 64 x 64 map,
the 1x1/2 downsample of a 64-channel source as one more K chunk; one image is
enough here) the bar
  * accepts a float32-accumulated F.conv2d rounded once to fp16;
  * rejects, with more than 10 % of the elements over it, the same output
    rounded through bf16, the same conv with bf16-rounded weights, and the conv
    without its last 64-channel K chunk.
"""
import zlib

import pytest
import torch
import torch.nn.functional as F

import fp16_ref as R16

NAME, N, H, CIN, COUT, CIN1 = 'l2ds-31', 1, 64, 128, 128, 64
K = 9 * CIN + CIN1


@pytest.fixture(scope='module')
def case():
    g = torch.Generator().manual_seed(zlib.crc32(NAME.encode()))
    x = R16.rand_f16(g, N, H, H, CIN)
    sc = R16.rand_f16(g, N, 2 * H, 2 * H, CIN1)
    w = R16.rand_f16(g, COUT, K)
    bias = torch.randn(COUT, generator=g) * 0.1
    ref = R16.conv_ref(x, w, bias, 1, sc, 2)
    return x, sc, w, bias, ref


def _f32_conv(x, sc, w, bias, drop_last=False):
    """float32-accumulated conv of the operands (NHWC out, fp32)."""
    wc = w[:, :9 * CIN].float().reshape(COUT, 3, 3, CIN).permute(0, 3, 1, 2)
    y = F.conv2d(x.float().permute(0, 3, 1, 2), wc, padding=1)
    if not drop_last:
        y = y + F.conv2d(sc.float().permute(0, 3, 1, 2), w[:, 9 * CIN:].float()[:, :, None, None], stride=2)
    return (y + bias.view(1, -1, 1, 1)).clamp_min(0).permute(0, 2, 3, 1)


def test_operands_in_normal_range(case):
    x, sc, w, _, ref = case
    for t in (x, sc, w):
        m = t.abs().double()
        assert bool(((m == 0) | ((m >= 2.0 ** -8) & (m <= 8.0))).all())
    assert (ref > 0).double().mean().item() > 0.25


def test_accepts_f32_accumulation_rounded_to_fp16(case):
    x, sc, w, bias, ref = case
    y32 = _f32_conv(x, sc, w, bias)
    frac, worst = R16.over_bar(y32.to(torch.float16), ref, K)
    # the accumulation alone against the floor term alone
    floor = 4.0 * K ** 0.5 * R16.U32 * ref.abs().max()
    acc = ((y32.double() - ref).abs().max() / floor).item()
    print(f'RATIO fp16 bar {NAME}: rounded stand-in worst |d|/bar {worst:.3f}, fp32 accumulation / floor {acc:.3f}')
    assert frac == 0.0 and worst <= 1.0
    assert acc <= 1.0


def test_rejects_bf16_output_rounding(case):
    x, sc, w, bias, ref = case
    out = _f32_conv(x, sc, w, bias).to(torch.bfloat16).float()
    frac, _ = R16.over_bar(out, ref, K)
    print(f'bf16-rounded output: {frac:.3f} of the elements over the bar')
    assert frac > 0.10


def test_rejects_bf16_weights(case):
    x, sc, w, bias, ref = case
    out = _f32_conv(x, sc, w.to(torch.bfloat16).to(torch.float16), bias).to(torch.float16)
    frac, _ = R16.over_bar(out, ref, K)
    print(f'bf16-rounded weights: {frac:.3f} of the elements over the bar')
    assert frac > 0.10


def test_rejects_dropped_last_k_chunk(case):
    x, sc, w, bias, ref = case
    out = _f32_conv(x, sc, w, bias, drop_last=True).to(torch.float16)
    frac, _ = R16.over_bar(out, ref, K)
    print(f'last 64-channel K chunk dropped: {frac:.3f} of the elements over the bar')
    assert frac > 0.10


def test_saturate_and_exact_operands():
    g = torch.Generator().manual_seed(5)
    x, w, bias, sc, r = R16.exact_operands(g, 1, 8, 8, 64, 64, cin1=64, sc_hw=(16, 16), res=True)
    assert int((w != 0).sum(1).max()) <= 16 and set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    ref = R16.conv_ref(x, w, bias, 1, sc, 2, r)
    assert torch.equal(ref, ref.round()) and ref.abs().max() < 256      # integers exact in bf16 and fp16
    assert torch.equal(R16.saturate(torch.tensor([1e5, -1e5, 3.0], dtype=torch.float64)),
                       torch.tensor([65504.0, -65504.0, 3.0], dtype=torch.float64))
