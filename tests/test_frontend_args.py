"""CPU: both front-end plan-create entries of csrc/frontend.hip refuse what
their kernels cannot run before any device call or allocation (no compute
calls: there is no GPU here), and leave *out untouched.

The power buffer of fe_mel_db is FE_POW = 800 floats per wave; bin k of the
bank's non-zero range [bin_lo, bin_hi] lands at slot k - bin_lo + FE_PWPAD
(FE_PWPAD = 8), on the lane path and in the CSR loop alike.  So the plan accepts
bin_hi - bin_lo <= 791 and refuses a wider bank with SAD_ERR_ARG (before the
check, a 0 Hz .. Nyquist bank -- torchaudio's default f_max -- wrote up to slot
1030 of a wave's 800: the next wave's slice).  Also here: sad_crop_resize_run's
n <= 65535 check.
"""
import ctypes

import numpy as np
import pytest

SAD_ERR_ARG = -1
N_FREQS = 1025
SPAN_LIMIT = 791          # FE_POW - FE_PWPAD - 1 (include/sad.h)
SENTINEL = 0x5AD5AD


def _cfg(n_fft=2048, hop=512, n_mels=128, f_min=20.0, f_max=12000.0, slaney=1, n_samples=4096):
    from sad import _lib
    return _lib.FrontendCfg(32000, n_fft, hop, n_mels, f_min, f_max, slaney, 80.0, n_samples)


def _create(cfg, fb=None):
    """(rc, message, *out after the call) of the library-bank or custom-bank entry."""
    from sad import _lib
    lib = _lib.load()
    out = _lib.P(SENTINEL)
    if fb is None:
        rc = lib.sad_frontend_plan_create(ctypes.byref(cfg), ctypes.byref(out))
    else:
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        assert fb.shape == (N_FREQS, max(cfg.n_mels, 1))
        rc = lib.sad_frontend_plan_create_fb(ctypes.byref(cfg), fb.ctypes.data, ctypes.byref(out))
    return rc, lib.sad_last_error(), out.value


def _single_bins(*bins):
    fb = np.zeros((N_FREQS, len(bins)), np.float32)
    for m, k in enumerate(bins):
        fb[k, m] = 1.0
    return fb


def test_library_bank_over_wide_is_refused():
    """0 .. 16000 Hz at 32 kHz: every bin 1..1023 carries weight (span 1022)."""
    rc, msg, out = _create(_cfg(f_min=0.0, f_max=16000.0))
    assert rc == SAD_ERR_ARG
    assert b'exceeds the limit of %d bins' % SPAN_LIMIT in msg, msg
    assert b'bin_hi - bin_lo = 1022' in msg, msg
    assert out == SENTINEL


def test_custom_bank_over_wide_is_refused():
    """Single bins 1 and 793: span 792, one past the last legal power slot."""
    rc, msg, out = _create(_cfg(n_mels=2), _single_bins(1, 793))
    assert rc == SAD_ERR_ARG
    assert b'exceeds the limit of %d bins' % SPAN_LIMIT in msg, msg
    assert b'FFT bins 1..793' in msg, msg
    assert out == SENTINEL


def test_over_wide_bank_raises_through_the_binding():
    from sad import _lib
    cfg = _cfg(f_min=0.0, f_max=16000.0)
    out = _lib.P()
    with pytest.raises(RuntimeError, match='libsad.*exceeds the limit of 791 bins'):
        _lib.call('sad_frontend_plan_create', ctypes.byref(cfg), ctypes.byref(out))
    assert not out.value


@pytest.mark.parametrize('bad', [-1e-3, float('nan'), float('inf')])
def test_custom_bank_weight_must_be_finite_and_non_negative(bad):
    fb = _single_bins(10, 20)
    fb[15, 1] = bad
    rc, msg, out = _create(_cfg(n_mels=2), fb)
    assert rc == SAD_ERR_ARG
    assert b'finite and >= 0' in msg, msg
    assert out == SENTINEL


@pytest.mark.parametrize('kw', [dict(n_fft=1024), dict(n_fft=4096), dict(hop=0), dict(hop=-512), dict(n_mels=1025),
                                dict(n_mels=0), dict(n_samples=1024), dict(n_samples=0)])
@pytest.mark.parametrize('custom', [False, True])
def test_unsupported_configuration_is_refused(kw, custom):
    cfg = _cfg(**kw)
    fb = None
    if custom:
        fb = np.zeros((N_FREQS, max(cfg.n_mels, 1)), np.float32)
        fb[5, :] = 1.0
    rc, msg, out = _create(cfg, fb)
    assert rc == SAD_ERR_ARG
    assert msg.startswith(b'argument check failed'), msg
    assert out == SENTINEL


def test_null_arguments_are_refused():
    from sad import _lib
    lib = _lib.load()
    out = _lib.P(SENTINEL)
    cfg = _cfg()
    assert lib.sad_frontend_plan_create(None, ctypes.byref(out)) == SAD_ERR_ARG
    assert lib.sad_frontend_plan_create(ctypes.byref(cfg), None) == SAD_ERR_ARG
    assert lib.sad_frontend_plan_create_fb(ctypes.byref(cfg), None, ctypes.byref(out)) == SAD_ERR_ARG
    assert out.value == SENTINEL


def test_crop_resize_refuses_more_than_65535_maps():
    """The grid's y dimension: the entry answers before it launches (the
    pointers are never read)."""
    from sad import _lib
    lib = _lib.load()
    buf = np.zeros(16, np.float32)
    for dt in (_lib.SAD_F32, _lib.SAD_BF16):
        rc = lib.sad_crop_resize_run(buf.ctypes.data, 65536, 2, 3, None, 512, dt, buf.ctypes.data, None)
        assert rc == SAD_ERR_ARG
        assert b'n > 65535' in lib.sad_last_error()
