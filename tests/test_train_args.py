"""CPU: the BatchNorm workspace-size entries of csrc/train.hip refuse a channel
count their kernels cannot run, before any arithmetic on it, and size the
workspace by the documented formula (no compute calls: there is no GPU here).

bn_nblocks(P, C) works with R = 256 / (C / 8) rows per workgroup pass and
ceil(P / (16 R)) workgroups, at least 1 and at most 1024.  C < 8 made C / 8 zero and
C > 2048 made R zero: an integer division by zero in host code, where the _run
entries answer SAD_ERR_ARG.  The size entries now make the same check (a
multiple of 8 in [8, 2048]) first.
"""
import ctypes

import pytest

SAD_ERR_ARG = -1


def _bn_nblocks(P, C):
    R = 256 // (C // 8)
    return max(1, min(1024, (P + R * 16 - 1) // (R * 16)))


def _bn_bytes(P, C):
    """[nblocks][2][C] fp32 partials + [3][C] fp32 backward coefficients:
    what sad_bn_stats_run / sad_bn_backward_run require of ws_bytes."""
    return _bn_nblocks(P, C) * 2 * C * 4 + 3 * C * 4


@pytest.mark.parametrize('C', [4, 12, 2056, 4096])
def test_bn_workspace_size_refuses_unsupported_channels(C):
    from sad import _lib
    lib = _lib.load()
    sz = _lib.SZ(12345)
    rc = lib.sad_bn_workspace_size(1000, C, ctypes.byref(sz))
    assert rc == SAD_ERR_ARG
    assert b'multiple of 8 in [8, 2048]' in lib.sad_last_error()
    assert sz.value == 12345
    with pytest.raises(RuntimeError, match='libsad'):
        _lib.call('sad_bn_workspace_size', 1000, C, ctypes.byref(sz))


@pytest.mark.parametrize('Cout', [4, 12, 2056, 4096])
def test_conv_bn_train_workspace_size_refuses_unsupported_channels(Cout):
    from sad import _lib
    lib = _lib.load()
    sz = _lib.SZ(12345)
    rc = lib.sad_conv_bn_train_workspace_size(2, 16, 16, Cout, 3, 1, 1, ctypes.byref(sz))
    assert rc == SAD_ERR_ARG
    assert b'multiple of 8 in [8, 2048]' in lib.sad_last_error()
    assert sz.value == 12345


@pytest.mark.parametrize('C', [8, 24, 136, 2048])
@pytest.mark.parametrize('P', [0, 1, 511, 512, 513, 4097, 16389, 1 << 24])
def test_bn_workspace_size_follows_the_formula(P, C):
    """The rows-per-pass and the 1024-workgroup cap, on both sides of each."""
    from sad import _lib
    sz = _lib.SZ()
    _lib.call('sad_bn_workspace_size', P, C, ctypes.byref(sz))
    assert sz.value == _bn_bytes(P, C)


def test_bn_workspace_size_cap_and_minimum():
    assert _bn_nblocks(0, 8) == 1 and _bn_nblocks(4096, 8) == 1 and _bn_nblocks(4097, 8) == 2
    assert _bn_nblocks(16389, 2048) == 1024 and _bn_nblocks(16384, 2048) == 1024 and _bn_nblocks(16368, 2048) == 1023


@pytest.mark.parametrize('Cout', [8, 2048])
@pytest.mark.parametrize('N,H,k,stride,pad', [(0, 8, 3, 1, 1), (2, 16, 3, 1, 1), (64, 128, 1, 2, 0), (512, 128, 3, 1, 1)])
def test_conv_bn_train_workspace_size_follows_the_formula(Cout, N, H, k, stride, pad):
    """max(fused: 512 partial rows, unfused: the bn_reduce pass over the output)."""
    from sad import _lib
    sz = _lib.SZ()
    _lib.call('sad_conv_bn_train_workspace_size', N, H, H, Cout, k, stride, pad, ctypes.byref(sz))
    Ho = (H + 2 * pad - k) // stride + 1
    fused = 512 * 2 * Cout * 4 + 3 * Cout * 4
    assert sz.value == max(fused, _bn_bytes(N * Ho * Ho, Cout))


def test_size_entries_refuse_null_output():
    from sad import _lib
    lib = _lib.load()
    assert lib.sad_bn_workspace_size(10, 64, None) == SAD_ERR_ARG
    assert lib.sad_conv_bn_train_workspace_size(1, 8, 8, 64, 3, 1, 1, None) == SAD_ERR_ARG
