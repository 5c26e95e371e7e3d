"""CPU: the evidence entries refuse bad arguments with SAD_ERR_ARG and a
message before any launch or device call (no compute calls: there is no GPU
here).  sad_evidence_run: null l4 / g / g[m] / out, C not a positive multiple
of 64, hw < 1, n_maps outside 1..16, n_maps * C past the LDS budget, a bad
dtype.  The two keep entries: not exactly one of map and img, a null output.
sad_heads_grad_run: null pointers and a class other than 0 / 1.

The pointers handed over are never dereferenced on the refusing paths.
"""
import ctypes

import pytest

SAD_ERR_ARG = -1
FAKE = 0x1000          # a non-null pointer that is never read


def _lib():
    from sad import _lib
    return _lib


def _gp(n, null_at=None):
    return (ctypes.c_void_p * n)(*[None if i == null_at else FAKE for i in range(n)])


def _evidence(l4=FAKE, dtype=1, B=2, hw=256, C=512, g='ok', n_maps=2, out=FAKE):
    L = _lib()
    gp = _gp(max(n_maps, 1)) if g == 'ok' else g
    rc = L.load().sad_evidence_run(l4, dtype, B, hw, C, gp, n_maps, out, None)
    return rc, L.load().sad_last_error()


@pytest.mark.parametrize('kw, word', [
    (dict(l4=None), b'null'),
    (dict(g=None), b'null'),
    (dict(out=None), b'null'),
    (dict(g=_gp(2, null_at=1)), b'null gradient pointer'),
    (dict(C=0), b'multiple of 64'),
    (dict(C=-64), b'multiple of 64'),
    (dict(C=96), b'multiple of 64'),
    (dict(C=520), b'multiple of 64'),
    (dict(hw=0), b'hw'),
    (dict(hw=-3), b'hw'),
    (dict(n_maps=0), b'n_maps'),
    (dict(n_maps=17), b'n_maps'),
    (dict(n_maps=-1), b'n_maps'),
    (dict(n_maps=16, C=4096), b'n_maps * C'),
    (dict(dtype=4), b'dtype'),
    (dict(B=-1), b'batch'),
])
def test_evidence_run_refusals(kw, word):
    rc, msg = _evidence(**kw)
    assert rc == SAD_ERR_ARG, (rc, msg)
    assert msg.startswith(b'argument check failed') and word in msg, msg


def test_evidence_run_empty_batch_launches_nothing():
    """B = 0 with otherwise valid arguments is a no-op, not an error."""
    rc, msg = _evidence(B=0)
    assert rc == 0, msg


@pytest.mark.parametrize('entry', ['sad_backbone_run_keep', 'sad_resnet_run_keep'])
@pytest.mark.parametrize('args, word', [
    ((FAKE, None, None, 2, FAKE, FAKE, FAKE, 1 << 30, None), b'exactly one of map and img'),
    ((FAKE, FAKE, FAKE, 2, FAKE, FAKE, FAKE, 1 << 30, None), b'exactly one of map and img'),
    ((None, FAKE, None, 2, FAKE, FAKE, FAKE, 1 << 30, None), b'null'),
    ((FAKE, FAKE, None, 2, None, FAKE, FAKE, 1 << 30, None), b'null'),
    ((FAKE, FAKE, None, 2, FAKE, None, FAKE, 1 << 30, None), b'null'),
    ((FAKE, FAKE, None, 2, FAKE, FAKE, None, 1 << 30, None), b'null'),
    ((FAKE, FAKE, None, -2, FAKE, FAKE, FAKE, 1 << 30, None), b'negative B'),
])
def test_keep_refusals(entry, args, word):
    L = _lib()
    rc = getattr(L.load(), entry)(*args)
    msg = L.load().sad_last_error()
    assert rc == SAD_ERR_ARG, (rc, msg)
    assert msg.startswith(b'argument check failed') and word in msg, msg


@pytest.mark.parametrize('args, word', [
    ((None, FAKE, 2, 1, FAKE, None), b'null'),
    ((FAKE, None, 2, 1, FAKE, None), b'null'),
    ((FAKE, FAKE, 2, 1, None, None), b'null'),
    ((FAKE, FAKE, 2, 2, FAKE, None), b'cls'),
    ((FAKE, FAKE, 2, -1, FAKE, None), b'cls'),
    ((FAKE, FAKE, -2, 1, FAKE, None), b'negative B'),
])
def test_heads_grad_refusals(args, word):
    L = _lib()
    rc = L.load().sad_heads_grad_run(*args)
    msg = L.load().sad_last_error()
    assert rc == SAD_ERR_ARG, (rc, msg)
    assert msg.startswith(b'argument check failed') and word in msg, msg


def test_refusal_raises_through_the_binding():
    L = _lib()
    with pytest.raises(RuntimeError, match='libsad.*n_maps must be in 1..16'):
        L.call('sad_evidence_run', FAKE, 1, 2, 256, 512, _gp(1), 0, FAKE, None)
