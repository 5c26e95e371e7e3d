"""CPU: both backbone plan-create entries (api.hip sad_backbone_plan_create,
resnet.hip sad_resnet_plan_create) refuse a map the stem would have to
DOWNSAMPLE, before any allocation or device call, and leave *out untouched (no
compute calls: there is no GPU here).

The stems' in-kernel resize is the plain bilinear filter -- what the
reference's antialiased Resize((512,512)) reduces to when it enlarges.  A map
side above 512 would be point-sampled instead of filtered, so the limit is 512
per side (include/sad.h).  The parameter pointers are never read on the
refusing path; at 512 x 512 the shape check passes and the call fails later, on
the first device call, with another status.
"""
import ctypes

import numpy as np
import pytest

SAD_ERR_ARG = -1
SENTINEL = 0x5AD5AD
LIMIT_MSG = b'exceeds the limit of 512 per side'


def _params(n):
    """n non-null host pointers into one zero buffer: never read on the
    refusing path, and as large as the largest parameter (a 512 x 512 x 3 x 3
    conv) for the call that passes the check where there is a device."""
    buf = np.zeros(512 * 512 * 9, np.float32)
    return buf, (ctypes.c_void_p * n)(*([buf.ctypes.data] * n))


def _backbone(map_h, map_w):
    from sad import _lib
    lib = _lib.load()
    buf, arr = _params(100)
    out = _lib.P(SENTINEL)
    rc = lib.sad_backbone_plan_create(arr, 100, _lib.SAD_BF16, map_h, map_w, ctypes.byref(out))
    msg = lib.sad_last_error()
    if rc == 0:
        lib.sad_backbone_plan_destroy(out)
    return rc, msg, out.value


def _resnet(map_h, map_w, layers=(3, 4, 6, 3)):
    from sad import _lib
    from sad.weights import backbone_param_shapes
    lib = _lib.load()
    n = sum(1 if kind == 'conv' else 4 for _, _, kind in backbone_param_shapes(layers, 'bottleneck'))
    buf, arr = _params(n)
    out = _lib.P(SENTINEL)
    lay = (_lib.I32 * 4)(*layers)
    rc = lib.sad_resnet_plan_create(arr, n, 1, lay, _lib.SAD_BF16X3, map_h, map_w, ctypes.byref(out))
    msg = lib.sad_last_error()
    if rc == 0:
        lib.sad_resnet_plan_destroy(out)
    return rc, msg, out.value


@pytest.mark.parametrize('create', [_backbone, _resnet])
@pytest.mark.parametrize('shape', [(513, 251), (128, 513)])
def test_downsampling_map_is_refused(create, shape):
    rc, msg, out = create(*shape)
    assert rc == SAD_ERR_ARG
    assert msg.startswith(b'argument check failed'), msg
    assert LIMIT_MSG in msg and b'%d x %d' % shape in msg, msg
    assert b'upsampling only' in msg, msg
    assert out == SENTINEL


@pytest.mark.parametrize('create', [_backbone, _resnet])
def test_full_size_map_passes_the_shape_check(create):
    """512 x 512 (the identity resize) is legal: whatever the call answers on a
    machine without a device, it is not the map-shape refusal."""
    rc, msg, out = create(512, 512)
    if rc == 0:        # a device is present: the plan was built (and destroyed again)
        return
    assert LIMIT_MSG not in msg and b'map shape' not in msg, msg


@pytest.mark.parametrize('create', [_backbone, _resnet])
@pytest.mark.parametrize('shape', [(0, 251), (128, -1)])
def test_empty_map_is_still_refused(create, shape):
    rc, msg, out = create(*shape)
    assert rc == SAD_ERR_ARG and b'map shape' in msg, msg
    assert out == SENTINEL


def test_refusal_raises_through_the_binding():
    from sad import _lib
    buf, arr = _params(100)
    out = _lib.P()
    with pytest.raises(RuntimeError, match='libsad.*600 x 251 exceeds the limit of 512 per side'):
        _lib.call('sad_backbone_plan_create', arr, 100, _lib.SAD_F32, 600, 251, ctypes.byref(out))
    assert not out.value
