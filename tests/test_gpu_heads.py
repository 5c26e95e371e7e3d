"""GPU: sad_heads_merge_run stage by stage -- the first Linear of all heads of
one backbone as one fp32 GEMM, the second as one grouped launch or one launch
per head, heads_final_kernel's last Linear + merge -- element for element
against the float64 reference of tests/heads_ref.py under that file's a-priori
bars ((K + 8) u (sum |x| |w'| + |b'|) per stage, each stage on the input the
device itself stored for it; exact zeros where the pre-activation is <= -bar;
merged synthetic columns bit for bit; the real mean within (N + 2) u).  No bar
is a measured error, no element is left out, and every case prints its worst
error / bar per stage.

Reached here and nowhere else in the suite: irregular plans (hidden columns in
group order, second layer per head) against an independent reference, an empty
feature group with a NULL pointer, one head, feat_dim 64 and 2048, logits =
NULL, B on either side of the 128-row tile and B % 4 != 0, BatchNorm statistics
with tiny variances and zero / negative gammas, guard regions behind every
buffer, position invariance of a row, the refusals before any launch, and a
batch past the 2 GiB range of the GEMM operands (64 heads, 16,645 rows).
"""
import ctypes

import pytest
import torch

import heads_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SAD_ERR_ARG, SAD_ERR_NOMEM = -1, -4
GUARD = 4096                     # sentinel bytes before and after every buffer
FILL = 0xFF                      # (as fp32: NaN, so an unwritten element fails the comparison)


class Guarded:
    """A device buffer of `nbytes` between two guard regions, all bytes FILL."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.raw = torch.full((GUARD + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)

    @property
    def ptr(self):
        return self.raw.data_ptr() + GUARD

    def floats(self, *shape):
        return self.raw[GUARD:GUARD + self.nbytes].view(torch.float32).view(*shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == FILL).all() and (self.raw[GUARD + self.nbytes:] == FILL).all())

    def untouched(self):
        return bool((self.raw == FILL).all())


def _lib():
    from sad import _lib
    return _lib


def _plan(sds, feat_index, n_feat, feat_dim):
    from sad.engine import Heads
    return Heads(sds, feat_index, n_feat, DEV, feat_dim=feat_dim)


def _ws_bytes(heads, B):
    L = _lib()
    sz = L.SZ()
    L.call('sad_heads_workspace_size', heads._plan, B, ctypes.byref(sz))
    assert sz.value >= R.workspace_floats(B, heads.n_heads) * 4
    return sz.value


def _raw(heads, dev_feats, B, want_logits=True, ws_short=0):
    """One raw sad_heads_merge_run into guarded buffers -> (rc, logits, merged, ws)."""
    L = _lib()
    N = heads.n_heads
    logits, merged = Guarded(B * N * 2 * 4), Guarded(B * (N + 1) * 4)
    ws = Guarded(_ws_bytes(heads, B))
    fp = (ctypes.c_void_p * len(dev_feats))(*[L.ptr(f) for f in dev_feats])
    with torch.cuda.device(DEV):
        rc = L.load().sad_heads_merge_run(heads._plan, fp, B, logits.ptr if want_logits else None, merged.ptr,
                                          ws.ptr, ws.nbytes - ws_short, L.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, logits, merged, ws


def _check(case, folded, feats, logits, merged, ws, B):
    N = case.n_heads
    for g in (logits, merged, ws):
        assert g.guards_intact(), case.name
    r = R.compare(folded, feats, case.feat_index, ws.floats(-1).cpu(), logits.floats(B, N, 2).cpu(),
                  merged.floats(B, N + 1).cpu())
    print(f'RATIO {case.name}: ' + ', '.join(f'{k} {v:.3g}' for k, v in r.items()))
    assert R.passes(r), (case.name, r)


@pytest.mark.parametrize('case', R.CASES, ids=lambda c: c.name)
def test_stages_and_merge_against_float64(case):
    sds, feats = R.make_case(case)
    folded = [R.fold(sd) for sd in sds]
    heads = _plan(sds, case.feat_index, case.n_feat, case.feat_dim)
    L = _lib()
    grouped, rows = L.I32(-1), L.I64(-1)
    L.call('sad_heads_plan_info', heads._plan, ctypes.byref(grouped), ctypes.byref(rows))
    assert bool(grouped.value) == R.is_regular(case.feat_index) == all(
        r == h for h, r in enumerate(R.rank(case.feat_index)))
    assert rows.value == R.row_range(case.n_heads, case.feat_dim)
    dev = [None if f is None else f.to(DEV) for f in feats]
    N, B = case.n_heads, case.B
    rc, logits, merged, ws = _raw(heads, dev, B)
    assert rc == 0, L.load().sad_last_error()
    _check(case, folded, feats, logits, merged, ws, B)

    # logits = NULL: the same merged, bit for bit, and the same workspace
    rc, l0, m0, w0 = _raw(heads, dev, B, want_logits=False)
    assert rc == 0 and l0.untouched() and m0.guards_intact() and w0.guards_intact()
    assert torch.equal(m0.raw, merged.raw)
    assert torch.equal(w0.floats(-1)[:R.workspace_floats(B, N)].view(torch.int32),
                       ws.floats(-1)[:R.workspace_floats(B, N)].view(torch.int32))

    # the engine's wrapper is the raw call
    wl, wm = heads(dev)
    torch.cuda.synchronize()
    assert torch.equal(wl.view(torch.int32), logits.floats(B, N, 2).view(torch.int32))
    assert torch.equal(wm.view(torch.int32), merged.floats(B, N + 1).view(torch.int32))


@pytest.mark.parametrize('plan', [(6, [0] * 6, 1), (4, [0, 1, 2, 0], 3)], ids=['regular', 'irregular'])
def test_a_row_does_not_depend_on_its_position(plan):
    """Rows run alone equal the same rows inside a larger batch bit for bit (the
    K order per row is fixed; the row-range loop and any chunking rely on it)."""
    n, fi, nf = plan
    case = next(c for c in R.CASES if c.n_heads == n and c.feat_index == fi and c.B == 257)
    sds, feats = R.make_case(case)
    heads = _plan(sds, fi, nf, 512)
    rc, logits, merged, ws = _raw(heads, [f.to(DEV) for f in feats], 257)
    assert rc == 0
    y1, y2 = R.split_workspace(ws.floats(-1), 257, fi)
    for rows in ([126, 127, 128, 129, 130], [256], [0, 255, 3]):
        rc, ls, ms, wss = _raw(heads, [f[rows].to(DEV) for f in feats], len(rows))
        assert rc == 0
        a1, a2 = R.split_workspace(wss.floats(-1), len(rows), fi)
        for big, small in ((logits.floats(257, n, 2), ls.floats(len(rows), n, 2)),
                           (merged.floats(257, n + 1), ms.floats(len(rows), n + 1)), (y1, a1), (y2, a2)):
            assert torch.equal(big[rows].contiguous().view(torch.int32), small.contiguous().view(torch.int32)), rows


def test_empty_batch_writes_nothing():
    case = R.CASES[0]
    sds, feats = R.make_case(case)
    heads = _plan(sds, case.feat_index, case.n_feat, case.feat_dim)
    L = _lib()
    logits, merged, ws = Guarded(64), Guarded(64), Guarded(_ws_bytes(heads, 0))
    fp = (ctypes.c_void_p * 1)(feats[0].to(DEV).data_ptr())
    rc = L.load().sad_heads_merge_run(heads._plan, fp, 0, logits.ptr, merged.ptr, ws.ptr, ws.nbytes,
                                      L.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0 and logits.untouched() and merged.untouched() and ws.untouched()


# ---------------------------------------------------------------- refusals --
def test_short_workspace_is_refused_before_any_launch():
    case = next(c for c in R.CASES if c.feat_index == [0, 1, 2, 0] and c.B == 3)
    sds, feats = R.make_case(case)
    heads = _plan(sds, case.feat_index, case.n_feat, case.feat_dim)
    rc, logits, merged, ws = _raw(heads, [f.to(DEV) for f in feats], case.B, ws_short=1)
    assert rc == SAD_ERR_NOMEM and b'workspace' in _lib().load().sad_last_error()
    assert logits.untouched() and merged.untouched() and ws.untouched()


def test_null_features_of_a_used_group_are_refused_before_any_launch():
    """Group 2 of [0,1,2,0] is NULL: groups 0 and 1 must not have been queued."""
    case = next(c for c in R.CASES if c.feat_index == [0, 1, 2, 0] and c.B == 3)
    sds, feats = R.make_case(case)
    heads = _plan(sds, case.feat_index, case.n_feat, case.feat_dim)
    dev = [f.to(DEV) for f in feats]
    rc, logits, merged, ws = _raw(heads, dev[:2] + [None], case.B)
    assert rc == SAD_ERR_ARG and b'null feature' in _lib().load().sad_last_error()
    assert logits.untouched() and merged.untouched() and ws.untouched()


@pytest.mark.parametrize('what', ['feat_dim 96', 'feat_index 2 of 2', 'feat_index -1'])
def test_plan_create_refusals_leave_out_untouched(what):
    from sad.engine import _head_arrays
    L = _lib()
    feat_dim = 96 if what == 'feat_dim 96' else 512
    fi = {'feat_dim 96': [0, 1], 'feat_index 2 of 2': [0, 2], 'feat_index -1': [-1, 0]}[what]
    gen = torch.Generator().manual_seed(5)
    arrays = [a for _ in fi for a in _head_arrays(R.random_head(gen, feat_dim), feat_dim)]
    plan = L.P(0x5AD0)
    with torch.cuda.device(DEV):
        rc = L.load().sad_heads_plan_create_dim(L.pointer_array(arrays), len(fi), (L.I32 * len(fi))(*fi), 2,
                                                feat_dim, ctypes.byref(plan))
    assert rc == SAD_ERR_ARG and plan.value == 0x5AD0
    assert (b'feat_dim' if what == 'feat_dim 96' else b'feat_index') in L.load().sad_last_error()


def test_wrapper_checks_its_features():
    case = next(c for c in R.CASES if c.feat_index == [0, 1, 0, 1])
    sds, feats = R.make_case(case)
    heads = _plan(sds, case.feat_index, case.n_feat, case.feat_dim)
    a, b = [f.to(DEV) for f in feats]
    heads([a, b])
    bad = {
        'not fp32': [a, b.double()],
        'not contiguous': [a, torch.cat([b, b], dim=1)[:, :512]],
        'another device': [a, b.cpu()],
        'wrong width': [a, torch.cat([b, b], dim=1)],
        'not 2-D': [a, b.view(-1)],
        'no common B': [a, b[:-1]],
        'one tensor short': [a],
        'a used group missing': [a, None],
    }
    for name, fs in bad.items():
        with pytest.raises(ValueError):
            heads(fs)
    torch.cuda.synchronize()


# ------------------------------------------------------------- large batch --
def test_batch_past_the_buffer_range_runs_as_row_ranges():
    """64 heads on one backbone: the second GEMM's operand passes 2 GiB after
    16,384 rows.  B = 16,645 runs as two row ranges (the workspace, 3.3 GB, is
    allocated for real); the rows round the range boundary, the first and the
    last rows equal the same rows run as a small batch bit for bit, and that
    small batch meets the per-stage bars."""
    N, B, rows = R.LARGE_N, R.LARGE_B, R.LARGE_ROWS
    sds, big = R.make_large()
    heads = _plan(sds, [0] * N, 1, 512)
    assert B > R.row_range(N, 512) and ((B - 1) * N * 512 + 512) * 4 >= 2 ** 31 - 64
    x = big.to(DEV)
    rc, logits, merged, ws = _raw(heads, [x], B)
    assert rc == 0, _lib().load().sad_last_error()
    assert logits.guards_intact() and merged.guards_intact() and ws.guards_intact()
    small = big[rows].clone()
    rc, ls, ms, wss = _raw(heads, [small.to(DEV)], len(rows))
    assert rc == 0
    idx = torch.tensor(rows, device=DEV)
    wf = ws.floats(-1)
    pairs = ((logits.floats(B, N * 2), ls.floats(len(rows), N * 2)),
             (merged.floats(B, N + 1), ms.floats(len(rows), N + 1)),
             (wf[:B * N * 512].view(B, N * 512), wss.floats(-1)[:len(rows) * N * 512].view(len(rows), N * 512)),
             (wf[B * N * 512:B * N * 768].view(B, N * 256),
              wss.floats(-1)[len(rows) * N * 512:len(rows) * N * 768].view(len(rows), N * 256)))
    for bigt, smallt in pairs:
        assert torch.equal(bigt[idx].view(torch.int32), smallt.contiguous().view(torch.int32))
    # every row of the large run was written (no NaN fill left anywhere)
    assert bool(torch.isfinite(merged.floats(B, N + 1)).all()) and bool(torch.isfinite(logits.floats(B, N * 2)).all())
    case = R.LARGE._replace(B=len(rows))
    _check(case, [R.fold(sd) for sd in sds], [small], ls, ms, wss, len(rows))
