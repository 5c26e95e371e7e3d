"""CPU: the layer2 resident-weight conv's patch-piece table, shortcut pieces,
tile walk and hoisted lane constants (csrc/l2conv.hip, variants 41 / 42),
restated from the kernel's formulas and checked exhaustively.

* piece table: entry (wave, k, lane) = edge bits << 27 | source offset / 16
  from the tile's first patch pixel (one row up, one pixel left of the tile);
  edge bits: slot >= 324 (bit 27, which the shift to bytes leaves on top), row
  0, row 17, column 0, column 17.  A piece's source is the zero offset where
  entry & the tile's mask is non-zero (the mask always holds bit 27).  For
  every tile position class and both chunks the 41 pieces write every 16-B
  chunk of the 18 x 18 x 128-B patch exactly once, with what
  tests/test_rwconv_layout.py's readers expect there, and zeros exactly where
  the pixel lies outside the image or the slot is past the patch;
* an entry's offset fits its 27 bits wherever it is used, and never reaches
  the edge bits; the table's last byte lies inside the 160 KB budget in all
  three LDS layouts;
* a residual / downsample piece: one lane constant per wave plus a uniform
  term equals the per-piece formula it replaces, for every (wave, k, lane);
* the tile walk by steps visits the tiles that the division decodes, for
  workgroup ranges that begin and end mid-row and mid-image;
* the lane constants kept in registers give the addresses of the formulas they
  replace (those that tests/test_rwconv_layout.py checks for conflicts).
"""
import test_rwconv_layout as lay

NW, PW, PR, NDP, QP = 4, 18, 324, 41, 11
PATCH, ROWB = NDP * 1024, PW * 128
RESB = 256 * 256
OFF_RES = 2 * PATCH
SMEM_RES = OFF_RES + RESB
TABB = NW * QP * 256
LDS_BYTES = 160 * 1024
BAD = 0x7FFFFFF0
ESH = 27
M32 = 0xFFFFFFFF
key = lay.key30


def entry(wave, k, lane, W, ps):
    r = 8 * (wave + NW * k) + (lane >> 3)
    Y = (r * 3641) >> 16
    X = r - PW * Y
    edge = ((1 if r >= PR else 0) | (2 if Y == 0 else 0) | (4 if Y == PW - 1 else 0) | (8 if X == 0 else 0) |
            (16 if X == PW - 1 else 0))
    off = ((((Y * W + X) * ps + (((lane & 7) ^ key(X)) << 4)) & M32) >> 4)  # 32-bit arithmetic, as the kernel's
    return ((edge << ESH) | (off & ((1 << ESH) - 1))) & M32


def patch_mask(oy0, ox0, H, W):
    return (1 | (2 if oy0 == 0 else 0) | (4 if oy0 + 16 == H else 0) | (8 if ox0 == 0 else 0) |
            (16 if ox0 + 16 == W else 0)) << ESH


def piece_voff(e, pbase, pmask):
    return BAD if e & pmask else (pbase + ((e << 4) & M32)) & M32


def wave_pieces(wave):
    """the k this wave issues (the kernel's uniform test, compiled into k = 10 only)"""
    return [k for k in range(QP) if not (NW * k + NW - 1 >= NDP and wave + NW * k >= NDP)]


def test_r_over_18_by_multiply():
    for r in range(8 * NW * QP):
        assert (r * 3641) >> 16 == r // PW


def test_only_wave_0_has_the_last_piece():
    assert [len(wave_pieces(w)) for w in range(NW)] == [QP, QP - 1, QP - 1, QP - 1]
    assert sorted(w + NW * k for w in range(NW) for k in wave_pieces(w)) == list(range(NDP))


def test_table_fits_the_lds_budget():
    # plain / ST / X3 plain: behind the two patch buffers; RES / DS: behind the shortcut tile
    for off_b in (OFF_RES, SMEM_RES):
        off_t = off_b + 512
        last = 0
        for wave in range(NW):
            for k in range(QP):  # the loop reads entry k + 1 while it issues piece k: k + 1 <= QP - 1
                for lane in range(64):
                    ad = off_t + (wave * QP * 64 + lane) * 4 + 256 * k
                    assert off_t <= ad and ad + 4 <= off_t + TABB
                    last = max(last, ad + 4)
        assert last == off_t + TABB <= LDS_BYTES


def test_entry_offset_fits_its_bits():
    # an entry that a tile uses addresses a pixel inside the image, and the
    # launcher keeps the input under 2^31 - 65536 bytes: offset / 16 < 2^27.
    # The largest used offset is patch row 17 (only where the image has >= 32
    # rows) or row 16 of a 16-row image, pixel column 17, chunk 7
    lim = (1 << 31) - 65536
    for H in (16, 32):
        for ps in (256, 272, 1024):
            W = (lim // (H * ps)) // 16 * 16
            assert H * W * ps <= lim
            Ymax = 17 if H > 16 else 16
            assert ((Ymax * W + 17) * ps + 7 * 16) >> 4 < 1 << ESH
    # an entry that no tile uses (a 16-row image's rows 0 and 17 at a width where
    # the product passes 2^31) still carries its edge bits intact
    W, ps = 500_000 // 16 * 16, 256
    assert 17 * W * ps >= 1 << 31
    for wave in range(NW):
        for k in wave_pieces(wave):
            for lane in range(64):
                r = 8 * (wave + NW * k) + (lane >> 3)
                Y, X = divmod(r, PW)
                e = entry(wave, k, lane, W, ps)
                assert e >> ESH == ((r >= PR) | (Y == 0) << 1 | (Y == 17) << 2 | (X == 0) << 3 | (X == 17) << 4)


def _tile_classes():
    # (H, W, oy0, ox0): every combination of shared edges, the one-tile image included
    out = []
    for H, W in ((16, 16), (16, 48), (48, 16), (48, 64), (32, 32)):
        for oy0 in range(0, H, 16):
            for ox0 in range(0, W, 16):
                out.append((H, W, oy0, ox0))
    return out


def test_pieces_write_every_chunk_once_and_right():
    seen_masks = set()
    for ps in (256, 272):  # 128 channels packed; a padded pixel stride
        for H, W, oy0, ox0 in _tile_classes():
            b = 1  # second image of a batch: the base is non-zero
            base = ((b * H + oy0) * W + ox0) * ps
            pmask = patch_mask(oy0, ox0, H, W)
            seen_masks.add(pmask >> (ESH + 1))
            for c in range(2):
                pbase = (base - (W + 1) * ps + 128 * c) & M32
                written = {}
                for wave in range(NW):
                    for k in wave_pieces(wave):
                        q = wave + NW * k
                        for lane in range(64):
                            dst = c * PATCH + k * NW * 1024 + wave * 1024 + lane * 16  # M0 = dstw + the immediate
                            assert dst == c * PATCH + q * 1024 + lane * 16 and dst not in written
                            written[dst] = piece_voff(entry(wave, k, lane, W, ps), pbase, pmask)
                assert sorted(written) == list(range(c * PATCH, (c + 1) * PATCH, 16))
                # what each LDS chunk holds: (patch row, patch column, source chunk) or zeros
                held = {}
                for dst, voff in written.items():
                    slot, pos = (dst - c * PATCH) // 128, (dst % 128) // 16
                    Y, X = divmod(slot, PW)
                    iy, ix = oy0 - 1 + Y, ox0 - 1 + X
                    g = pos ^ key(X)
                    if slot < PR and 0 <= iy < H and 0 <= ix < W:
                        assert voff == ((b * H + iy) * W + ix) * ps + c * 128 + g * 16
                        held[dst] = (Y, X, g)
                    else:
                        assert voff == BAD
                        held[dst] = (Y, X, g) if slot < PR else None  # zeros stand for the padding pixel
                # the readers of test_rwconv_layout.py find their pixel and channels there
                for ky in range(3):
                    for kx in range(3):
                        for h in range(2):
                            for j in range(16):
                                for lane in range(64):
                                    frt, fgt = lane & 15, lane >> 4
                                    a = (((frt + kx) * 128 + ((fgt ^ key(frt + kx)) << 4)) ^ (h << 6)) + (j + ky) * ROWB
                                    assert held[c * PATCH + a] == (j + ky, frt + kx, fgt + 4 * h)
    assert seen_masks == set(range(16))  # every edge combination


def test_residual_and_downsample_pieces_are_one_lane_constant():
    H, W, b, oy0, ox0 = 48, 32, 2, 16, 16
    # residual: 16 pieces per wave, pixels 4q .. 4q + 3 of the tile, 256 B each
    for psr in (256, 272):
        srow = W * psr
        sbase = ((b * H + oy0) * W + ox0) * psr
        for wave in range(NW):
            for lane in range(64):
                pxr = 4 * wave + (lane >> 4)
                RV = pxr * psr + (((lane & 15) ^ pxr) << 4)
                for k in range(16):
                    q = wave + NW * k
                    px, pos = 4 * q + (lane >> 4), lane & 15
                    chunk = pos ^ (px & 15)
                    off = ((b * H + oy0 + (px >> 4)) * W + ox0 + (px & 15)) * psr + chunk * 16
                    assert RV + (sbase + k * srow) == off
                    # the LDS side: M0 = the wave's piece 0 + the piece's immediate
                    assert OFF_RES + k * NW * 1024 + wave * 1024 == OFF_RES + q * 1024
    # downsample: 8 pieces per wave, pixels 8q .. 8q + 7, 128 B each, source at stride 2
    ss1, H1, W1 = 2, 2 * H, 2 * W
    for ps1 in (128, 144):
        pss, srow = ss1 * ps1, ss1 * W1 * ps1
        sbase = ((b * H1 + oy0 * ss1) * W1 + ox0 * ss1) * ps1
        for wave in range(NW):
            for lane in range(64):
                pxd = 8 * (wave & 1) + (lane >> 3)
                DV = (wave >> 1) * srow + pxd * pss + (((lane & 7) ^ ((pxd >> 1) & 7)) << 4)
                for k in range(8):
                    q = wave + NW * k
                    px, pos = 8 * q + (lane >> 3), lane & 7
                    chunk = pos ^ ((px >> 1) & 7)
                    off = ((b * H1 + (oy0 + (px >> 4)) * ss1) * W1 + (ox0 + (px & 15)) * ss1) * ps1 + chunk * 16
                    assert DV + (sbase + 2 * k * srow) == off
                    assert lay.ds_write_map()[q * 1024 + lane * 16] == (px, chunk)


def _decode(t, H, W, ps, pso, psr, ps1):
    tiles_x, tiles_img = W // 16, (W // 16) * (H // 16)
    b, rem = divmod(t, tiles_img)
    ty, tx = divmod(rem, tiles_x)
    oy0, ox0 = 16 * ty, 16 * tx
    return (oy0, ox0, ((b * H + oy0) * W + ox0) * ps, ((b * H + oy0) * W + ox0) * pso,
            ((b * H + oy0) * W + ox0) * psr, ((b * 2 * H + oy0 * 2) * 2 * W + ox0 * 2) * ps1)


def test_tile_walk_by_steps_matches_the_division():
    ps, pso, psr, ps1 = 256, 272, 288, 144
    for N, H, W in ((5, 16, 16), (3, 16, 64), (3, 64, 16), (3, 48, 32), (2, 64, 64)):
        tiles_p = N * (H // 16) * (W // 16)
        # per-stream steps: 16 pixels right; on a row's end, down 16 rows and back to column 0
        orow, rrow = W * pso, W * psr
        dpss, dsrow = 2 * ps1, 2 * (2 * W) * ps1
        wrap_i, wrap_o, wrap_r, wrap_d = 15 * W * ps, 15 * orow, 16 * rrow - W * psr, 16 * dsrow - W * dpss
        for grid in (1, 2, 3, 5, 7, min(tiles_p, 256)):
            seen = []
            for w in range(grid):
                t0, t1 = w * tiles_p // grid, (w + 1) * tiles_p // grid
                if t0 >= t1:
                    continue
                oy0, ox0, base, obase, rbase, dbase = _decode(t0, H, W, ps, pso, psr, ps1)
                for t in range(t0, t1):
                    assert (oy0, ox0, base, obase, rbase, dbase) == _decode(t, H, W, ps, pso, psr, ps1)
                    seen.append(t)
                    n = [oy0, ox0 + 16, base + 16 * ps, obase + 16 * pso, rbase + 16 * psr, dbase + 16 * dpss]
                    if n[1] == W:
                        n[1] = 0
                        n[0] += 16
                        n[2] += wrap_i
                        n[3] += wrap_o
                        n[4] += wrap_r
                        n[5] += wrap_d
                        if n[0] == H:
                            n[0] = 0
                    # the next tile's pieces: the stepped origin, or at the range's end this tile's again
                    onext = n if t + 1 < t1 else [oy0, ox0, base, obase, rbase, dbase]
                    assert tuple(onext) == _decode(t + 1 if t + 1 < t1 else t, H, W, ps, pso, psr, ps1)
                    oy0, ox0, base, obase, rbase, dbase = n
            assert seen == list(range(tiles_p))
        # ranges begin and end mid-row and mid-image in these grids
    tiles_x, tiles_img, tiles_p = 2, 6, 18  # (3, 48, 32) on 7 workgroups
    starts = [w * tiles_p // 7 for w in range(7)]
    assert any(t % tiles_x for t in starts) and any(t % tiles_img for t in starts)


def test_hoisted_lane_constants_match_the_formulas_they_replace():
    W, pso = 48, 272
    for x3 in (False, True):
        for wave in range(NW):
            cw = (wave & 1) * 32 if x3 else wave * 32
            r0w = (wave >> 1) * 8 if x3 else 0
            TP = 8 if x3 else 16
            for ln in range(64):
                fr, fg = ln & 15, ln >> 4
                # fragment reads, both chunks
                for kx in range(3):
                    I2 = r0w * ROWB + (fr + kx) * 128 + ((fg ^ key(fr + kx)) << 4)
                    for c in range(2):
                        for h in range(2):
                            I2c = (I2 + c * PATCH) ^ (64 * h)
                            for j in range(TP):
                                for ky in range(3):
                                    old = (((fr + kx) * 128 + ((fg ^ key(fr + kx)) << 4)) ^ (h << 6)) + c * PATCH + \
                                        (r0w + j + ky) * ROWB
                                    assert I2c + (j + ky) * ROWB == old
                                    assert (j + ky) * ROWB < 1 << 16  # the read's immediate
                # bias, store offset
                for i in range(2):
                    assert SMEM_RES + (cw + fg * 4) * 4 + 64 * i == SMEM_RES + (cw + 16 * i + fg * 4) * 4
                    OV = ((r0w + (fg & 1)) * W + fr) * pso + ((64 * (cw >> 5) if x3 else cw) + (fg >> 1) * 8) * 2
                    for j in range(0, TP, 2):
                        px = (r0w + j + (fg & 1)) * W + fr
                        if x3:
                            pc = 64 * (cw >> 5) + 16 * i + (fg >> 1) * 8
                            assert OV + 32 * i + j * W * pso == px * pso + pc * 2
                            assert OV + 32 * i + 64 + j * W * pso == px * pso + (pc + 32) * 2
                        else:
                            co = cw + 16 * i + (fg >> 1) * 8
                            assert OV + 32 * i + j * W * pso == px * pso + co * 2
                # residual reads
                RB = OFF_RES + (r0w * 16 + fr) * 256 + ((((8 * (cw >> 5) if x3 else cw >> 3) + (fg >> 1)) ^ fr) << 4) + \
                    (fg & 1) * 8
                for i in range(2):
                    rbi = RB ^ 32 if i else RB
                    for j in range(TP):
                        assert j * 4096 + 8 < 1 << 16
                        pa = (r0w + j) * 16 + fr
                        if x3:
                            ch = 8 * (cw >> 5) + 2 * i + (fg >> 1)
                            rb = OFF_RES + pa * 256 + (fg & 1) * 8
                            assert rbi + j * 4096 == rb + ((ch ^ (pa & 15)) << 4)
                            assert (rbi ^ 64) + j * 4096 == rb + (((ch + 4) ^ (pa & 15)) << 4)
                        else:
                            ch = (cw >> 3) + 2 * i + (fg >> 1)
                            assert rbi + j * 4096 == OFF_RES + pa * 256 + ((ch ^ (pa & 15)) << 4) + (fg & 1) * 8
                # the downsample patch's fragments
                DD = OFF_RES + fr * 128 + ((fg ^ ((fr >> 1) & 7)) << 4)
                for h in range(2):
                    for j in range(16):
                        assert (DD ^ 64 if h else DD) + j * 16 * 128 == \
                            OFF_RES + fr * 128 + (((fg + 4 * h) ^ ((fr >> 1) & 7)) << 4) + j * 16 * 128
