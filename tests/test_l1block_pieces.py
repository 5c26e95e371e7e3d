"""CPU: the fused layer1 block's patch-piece table, tile walk and hoisted lane
constants (csrc/l1block.hip, variant 40), restated from the kernel's formulas
and checked exhaustively.

* piece table: entry (wave, k, lane) = edge bits << 28 | source offset / 16
  from the tile's first patch pixel; a piece's source is masked to zeros where
  entry & the tile's edge mask is non-zero.  For every tile position class the
  50 pieces of a strip-start tile write every 16-B chunk of the 20 x 20 patch
  exactly once, from the source chunk the readers expect there, and zeros
  exactly where the pixel lies outside the image;
* a continuation tile: the pieces that remain are exactly patch rows 4-19,
  the skipped ones are each wave's first pieces, and the LDS copy of the
  previous patch's rows 18, 19 covers rows 2, 3 exactly once;
* no table access passes the LDS budget; an entry's offset fits its 28 bits;
* the tile walk by steps visits the tiles that the division decodes;
* the lane constants kept in registers give the read addresses that
  tests/test_l1block_layout.py checks for conflicts (its conv1_addr), in both
  patch buffers.
"""
import test_l1block_layout as lay

NW, QP, NDP, QSKIP = 4, 13, 50, 10
PWD, PROW, IROW = lay.PWD, lay.PROW, lay.IROW
PATCH = 400 * 128
OFF_I = 2 * PATCH
OFF_B = OFF_I + 18 * IROW
OFF_T = OFF_B + 512
SMEM = OFF_T + NW * QP * 256
LDS_BYTES = 160 * 1024
BAD = 0x7FFFFFF0
key = lay.key


def entry(wave, k, lane, W):
    r = 8 * (wave + NW * k) + (lane >> 3)
    Y = (r * 205) >> 12
    X = r - 20 * Y
    c = (lane & 7) ^ key(X) ^ ((Y & 3) << 1)
    edge = (1 if Y < 2 else 0) | (2 if Y >= PWD - 2 else 0) | (4 if X < 2 else 0) | (8 if X >= PWD - 2 else 0)
    return ((edge << 28) | ((Y * W + X) * 8 + c)) & 0xFFFFFFFF


def patch_mask(oy0, ox0, H, W):
    return (((1 if oy0 == 0 else 0) | (2 if oy0 + 16 == H else 0) | (4 if ox0 == 0 else 0) |
             (8 if ox0 + 16 == W else 0)) << 28)


def piece_voff(e, pbase, pmask):
    return BAD if e & pmask else (pbase + ((e << 4) & 0xFFFFFFFF)) & 0xFFFFFFFF


def wave_pieces(wave, cont):
    """the k this wave issues (the kernel's uniform test)"""
    return [k for k in range(QP) if wave + NW * k < NDP and not (cont and wave + NW * k < QSKIP)]


def test_table_fits_the_lds_budget():
    assert SMEM <= LDS_BYTES
    last = 0
    for wave in range(NW):
        for k in range(QP):  # the loop reads entry k + 1 while it issues piece k: k + 1 <= QP - 1
            for lane in range(64):
                ad = OFF_T + (wave * QP * 64 + 64 * k + lane) * 4
                assert OFF_T <= ad and ad + 4 <= SMEM
                last = max(last, ad + 4)
    assert last == SMEM
    # 16-B units of the largest offset in 28 bits, for every W a launch can have
    # (an image range stays under 2^31 bytes and H >= 16)
    Wmax = (1 << 31) // (16 * 128)
    assert (19 * Wmax + 19) * 8 + 7 < 1 << 28


def _tile_classes():
    # (H, W, oy0, ox0): every combination of shared edges, 16 x 16 included
    out = []
    for H, W in ((16, 16), (16, 48), (48, 16), (48, 64), (32, 32)):
        for oy0 in range(0, H, 16):
            for ox0 in range(0, W, 16):
                out.append((H, W, oy0, ox0))
    return out


def test_strip_start_tile_writes_every_chunk_once_and_right():
    seen_masks = set()
    for H, W, oy0, ox0 in _tile_classes():
        b = 1  # second image of a batch: the base is non-zero
        base = ((b * H + oy0) * W + ox0) * 128
        pbase = base - (2 * W + 2) * 128
        pmask = patch_mask(oy0, ox0, H, W)
        seen_masks.add(pmask >> 28)
        written = {}
        for wave in range(NW):
            for k in wave_pieces(wave, False):
                q = wave + NW * k
                for lane in range(64):
                    dst = q * 1024 + lane * 16
                    assert dst not in written
                    written[dst] = piece_voff(entry(wave, k, lane, W), pbase, pmask)
        assert sorted(written) == list(range(0, PATCH, 16))
        for dst, voff in written.items():
            slot, pos = dst // 128, (dst % 128) // 16
            Y, X = divmod(slot, PWD)
            iy, ix = oy0 - 2 + Y, ox0 - 2 + X
            c = pos ^ key(X) ^ ((Y & 3) << 1)
            assert lay.patch_pos(Y, X, c) == pos
            if 0 <= iy < H and 0 <= ix < W:
                assert voff == ((b * H + iy) * W + ix) * 128 + c * 16
            else:
                assert voff == BAD
    assert seen_masks == set(range(16))  # every edge combination


def test_continuation_tile_rows():
    for wave in range(NW):
        full, cont = wave_pieces(wave, False), wave_pieces(wave, True)
        # the skipped pieces are the wave's first ones: the trip start decides
        assert cont == full[len(full) - len(cont):]
    slots = set()
    for wave in range(NW):
        for k in wave_pieces(wave, True):
            q = wave + NW * k
            for lane in range(64):
                s = 8 * q + (lane >> 3)
                slots.add(s)
    assert slots == set(range(4 * PWD, 20 * PWD))  # rows 4-19 by DMA
    assert sum(len(wave_pieces(w, True)) for w in range(NW)) == 40
    # rows 2, 3 by the copy: 320 chunks from row 18 of this patch to row 2 of the next
    dst = {}
    for tid in range(256):
        for i in (tid, min(tid + 256, 319)):
            src = 360 * 128 + i * 16
            d = 40 * 128 + i * 16
            assert dst.setdefault(d, src) == src  # the clamped lanes repeat chunk 319
    assert sorted(dst) == list(range(2 * PROW, 4 * PROW, 16))
    for d, src in dst.items():
        assert src - 18 * PROW == d - 2 * PROW


def test_tile_walk_by_steps_matches_the_division():
    for N, H, W in ((3, 16, 64), (2, 256, 16), (3, 48, 32), (2, 128, 128), (5, 16, 16)):
        ty_n, tx_n = H // 16, W // 16
        row_b, img_b = W * 128, H * W * 128
        for t0 in (0, 1, ty_n - 1, ty_n, ty_n * tx_n - 1):
            b, rem = divmod(t0, ty_n * tx_n)
            tx, ty = divmod(rem, ty_n)
            oy0, ox0, base = ty * 16, tx * 16, ((b * H + ty * 16) * W + tx * 16) * 128
            for t in range(t0 + 1, N * ty_n * tx_n):
                oy0 += 16
                base += 16 * row_b
                if oy0 == H:
                    oy0 = 0
                    ox0 += 16
                    base += 16 * 128 - img_b
                    if ox0 == W:
                        ox0 = 0
                        base += img_b - row_b
                b, rem = divmod(t, ty_n * tx_n)
                tx, ty = divmod(rem, ty_n)
                assert (oy0, ox0, base) == (ty * 16, tx * 16, ((b * H + ty * 16) * W + tx * 16) * 128)


def test_hoisted_read_addresses_match_the_layout():
    """LAp / L9 (conv1), LRr (residual), I2 (conv2) as the kernel keeps them in
    registers (LDS base 0), in patch buffer pb"""
    for pb in range(2):
        pbo = pb * PATCH
        for pg in range(2):
            for ln in range(64):
                fr, fg = ln & 15, ln >> 4
                e01, LY = fr & 1, 2 + 8 * pg + (fr >> 1)
                for ky in range(3):
                    for kx in range(3):
                        LAp = pbo + (2 + 8 * pg) * PROW + (fr + kx) * 128 + ((fg ^ key(fr + kx)) << 4)
                        L9 = pbo + ((LY + ky) * PWD + 16 + e01 + kx) * 128 + \
                            ((fg ^ key(16 + e01 + kx) ^ (((LY + ky) & 3) << 1)) << 4)
                        for h in range(2):
                            for k in range(8):
                                sg = (((2 + k + ky) & 3) << 5) ^ (h << 6)
                                assert (LAp ^ sg) + (k + ky) * PROW == pbo + lay.conv1_addr(pg, k, ln, ky, kx, h)
                            assert (L9 ^ 64 if h else L9) == pbo + lay.conv1_addr(pg, 8, ln, ky, kx, h)
                            # the strip-start prefix row pg, from LAp
                            Y = pg + ky
                            assert (LAp ^ (((Y & 3) << 5) ^ (h << 6))) + (Y - 2 - 8 * pg) * PROW == \
                                pbo + lay.conv1_addr(pg, 'PA', ln, ky, kx, h)
                for cg in range(2):
                    cw = 32 * cg
                    for i in range(2):
                        LRr = pbo + pg * 8 * PROW + (fr + 2) * 128 + \
                            ((((cw >> 3) + 2 * i + (fg >> 1)) ^ key(fr + 2)) << 4) + (fg & 1) * 8
                        for jj in range(8):
                            Y, X, co = 8 * pg + jj + 2, fr + 2, cw + 16 * i + 4 * fg
                            assert (LRr ^ (((jj + 2) & 3) << 5)) + (jj + 2) * PROW == \
                                pbo + (Y * PWD + X) * 128 + (lay.patch_pos(Y, X, co >> 3) << 4) + (co & 7) * 2
                        # conv1's store addresses: aligned fragment k, leftover
                        pa = (((cw >> 3) + (fg >> 1)) ^ key(fr)) * 16 + (fg & 1) * 8
                        pl = (((cw >> 3) + (fg >> 1)) ^ key(16 + e01)) * 16 + (fg & 1) * 8
                        co = cw + 16 * i + 4 * fg
                        for k in range(8):
                            y, x = lay.conv1_fragment(pg, k, ln)
                            E1A = OFF_I + (2 + 8 * pg) * IROW + fr * 128 + (pa ^ 32 if i else pa)
                            assert E1A + k * IROW == OFF_I + y * IROW + x * 128 + (((co >> 3) ^ key(x)) << 4) + (co & 7) * 2
                        y, x = lay.conv1_fragment(pg, 8, ln)
                        E1L = OFF_I + LY * IROW + (16 + e01) * 128 + (pl ^ 32 if i else pl)
                        assert E1L == OFF_I + y * IROW + x * 128 + (((co >> 3) ^ key(x)) << 4) + (co & 7) * 2
