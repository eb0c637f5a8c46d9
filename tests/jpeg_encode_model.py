"""TEST INFRASTRUCTURE: a vectorised numpy restatement of the baseline JPEG encoder that Pillow's default
`save(format='JPEG', quality=q)` runs (libjpeg-turbo: jccolor.c, jcsample.c h2v2_downsample, jfdctint.c, jcdctmgr.c
quantisation, jchuff.c, jcmarker.c), for RGB images whose sides are multiples of 16.  It is the specification the device
encoder (csrc/jpeg_enc.hip) is held to: `encode` returns the file's bytes and a census of what the entropy-coded stream
contains, `cases` is the case list the CPU and the GPU tests share.  All arithmetic is integer."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])
# Annex K.1 quantisation tables, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29,
                   51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121,
                   120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99,
                     99, 99, 99, 99, 99] + [99] * 32)
# Annex K.3 Huffman tables: (code counts per length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82,
            209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67,
            68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117,
            118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162,
            163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199,
            200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241,
            242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51,
              82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57,
              58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115,
              116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152,
              153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196,
              197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233,
              234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
HEADER_BYTES = 623


def quant_tables(quality):
    """jpeg_quality_scaling + jpeg_add_quant_table with force_baseline -> (luma, chroma) in natural order"""
    if not 1 <= quality <= 100:
        raise ValueError("quality %r" % (quality,))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int64) for t in (Q_LUMA, Q_CHROMA))


def header(H, W, quality):
    """everything in front of the entropy-coded data, as jcmarker.c writes it for Pillow's defaults"""
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)):
        out += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(v) for v in q[ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([H >> 8, H & 255, W >> 8, W & 255]) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        n = 19 + len(vals)
        out += b"\xff\xc4" + bytes([n >> 8, n & 255, tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def _derive(bits, vals):
    """jchuff.c jpeg_make_c_derived_tbl -> (code, length) per symbol, 256 entries each"""
    code = np.zeros(256, np.int64)
    size = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], size[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, size


def _fdct_1d(d, first):
    """one pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2) along the last axis of d [..., 8]"""
    def descale(x, n):
        return (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 11 if first else 15
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = descale(t10 + t11, 2), descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = descale(z1 + t13 * 6270, n)
    out[..., 6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = descale(t4 + z1 + z3, n)
    out[..., 5] = descale(t5 + z2 + z4, n)
    out[..., 3] = descale(t6 + z2 + z3, n)
    out[..., 1] = descale(t7 + z1 + z4, n)
    return out


def _blocks(plane):
    """[h, w] -> [h/8, w/8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def coefficients(rgb, quality):
    """rgb uint8 [H, W, 3] -> int16 [6 * MCUs, 64]: quantised coefficients in zigzag order, blocks in scan order
    (Y00 Y01 Y10 Y11 Cb Cr per MCU, MCUs row by row)"""
    rgb = np.asarray(rgb)
    H, W, _ = rgb.shape
    assert rgb.dtype == np.uint8 and H % 16 == 0 and W % 16 == 0
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2]), W // 4)[None, :]

    def down(p):
        return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    ql, qc = quant_tables(quality)

    def fdct_quant(plane, q):
        blk = _blocks(plane - 128)
        blk = _fdct_1d(blk, True)                                        # rows
        blk = _fdct_1d(blk.swapaxes(-1, -2), False).swapaxes(-1, -2)     # columns
        q8 = (q * 8).reshape(8, 8)
        mag = (np.abs(blk) + (q8 >> 1)) // q8
        return (np.sign(blk) * mag).reshape(blk.shape[0], blk.shape[1], 64)[..., ZIGZAG]
    yb, cbb, crb = fdct_quant(y, ql), fdct_quant(down(cb), qc), fdct_quant(down(cr), qc)
    my, mx = H // 16, W // 16
    out = np.empty((my, mx, 6, 64), np.int64)
    for j in range(4):
        out[:, :, j] = yb[j // 2::2, j % 2::2]
    out[:, :, 4], out[:, :, 5] = cbb, crb
    return out.reshape(-1, 64).astype(np.int16)


def _category(v):
    a = np.abs(v)
    cat = np.zeros(a.shape, np.int64)
    for k in range(16):
        cat += (a >> k) > 0
    return cat


def entropy(coef):
    """coef int16 [6 * MCUs, 64] (zigzag, scan order) -> (stuffed scan bytes, census)"""
    coef = np.asarray(coef).astype(np.int64)
    nb = coef.shape[0]
    comp = np.where(np.arange(nb) % 6 < 4, 0, np.arange(nb) % 6 - 3)     # 0 Y, 1 Cb, 2 Cr
    chroma = comp > 0
    dc = coef[:, 0]
    diff = dc.copy()
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        diff[idx[1:]] = dc[idx[1:]] - dc[idx[:-1]]
    tabs = {False: (_derive(*DC_LUMA), _derive(*AC_LUMA)), True: (_derive(*DC_CHROMA), _derive(*AC_CHROMA))}
    dc_code = np.stack([tabs[False][0][0], tabs[True][0][0]])
    dc_size = np.stack([tabs[False][0][1], tabs[True][0][1]])
    ac_code = np.stack([tabs[False][1][0], tabs[True][1][0]])
    ac_size = np.stack([tabs[False][1][1], tabs[True][1][1]])
    ci = chroma.astype(np.int64)

    def value_bits(v, cat):
        return np.where(v < 0, v + (1 << cat) - 1, v)
    # tokens: (block, order within block, bits, length); order = 4 * k + slot keeps the stream order after a sort
    dcat = _category(diff)
    toks = [(np.arange(nb), np.zeros(nb, np.int64), (dc_code[ci, dcat] << dcat) | value_bits(diff, dcat), dc_size[ci, dcat] + dcat)]
    ac = coef[:, 1:]
    bi, ki = np.nonzero(ac)                                               # row-major: block, then position
    ki = ki + 1
    first = np.concatenate(([True], bi[1:] != bi[:-1])) if bi.size else np.zeros(0, bool)
    prev = np.where(first, 0, np.concatenate(([0], ki[:-1])))
    run = ki - prev - 1
    v = coef[bi, ki]
    cat = _category(v)
    sym = ((run & 15) << 4) | cat
    cb_ = ci[bi]
    toks.append((bi, 4 * ki + 3, (ac_code[cb_, sym] << cat) | value_bits(v, cat), ac_size[cb_, sym] + cat))
    for z in range(3):                                                    # up to three ZRLs in front of a coefficient
        m = (run >> 4) > z
        toks.append((bi[m], 4 * ki[m] + z, ac_code[cb_[m], 0xF0], ac_size[cb_[m], 0xF0]))
    last = np.zeros(nb, np.int64)
    last[bi] = ki                                                         # ascending within a block: the last one stays
    eob = last < 63
    toks.append((np.nonzero(eob)[0], np.full(int(eob.sum()), 4 * 64, np.int64), ac_code[ci[eob], 0], ac_size[ci[eob], 0]))
    tb, to, tv, tl = (np.concatenate([t[i] for t in toks]) for i in range(4))
    order = np.lexsort((to, tb))
    tv, tl = tv[order], tl[order]
    ends = np.cumsum(tl)
    total = int(ends[-1])
    pad = (8 - total % 8) % 8
    which = np.repeat(np.arange(tl.size), tl)
    shift = ends[which] - 1 - np.arange(total)
    bits = np.concatenate((((tv[which] >> shift) & 1).astype(np.uint8), np.ones(pad, np.uint8)))
    raw = np.packbits(bits)
    ff = raw == 0xFF
    pos = np.arange(raw.size) + np.concatenate(([0], np.cumsum(ff)[:-1]))
    out = np.zeros(raw.size + int(ff.sum()), np.uint8)
    out[pos] = raw
    census = {"zrl": int(sum(t[0].size for t in toks[2:5])), "no_eob": int((~eob).sum()),
              "eob_only": int((last == 0).sum()), "dc_cats": set(int(c) for c in np.unique(dcat)),
              "ac_cats": set(int(c) for c in np.unique(cat)), "stuffed": int(ff.sum()), "pad_bits": pad,
              "last_byte_ff_padded": bool(pad > 0 and raw[-1] == 0xFF), "blocks": nb}
    return out.tobytes(), census


def encode(rgb, quality=75):
    """rgb uint8 [H, W, 3] -> (the bytes of Pillow's `save(format='JPEG', quality=quality)`, census of the scan)"""
    rgb = np.asarray(rgb)
    scan, census = entropy(coefficients(rgb, quality))
    return header(rgb.shape[0], rgb.shape[1], quality) + scan + b"\xff\xd9", census


def to_bytes_host(x):
    """the host loop's conversion of a [-1, 1] fp32 image [3, H, W] -> uint8 [H, W, 3]: add(1), div(2), mul(255),
    clamp(0, 255), truncation, each its own fp32 operation"""
    x = np.asarray(x, np.float32)
    v = np.clip((x + np.float32(1)) / np.float32(2) * np.float32(255), np.float32(0), np.float32(255))
    return np.ascontiguousarray(v.astype(np.uint8).transpose(1, 2, 0))


def pillow(rgb, quality=75):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


# ---- the case list ---------------------------------------------------------------------------------------------
SIZES = ((16, 16), (16, 32), (48, 16), (64, 64))
QUALITIES = (75, 1, 30, 95, 100)


def _content(kind, H, W, rng):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "smooth":
        f = np.stack([128 + 100 * np.sin(xx / 9.0 + 0.3) * np.cos(yy / 7.0), 128 + 90 * np.cos((xx + yy) / 11.0),
                      (xx * 3 + yy * 2) % 256 * 0.5 + 60], -1)
        return np.clip(f, 0, 255).astype(np.uint8)
    if kind == "constant":
        return np.broadcast_to(np.array([37, 141, 213], np.uint8), (H, W, 3)).copy()
    if kind == "zeros":
        return np.zeros((H, W, 3), np.uint8)
    if kind == "ones":
        return np.full((H, W, 3), 255, np.uint8)
    if kind == "primaries":
        pal = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [0, 0, 0],
                        [255, 255, 255]], np.uint8)
        return pal[((xx // 5) + (yy // 3)) % 8]
    if kind == "basis":                                                  # one high-frequency basis pattern: long zero runs
        g = 128 + 120 * np.cos((2 * (xx % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (yy % 8) + 1) * 6 * np.pi / 16)
        return np.repeat(np.clip(np.rint(g), 0, 255).astype(np.uint8)[..., None], 3, -1)
    if kind == "extremes":                                               # 0 / 255 noise per 8 x 8 block and per pixel
        coarse = rng.integers(0, 2, (H // 8, W // 8, 1), dtype=np.uint8).repeat(8, 0).repeat(8, 1) * 255
        fine = rng.integers(0, 2, (H, W, 1), dtype=np.uint8) * 255
        return np.repeat(np.where((yy // 8 % 2 == 0)[..., None], coarse, fine).astype(np.uint8), 3, -1)
    if kind == "stripes":
        return np.repeat(((xx % 2) * 255).astype(np.uint8)[..., None], 3, -1)
    raise ValueError(kind)


CONTENTS = ("noise", "smooth", "constant", "zeros", "ones", "primaries", "basis", "extremes", "stripes")


def cases(big=False):
    """[(name, rgb uint8 [H, W, 3], quality)]: every size x quality x content; big adds one 256 x 256 per quality"""
    out = []
    for si, (H, W) in enumerate(SIZES + (((256, 256),) if big else ())):
        for q in QUALITIES:
            kinds = CONTENTS if H < 256 else (("noise", "smooth", "extremes", "primaries", "basis")[QUALITIES.index(q)],)
            for ki, kind in enumerate(kinds):
                rng = np.random.default_rng(1000 * si + 10 * q + ki)
                out.append(("%dx%d_q%d_%s" % (H, W, q, kind), _content(kind, H, W, rng), q))
    return out
