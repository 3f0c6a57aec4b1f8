"""A small baseline JPEG WRITER for tests: a stream from explicit quantised coefficient blocks, quantisation tables, sampling
factors, restart interval and extra segments, so that the edge streams (ZRL runs, 16-bit codes, category-11 DC differences, stuffed
bytes, fill bytes before RSTn, ...) depend on no encoder's choices.  Huffman tables are built here from the symbols the blocks
need, with the code lengths the caller asks for.  Test infrastructure only."""
import struct

import numpy as np

from jpeg_oracle import ZIGZAG


def segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def jfif():
    return segment(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")


def adobe(transform):
    return segment(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([transform]))


def exif(orientation, little_endian=True, extra_entries=0):
    """An APP1 Exif segment whose IFD0 holds ``extra_entries`` other tags and then the orientation"""
    e = "<" if little_endian else ">"
    entries = b"".join(struct.pack(e + "HHIHH", 0x0100 + i, 3, 1, 7, 0) for i in range(extra_entries))
    entries += struct.pack(e + "HHIHH", 0x0112, 3, 1, orientation, 0)
    tiff = (b"II" if little_endian else b"MM") + struct.pack(e + "HI", 42, 8) + struct.pack(e + "H", extra_entries + 1) + entries + struct.pack(e + "I", 0)
    return segment(0xE1, b"Exif\0\0" + tiff)


def dqt(tables, sixteen=False):
    """One DQT segment holding every table of ``{index: 64 natural-order values}``"""
    out = b""
    for tq, q in tables.items():
        z = np.asarray(q).reshape(64)[ZIGZAG]
        out += bytes([(16 if sixteen else 0) | tq]) + (z.astype(">u2").tobytes() if sixteen else z.astype(np.uint8).tobytes())
    return segment(0xDB, out)


def canonical(lengths):
    """``{symbol: code length}`` -> ``(bits[16], values, {symbol: (length, code)})`` in canonical order (by length, then as given)"""
    order = sorted(lengths, key=lambda s: lengths[s])  # stable
    bits, codes, code, prev = [0] * 16, {}, 0, 0
    for s in order:
        code <<= lengths[s] - prev
        prev = lengths[s]
        codes[s] = (prev, code)
        bits[prev - 1] += 1
        code += 1
        assert code < (1 << prev), "code lengths do not fit a prefix code that leaves the all-ones code unused"
    return bits, order, codes


def dht(tables):
    """One DHT segment holding every table of ``{(class, index): (bits, values)}``"""
    return segment(0xC4, b"".join(bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals) for (tc, th), (bits, vals) in tables.items()))


def _category(v):
    return int(abs(int(v))).bit_length()


def _block_symbols(blk, pred):
    """The (symbol, extra bits value, extra bit count) list of one block in zig-zag order: DC first"""
    z = [int(v) for v in np.asarray(blk).reshape(64)[ZIGZAG]]
    diff = z[0] - pred
    t = _category(diff)
    assert t <= 15, f"a DC difference of {diff} needs category {t}: decoders refuse it (give the DC values unwrapped, in a wide integer type)"
    out = [("dc", t, diff if diff >= 0 else diff + (1 << t) - 1, t)]
    run = 0
    last = max([i for i in range(1, 64) if z[i]], default=0)
    for i in range(1, last + 1):
        if z[i] == 0:
            run += 1
            continue
        while run > 15:
            out.append(("ac", 0xF0, 0, 0))
            run -= 16
        t = _category(z[i])
        out.append(("ac", (run << 4) | t, z[i] if z[i] >= 0 else z[i] + (1 << t) - 1, t))
        run = 0
    if last < 63:
        out.append(("ac", 0x00, 0, 0))
    return out, z[0]


def write_jpeg(width, height, comps, blocks, qtables, dri=0, segments=(), sof=0xC0, dqt16=False, fill_before_rst=0, dc_lengths=None, ac_lengths=None, tail=b"\xff\xd9",
               split_tables=False):
    """``comps``: ``[(id, h, v, tq, td, ta)]``; ``blocks``: per component a (bh, bw, 64) array of quantised coefficients in natural
    order over the component's whole block grid; ``qtables``: ``{index: 64 natural-order values}``; ``segments``: bytes placed
    after SOI.  ``dc_lengths`` / ``ac_lengths``: ``{table index: {symbol: code length}}`` to force code lengths (symbols the blocks
    do not use may be listed); the default gives every used symbol the same length.  Returns the stream's bytes."""
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:
        hmax = vmax = 1
    mcux, mcuy = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    # symbols per MCU, in coding order
    mcus, pred = [], [0] * len(comps)
    for k in range(mcux * mcuy):
        if dri and k % dri == 0:
            pred = [0] * len(comps)
        my, mx = divmod(k, mcux)
        syms = []
        for ci, (_id, h, v, _tq, td, ta) in enumerate(comps):
            if len(comps) == 1:
                h = v = 1
            for by in range(v):
                for bx in range(h):
                    out, pred[ci] = _block_symbols(blocks[ci][my * v + by, mx * h + bx], pred[ci])
                    syms += [((0, td) if kind == "dc" else (1, ta), sym, val, n) for kind, sym, val, n in out]
        mcus.append(syms)
    # tables
    used = {}
    for syms in mcus:
        for key, sym, _val, _n in syms:
            used.setdefault(key, {})[sym] = True
    tables, codes = {}, {}
    for key, symbols in used.items():
        forced = ((dc_lengths if key[0] == 0 else ac_lengths) or {}).get(key[1])
        if forced is None:
            n = max(1, len(symbols).bit_length())  # 2^n >= len + 1: the all-ones code stays unused
            forced = {s: n for s in sorted(symbols)}
        assert all(s in forced for s in symbols), "a used symbol has no code length"
        bits, vals, codes[key] = canonical(forced)
        tables[key] = (bits, vals)
    # entropy-coded data
    body, rst = b"", 0
    per = dri if dri else len(mcus)
    for first in range(0, len(mcus), per):
        bits = []
        for syms in mcus[first : first + per]:
            for key, sym, val, n in syms:
                length, code = codes[key][sym]
                bits.append(format(code, f"0{length}b"))
                if n:
                    bits.append(format(val, f"0{n}b"))
        text = "".join(bits)
        text += "1" * (-len(text) % 8)
        raw = int(text, 2).to_bytes(len(text) // 8, "big") if text else b""
        body += raw.replace(b"\xff", b"\xff\x00")
        if first + per < len(mcus):
            body += b"\xff" * fill_before_rst + bytes([0xFF, 0xD0 + rst])
            rst = (rst + 1) & 7
    head = b"\xff\xd8" + b"".join(segments) + dqt(qtables, dqt16)
    head += segment(sof, struct.pack(">BHHB", 8, height, width, len(comps)) + b"".join(bytes([c[0], (c[1] << 4) | c[2], c[3]]) for c in comps))
    head += b"".join(dht({k: t}) for k, t in tables.items()) if split_tables else dht(tables)
    if dri:
        head += segment(0xDD, struct.pack(">H", dri))
    head += segment(0xDA, bytes([len(comps)]) + b"".join(bytes([c[0], (c[4] << 4) | c[5]]) for c in comps) + b"\x00\x3f\x00")
    return head + body + tail


def grid(width, height, comps, ci):
    """(bh, bw) of component ``ci``'s whole block grid"""
    if len(comps) == 1:
        return -(-height // 8), -(-width // 8)
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    return -(-height // (8 * vmax)) * comps[ci][2], -(-width // (8 * hmax)) * comps[ci][1]


GRAY = [(1, 1, 1, 0, 0, 0)]
YCC444 = [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
YCC422 = [(1, 2, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
YCC420 = [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]


def random_blocks(rng, width, height, comps, amplitude=40, density=0.15):
    """Sparse random quantised blocks for every component"""
    out = []
    for ci in range(len(comps)):
        bh, bw = grid(width, height, comps, ci)
        b = (rng.integers(-amplitude, amplitude + 1, (bh, bw, 64)) * (rng.random((bh, bw, 64)) < density)).astype(np.int16)
        b[:, :, 0] = rng.integers(-60, 61, (bh, bw))
        out.append(b)
    return out
