"""Python model of range decode over a framed stream: the seek
table, the span and unit rule of csrc/snappy_frame_ranges.h, the header stage's
verdict, and a range's status, all over frame_model's strict walk.  It knows
nothing of the library."""
import struct

import frame_model as fm

CH = 65536
U64 = (1 << 64) - 1
OK, ERR_ARG, ERR_HEADER, ERR_TRUNCATED, ERR_OFFSET, ERR_OVERRUN, ERR_CAPACITY = 0, -1, -2, -3, -4, -5, -6
ERR_UNSUPPORTED, ERR_INDEX, ERR_CHECKSUM = -9, -11, -12
BAD = 0xFFFFFFFF  # hi of a unit the tables contradict themselves about


def chunk_info(stream, pos, end=None):
    """(status, kind, len field, decoded bytes) of the chunk at pos by the format's
    rules for a data chunk (frame_model.chunk_table's, without the identifier), the
    stream ending at `end`; status 0 = a data chunk, 1 = a chunk that holds no data"""
    n = len(stream) if end is None else end
    if n - pos < 4:
        return ERR_TRUNCATED, 0, 0, 0
    kind = stream[pos]
    ln = stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16
    if kind == 0xFF:
        if ln != 6:
            return ERR_HEADER, kind, ln, 0
        if n - pos < 10:
            return ERR_TRUNCATED, kind, ln, 0
        return (1 if stream[pos:pos + 10] == fm.IDENTIFIER else ERR_HEADER), kind, ln, 0
    if 0x02 <= kind <= 0x7F:
        return ERR_UNSUPPORTED, kind, ln, 0
    if kind >= 0x80:
        return (ERR_TRUNCATED if n - pos - 4 < ln else 1), kind, ln, 0
    if ln < 4:
        return ERR_HEADER, kind, ln, 0
    if n - pos - 4 < ln:
        return ERR_TRUNCATED, kind, ln, 0
    d = ln - 4
    if kind == 0x00:
        d, shift, done = 0, 0, False
        for b in stream[pos + 8:pos + 8 + min(ln - 4, 5)]:
            d |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                done = True
                break
        if not done:
            return ERR_HEADER, kind, ln, 0
    if d > CH:
        return ERR_OVERRUN, kind, ln, 0
    return OK, kind, ln, d


def seek_table(stream, table=None):
    """(status, starts): starts[i] = the decoded position of data chunk i, then the
    decoded length; the first failing table entry's status, as the framed decode
    gives it (an entry past the stream ERR_TRUNCATED, no data chunk ERR_INDEX)"""
    if table is None:
        st, table, _ = fm.chunk_table(stream)
        assert st == fm.OK
    starts, total = [], 0
    for pos in table[:-1]:
        if pos >= len(stream):
            return ERR_TRUNCATED, None
        st, kind, ln, d = chunk_info(stream, pos)
        if st == 1:
            return ERR_INDEX, None
        if st != OK:
            return st, None
        if kind == 0x00 and d == 0:
            used = next(k + 1 for k, b in enumerate(stream[pos + 8:pos + 13]) if not b & 0x80)
            if used != ln - 4:  # elements behind an empty chunk's preamble overrun it
                return ERR_OVERRUN, None
        starts.append(total)
        total += d
    return OK, starts + [total]


def seek(starts, nchunks, pos):
    """the last i in [0, nchunks) with starts[i] <= pos, by the header's binary search"""
    lo, hi = 0, nchunks - 1
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if starts[mid] <= pos:
            lo = mid
        else:
            hi = mid - 1
    return lo


def span(starts, rng, out_bytes):
    """(status, u0, u1, units)"""
    start, length, oo = rng
    nchunks = len(starts) - 1
    s0, s1 = starts[0], starts[nchunks]
    if start < s0 or start > s1 or length > s1 - start:
        return ERR_ARG, 0, 0, 0
    if oo > out_bytes or length > out_bytes - oo:
        return ERR_CAPACITY, 0, 0, 0
    if length == 0:
        return OK, 0, 0, 0
    u0, u1 = seek(starts, nchunks, start), seek(starts, nchunks, start + length - 1)
    if u1 < u0:
        return ERR_INDEX, u0, u1, 0
    return OK, u0, u1, u1 - u0 + 1


def unit(starts, rng, i, u0, u1, u):
    """((unit, land, range, lo, hi), is_edge)"""
    start, length, oo = rng
    b0, size, end = starts[u], (starts[u + 1] - starts[u]) & U64, start + length
    first, last = u == u0, u == u1
    land = (oo + b0 - start) & U64
    bad = (u, land, i, 0, BAD), False
    if size > CH:
        return bad
    if size == 0:
        return ((u, land, i, 0, 0), False) if not first and not last else bad
    if not first and b0 < start:
        return bad
    if not last and (b0 > end - 1 or end - b0 < size):
        return bad
    lo, hi = (start - b0 if first else 0), (end - b0 if last else size)
    if lo >= hi or hi > size:
        return bad
    return (u, land, i, lo, hi), (lo != 0 or hi != size)


def plan(starts, ranges, out_bytes):
    """-> (statuses, units): units = [(unit, land mod 2^64, range, lo, hi, edge)],
    edge = 0 or the 1-based count of edge units so far"""
    statuses, units, edges = [], [], 0
    for i, rng in enumerate(ranges):
        st, u0, u1, k = span(starts, rng, out_bytes)
        statuses.append(st)
        for u in range(u0, u0 + k):
            e, is_edge = unit(starts, rng, i, u0, u1, u)
            edge = 0
            if is_edge:
                edges += 1
                edge = edges
            units.append(e + (edge,))
    return statuses, units


def unit_check(stream, chunks, starts, u, hi, w0, w1):
    """the header stage's verdict on table entry u seen through the window [w0, w1)"""
    pos, nxt, size = chunks[u], chunks[u + 1], (starts[u + 1] - starts[u]) & U64
    if pos < w0 or pos >= w1:
        return ERR_TRUNCATED
    st, kind, ln, d = chunk_info(stream, pos, w1)
    if st < 0:
        return st
    if st == 1 or d != size:
        return ERR_INDEX
    if nxt < pos or 4 + ln > nxt - pos:
        return ERR_INDEX
    if hi > d:
        return ERR_INDEX
    return OK


def chunk_decode_status(stream, pos, decompress_status):
    """element or CRC status of the data chunk at pos: decompress_status(payload) ->
    (status, raw bytes) for a compressed chunk"""
    ln = stream[pos + 1] | stream[pos + 2] << 8 | stream[pos + 3] << 16
    crc, = struct.unpack_from("<I", stream, pos + 4)
    body = bytes(stream[pos + 8:pos + 4 + ln])
    if stream[pos] == 0x01:
        st, raw = OK, body
    else:
        st, raw = decompress_status(body)
    if st != OK:
        return st, None
    return (OK if fm.mask(fm.crc32c(raw)) == crc else ERR_CHECKSUM), raw


def range_status(stream, chunks, starts, rng, out_bytes, decompress_status, w0=0, w1=None):
    """(status, early): the range's status by the rule of DESIGN.md 7.7; early = it
    was refused before any decode (nothing of it is stored)"""
    w1 = len(stream) if w1 is None else w1
    st, u0, u1, k = span(starts, rng, out_bytes)
    if st != OK:
        return st, True
    us = [unit(starts, rng, 0, u0, u1, u)[0] for u in range(u0, u0 + k)]
    for e in us:
        if e[4] == 0:
            continue
        st = unit_check(stream, chunks, starts, e[0], e[4], w0, w1)
        if st != OK:
            return st, True
    for e in us:
        if e[4] == 0:
            continue
        st, _ = chunk_decode_status(stream, chunks[e[0]], decompress_status)
        if st != OK:
            return st, False
    return OK, False
