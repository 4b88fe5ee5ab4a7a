"""Python model of range decode over a Hadoop or snappy-java container (DESIGN.md
7.8): the span and unit rule of csrc/snappy_container_ranges.h over the chunk
tables of container_model.walk, the packing of edge chunks into the staging area,
the table stage's verdict, and a range's status.  It knows nothing of the library.

Tables are lists of pairs: comp = [(payload offset, comp_len)], outp = [(decoded
offset, length)], as container_model.walk gives them."""
import container_model as cm

BLOCK = 65536
CHUNK_MAX = 1 << 30
U64 = (1 << 64) - 1
OK, ERR_ARG, ERR_HEADER, ERR_TRUNCATED, ERR_OFFSET, ERR_OVERRUN, ERR_CAPACITY = 0, -1, -2, -3, -4, -5, -6
ERR_UNSUPPORTED, ERR_INDEX = -9, -11
BAD = 0xFFFFFFFF  # hi of a unit the tables contradict themselves about


def tables(stream, fmt):
    """(comp, outp, decoded bytes) of a well-formed container, by the model's walk"""
    st, comp, outp, total = cm.walk(stream, fmt)
    assert st == cm.OK
    return comp, outp, total


def seek(outp, pos):
    """the last i with outp[i][0] <= pos, by the header's binary search"""
    lo, hi = 0, len(outp) - 1
    while lo < hi:
        mid = lo + (hi - lo + 1) // 2
        if outp[mid][0] <= pos:
            lo = mid
        else:
            hi = mid - 1
    return lo


def span(outp, rng, out_bytes):
    """(status, u0, u1, units)"""
    start, length, oo = rng
    if not outp:
        if length:
            return ERR_ARG, 0, 0, 0
    else:
        s0, s1 = outp[0][0], (outp[-1][0] + outp[-1][1]) & U64
        if start < s0 or start > s1 or length > s1 - start:
            return ERR_ARG, 0, 0, 0
    if oo > out_bytes or length > out_bytes - oo:
        return ERR_CAPACITY, 0, 0, 0
    if length == 0:
        return OK, 0, 0, 0
    u0, u1 = seek(outp, start), seek(outp, start + length - 1)
    if u1 < u0:
        return ERR_INDEX, u0, u1, 0
    return OK, u0, u1, u1 - u0 + 1


def unit(outp, rng, i, u0, u1, u):
    """((unit, land, range, lo, hi), is_edge)"""
    start, length, oo = rng
    b0, size = outp[u]
    end = start + length
    first, last = u == u0, u == u1
    land = (oo + b0 - start) & U64
    bad = (u, land, i, 0, BAD), False
    if size > CHUNK_MAX:
        return bad
    if size == 0:
        return ((u, land, i, 0, 0), False) if not first and not last and outp[u + 1][0] == b0 else bad
    if not first and b0 < start:
        return bad
    if not last and (b0 > end - 1 or end - b0 < size or outp[u + 1][0] != (b0 + size) & U64):
        return bad
    lo, hi = (start - b0 if first else 0), (end - b0 if last else size)
    if lo >= hi or hi > size:
        return bad
    return (u, land, i, lo, hi), (lo != 0 or hi != size)


def plan(outp, ranges, out_bytes):
    """-> (statuses, units): units = [(unit, land mod 2^64, range, lo, hi, edge)], edge =
    0, or 2 range + 1 for the span's first chunk, 2 range + 2 for a last one that is not"""
    statuses, units = [], []
    for i, rng in enumerate(ranges):
        st, u0, u1, k = span(outp, rng, out_bytes)
        statuses.append(st)
        for u in range(u0, u0 + k):
            e, is_edge = unit(outp, rng, i, u0, u1, u)
            units.append(e + ((2 * i + (1 if u == u0 else 2)) if is_edge else 0,))
    return statuses, units


def classify(outp, rng, out_bytes):
    """what kind of range this is, for the tests to prove that their inputs reach a
    case: a set of words"""
    st, u0, u1, k = span(outp, rng, out_bytes)
    if st != OK or k == 0:
        return {"refused" if st != OK else "empty"}
    us = [unit(outp, rng, 0, u0, u1, u) for u in range(u0, u0 + k)]
    kinds = set()
    if any(e[4] == BAD for e, _ in us):
        kinds.add("bad")
    if any(e[4] == 0 for e, _ in us):
        kinds.add("empty chunk inside")
    if any(not edge and e[4] not in (0, BAD) for e, edge in us):
        kinds.add("interior")
    first, last = us[0][1], us[-1][1] and k > 1
    if k == 1:
        kinds.add("single edge" if first else "single whole")
    else:
        kinds.add({(True, True): "both edges", (True, False): "first edge", (False, True): "last edge",
                   (False, False): "no edge"}[(first, bool(last))])
    return kinds


def stage_size(size):
    return (size + 15) & ~15


def pack(outp, units, budget):
    """the staging of the edge units in plan order -> (places {edge word: place},
    group starts [unit index], stage bytes used)"""
    places, gstart, fill, stage = {}, [0], 0, 0
    for p, e in enumerate(units):
        if not e[5]:
            continue
        need = stage_size(outp[e[0]][1])
        if fill and (need > budget or fill > budget - need):
            fill = 0
            gstart.append(p)
        places[e[5]] = fill
        fill += need
        stage = max(stage, fill)
    return places, gstart, stage


def unit_check(payload5, co, cl, w0, w1, size, hi):
    """the table stage's verdict on a non-empty unit; payload5 = the payload's first
    min(cl, 5) bytes (looked at only after the first two checks)"""
    if co < w0 or co > w1 or cl > w1 - co:
        return ERR_TRUNCATED
    if cl == 0:
        return ERR_HEADER
    if size > CHUNK_MAX:
        return ERR_UNSUPPORTED
    if hi == BAD:
        return ERR_INDEX
    length, shift, done = 0, 0, False
    for b in payload5[:min(cl, 5)]:
        length |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            done = True
            break
    if not done or length != size:
        return ERR_HEADER
    return OK


def range_status(stream, comp, outp, rng, out_bytes, decode_status, w0=0, w1=None):
    """(status, early): the range's status by the rule of DESIGN.md 7.8; early = it was
    refused before any decode (nothing of it is stored).  decode_status(payload) ->
    the element status of one raw stream."""
    w1 = len(stream) if w1 is None else w1
    st, u0, u1, k = span(outp, rng, out_bytes)
    if st != OK:
        return st, True
    us = [unit(outp, rng, 0, u0, u1, u)[0] for u in range(u0, u0 + k)]
    for e in us:
        if e[4] == 0:
            continue
        co, cl = comp[e[0]]
        inside = w0 <= co <= w1 and cl <= w1 - co
        st = unit_check(bytes(stream[co:co + min(cl, 5)]) if inside else b"", co, cl, w0, w1, outp[e[0]][1], e[4])
        if st != OK:
            return st, True
    for e in us:
        if e[4] == 0:
            continue
        co, cl = comp[e[0]]
        st = decode_status(bytes(stream[co:co + cl]))
        if st != OK:
            return st, False
    return OK, False


def defers_in_pass_one(payload):
    """True when a block after the first of this raw stream holds a copy that reaches
    into an earlier block: the long-record decode defers such a block to its second
    pass.  The stream is walked element by element."""
    p, n, shift = 0, 0, 0
    while True:
        b = payload[p]
        p += 1
        n |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    op = 0
    while p < len(payload) and op < n:
        tag = payload[p]
        t = tag & 3
        if t == 0:
            m = tag >> 2
            k = m - 59 if m >= 60 else 0
            ln = (int.from_bytes(payload[p + 1:p + 1 + k], "little") if k else m) + 1
            p += 1 + k + ln
            op += ln
            continue
        if t == 1:
            ln, off = 4 + ((tag >> 2) & 7), ((tag >> 5) << 8) | payload[p + 1]
            p += 2
        elif t == 2:
            ln, off = (tag >> 2) + 1, int.from_bytes(payload[p + 1:p + 3], "little")
            p += 3
        else:
            ln, off = (tag >> 2) + 1, int.from_bytes(payload[p + 1:p + 5], "little")
            p += 5
        if op // BLOCK >= 1 and op - off < (op // BLOCK) * BLOCK:
            return True
        op += ln
    return False
