"""Planted inputs of the framed range decode tests, shared by the
CPU model test, the plan check and the GPU tests: which streams, which ranges,
where they land.  The streams are test_frame's FOREIGN builders; the plain bytes
they return are the reference."""
import random

import frame_model as fm
import frame_ranges_model as frm

SENT = 0xA5
SLICE_STREAMS = ["three runs", "rising sizes (a run each)", "compressed and stored mixed",
                 "empty chunks between full ones", "padding of 0 and of 7 bytes"]


def tables(stream):
    """(chunk table, seek table) of a well-formed stream, by the model"""
    st, chunks, total = fm.chunk_table(stream)
    assert st == fm.OK
    st, starts = frm.seek_table(stream, chunks)
    assert st == frm.OK and starts[-1] == total
    return chunks, starts


def slice_spans(starts, seed=7):
    """[(a, b)]: every range whose ends fall on a chunk boundary +- 1, and one seeded
    random cut inside every non-empty chunk"""
    n = starts[-1]
    pts = sorted({p for b in starts for p in (b - 1, b, b + 1) if 0 <= p <= n})
    spans = [(a, b) for i, a in enumerate(pts) for b in pts[i + 1:]]
    rnd = random.Random(seed)
    for u in range(len(starts) - 1):
        size = starts[u + 1] - starts[u]
        if size >= 2:
            a = rnd.randrange(starts[u], starts[u + 1] - 1)
            spans.append((a, rnd.randrange(a + 1, starts[u + 1])))
    return spans


def residue_spans(starts):
    """16 x one edge pair: the two bytes around the first boundary inside the stream"""
    inner = [b for b in starts[1:-1] if 0 < b < starts[-1]]
    return [(inner[0] - 1, inner[0] + 1)] * 16 if inner else []


def lay_out(spans, residues=0):
    """[(start, length, out_offset)] back to back with gaps of 1..16 sentinel bytes; the
    last `residues` ranges at the output residues 0..15 mod 16.  -> (ranges, out_bytes)"""
    ranges, oo = [], 3
    for k, (a, b) in enumerate(spans):
        if k >= len(spans) - residues:
            oo += 1 + ((k - (len(spans) - residues)) - (oo + 1)) % 16
        ranges.append((a, b - a, oo))
        oo += (b - a) + k % 16 + 1
    return ranges, oo + 5


def slice_case(stream, seed=7):
    chunks, starts = tables(stream)
    res = residue_spans(starts)
    ranges, out_bytes = lay_out(slice_spans(starts, seed) + res, len(res))
    return chunks, starts, ranges, out_bytes


def expected(raw, ranges, out_bytes, accepted=None):
    """the output buffer: the accepted ranges' slices of raw, the sentinel elsewhere"""
    buf = bytearray([SENT]) * max(out_bytes, 1)
    for i, (a, ln, oo) in enumerate(ranges):
        if accepted is None or i in accepted:
            buf[oo:oo + ln] = raw[a:a + ln]
    return bytes(buf)
