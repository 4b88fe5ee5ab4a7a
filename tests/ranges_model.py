"""Python models of range decode: the plan rule of
csrc/snappy_ranges.h, and which blocks of a stream built from an `ops` list
(golden_inputs.build_stream) can be decoded on their own.

A block is dependent if and only if it resumes a copy (a copy element that began
in an earlier block still has bytes to write at the block's first byte) or holds
a copy whose source lies before the block.  A literal that straddles into the
block is not a dependency: its remaining bytes stand in the compressed stream."""
from golden_inputs import enc_copy, enc_literal, varint

import datagen

BLOCK = 65536
OK, ERR_ARG, ERR_CAPACITY, ERR_DEPENDENT = 0, -1, -6, -13
U64 = (1 << 64) - 1


def plan(n, unit, ranges, out_bytes):
    """-> (statuses, units): units = [(unit, land mod 2^64, range, lo, hi, edge)],
    edge = 0 for a unit wholly inside its range, else the 1-based count of edge
    units so far."""
    assert 1 <= unit <= BLOCK
    statuses, units, edges = [], [], 0
    for i, (start, length, oo) in enumerate(ranges):
        st = OK
        if start > n or length > n - start:
            st = ERR_ARG
        elif oo > out_bytes or length > out_bytes - oo:
            st = ERR_CAPACITY
        statuses.append(st)
        if st != OK or length == 0:
            continue
        end = start + length
        for u in range(start // unit, (end - 1) // unit + 1):
            b0 = u * unit
            size = min(unit, n - b0)
            lo, hi = max(start, b0) - b0, min(end, b0 + size) - b0
            edge = 0
            if lo != 0 or hi != size:
                edges += 1
                edge = edges
            units.append((u, (oo + b0 - start) & U64, i, lo, hi, edge))
    return statuses, units


def elements(ops):
    """[(kind, out_pos, length, offset or literal bytes)] of an ops list"""
    out, pos = [], 0
    for op in ops:
        if op[0] == "lit":
            out.append(("lit", pos, op[1], datagen.make("R", op[1], op[2]).tobytes()))
        else:
            out.append(("copy", pos, op[1], op[2]))
        pos += op[1]
    return out


def dependent_blocks(ops, block=BLOCK):
    dep = set()
    for kind, pos, length, x in elements(ops):
        if kind != "copy":
            continue
        for b in range(pos // block, (pos + length - 1) // block + 1):
            b0 = b * block
            if pos < b0:          # the block resumes this copy
                dep.add(b)
            elif pos - x < b0:    # its source starts before the block
                dep.add(b)
    return dep


def range_status(ops, start, length, block=BLOCK):
    if length == 0:
        return OK
    dep = dependent_blocks(ops, block)
    blocks = range(start // block, (start + length - 1) // block + 1)
    return ERR_DEPENDENT if any(b in dep for b in blocks) else OK


def block_alone(ops, b, block=BLOCK):
    """Block b of the stream as a stream of its own: its elements from their
    boundaries, a literal straddling in or any element straddling out cut to the
    block.  Only for a block that is not dependent."""
    b0, b1 = b * block, (b + 1) * block
    body, total = bytearray(), 0
    for kind, pos, length, x in elements(ops):
        lo, hi = max(pos, b0), min(pos + length, b1)
        if lo >= hi:
            continue
        if kind == "lit":
            body += enc_literal(x[lo - pos:hi - pos])
        else:
            assert pos >= b0, "a resumed copy: the block is dependent"
            body += enc_copy(hi - lo, x, 4)
        total += hi - lo
    return varint(total) + bytes(body)
