"""CPU: the models of range decode (tests/ranges_model.py).  The plan model is
checked on hand-worked cases; the dependency model is pinned to oracle.decompress:
a block the model calls independent decodes alone, from its own element
boundaries, to exactly its bytes of the whole stream, and a block it calls
dependent either resumes a copy or fails alone with a copy before its start."""
import pytest

import oracle
import ranges_cases as rc
import ranges_model as rm
from golden_inputs import build_stream

B = rm.BLOCK


def test_plan_model_by_hand():
    n = 4 * B + 1234
    st, units = rm.plan(n, B, [(65535, 2, 7), (B, B, 100), (100, 262044, 0), (n - 10, 10, 5), (0, 0, 0), (n, 1, 0),
                               (0, 10, 1 << 20)], 1 << 20)
    assert st == [0, 0, 0, 0, 0, rm.ERR_ARG, rm.ERR_CAPACITY]
    assert units == [
        (0, (7 - 65535) & rm.U64, 0, 65535, 65536, 1), (1, 8, 0, 0, 1, 2),     # two edges, no interior
        (1, 100, 1, 0, B, 0),                                                   # a whole block: no edge
        (0, (0 - 100) & rm.U64, 2, 100, B, 3), (1, B - 100, 2, 0, B, 0), (2, 2 * B - 100, 2, 0, B, 0),
        (3, 3 * B - 100, 2, 0, B, 0),                                           # ends at 262144: the last one is interior
        (4, (5 + 4 * B - (n - 10)) & rm.U64, 3, 1224, 1234, 4),                 # inside the short last block
    ]
    # a range ending at n makes the short last block an interior unit
    assert rm.plan(n, B, [(4 * B, 1234, 0)], 1234)[1] == [(4, 0, 0, 0, 1234, 0)]
    # STREAMS units
    assert rm.plan(40, 17, [(16, 19, 3)], 64) == ([0], [(0, (3 - 16) & rm.U64, 0, 16, 17, 1), (1, 4, 0, 0, 17, 0),
                                                        (2, 21, 0, 0, 1, 2)])


@pytest.mark.parametrize("name", sorted(rc.FOREIGN))
def test_dependency_model_against_the_oracle(name):
    ops = rc.FOREIGN[name]
    stream = build_stream(ops)
    whole = oracle.decompress(stream)
    dep = rm.dependent_blocks(ops)
    els = rm.elements(ops)
    nblk = (len(whole) + B - 1) // B
    assert dep == set(rc.FOREIGN_DEPENDENT[name]) and 0 < len(dep) < nblk
    for b in range(nblk):
        b0 = b * B
        resumes_copy = any(k == "copy" and p < b0 < p + ln for k, p, ln, _ in els)
        if b not in dep:
            assert not resumes_copy
            assert oracle.decompress(rm.block_alone(ops, b)) == whole[b0:b0 + B], (name, b)
        elif not resumes_copy:
            with pytest.raises(ValueError):
                oracle.decompress(rm.block_alone(ops, b))


@pytest.mark.parametrize("name", sorted(rc.FOREIGN))
def test_range_status_model(name):
    """the hand-worked statuses of the shared cases are the model's"""
    ops = rc.FOREIGN[name]
    assert sum(op[1] for op in ops) == rc.FOREIGN_LEN[name]
    for start, length, want in rc.foreign_ranges(name):
        assert rm.range_status(ops, start, length) == want, (name, start, length)
