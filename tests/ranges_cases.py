"""Foreign streams for the range-decode tests, as `ops` lists of
golden_inputs.build_stream, with the blocks and ranges worked out by hand.

straddles (266,773 bytes, blocks 0..4):
  a 70,000-byte literal over blocks 0 and 1; a literal up to 131,172 (into block
  2); a copy in block 2 with offset 70,000 (source in block 0); a literal up to
  196,598; a 64-byte copy that straddles into block 3; literals over blocks 3 and
  4; an overlapping copy-1 inside block 4.  Blocks 2 and 3 are dependent; blocks
  1 and 4 only resume literals.
copies (131,779 bytes, blocks 0..2):
  a literal of 65,540 bytes; a copy in block 1 reaching 60,000 back (block 0);
  literals into block 2; two copies inside block 2.  Block 1 is dependent."""

OK, ERR_DEPENDENT = 0, -13

FOREIGN = {
    "straddles": [["lit", 70000, 101], ["lit", 61172, 102], ["copy", 64, 70000, 4], ["lit", 65362, 103],
                  ["copy", 64, 100, 2], ["lit", 30000, 104], ["lit", 40000, 105], ["copy", 11, 4, 1], ["lit", 100, 106]],
    "copies": [["lit", 65540, 107], ["copy", 64, 60000, 2], ["lit", 65000, 108], ["lit", 1000, 109], ["copy", 11, 4, 1],
               ["copy", 64, 500, 2], ["lit", 100, 110]],
}
FOREIGN_LEN = {"straddles": 266773, "copies": 131779}
FOREIGN_DEPENDENT = {"straddles": [2, 3], "copies": [1]}

_RANGES = {
    "straddles": [
        (0, 1, OK), (100, 65000, OK), (65535, 2, OK), (65536, 65536, OK), (69995, 10, OK), (1, 65535, OK),
        (0, 131072, OK), (262144, 4629, OK), (266000, 773, OK), (266772, 1, OK),
        (131072, 10, ERR_DEPENDENT), (131000, 100, ERR_DEPENDENT), (196608, 1, ERR_DEPENDENT),
        (200000, 62145, ERR_DEPENDENT), (0, 266773, ERR_DEPENDENT), (131171, 2, ERR_DEPENDENT),
        (196607, 2, ERR_DEPENDENT),
    ],
    "copies": [
        (0, 65536, OK), (65535, 1, OK), (131072, 707, OK), (131600, 100, OK),
        (65536, 1, ERR_DEPENDENT), (65535, 2, ERR_DEPENDENT), (100000, 31000, ERR_DEPENDENT), (0, 131779, ERR_DEPENDENT),
    ],
}


def foreign_ranges(name):
    """[(start, length, the status the device call must give)]"""
    return list(_RANGES[name])
