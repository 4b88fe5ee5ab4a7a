"""CPU, no kernel: the output bound of the framed compressor with a chunk size,
and the store rule on pieces planted at its threshold (frame_store_cases.py)."""
import numpy as np
import pytest

import frame_store_cases as fs
import snappy_amd

CHUNKS = [1, 17, 4096, 32768, 32769, 65536]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_max_frame_output_ex_formula(chunk):
    lib = snappy_amd.lib()
    for k in (0, 1, 2, 3, 7, 100):
        for d in (-1, 0, 1):
            n = k * chunk + d
            if n < 0:
                continue
            units = (n + chunk - 1) // chunk
            want = 10 + 8 * units + lib.snappy_amd_max_output(n, chunk, snappy_amd.STREAMS)
            assert lib.snappy_amd_max_frame_output_ex(n, chunk) == want, (n, chunk)
            assert snappy_amd.max_frame_output(n, chunk) == want
            # the bound holds whatever is stored: a stored chunk is 8 + R bytes
            assert want >= 10 + 8 * units + n


def test_max_frame_output_ex_refuses_chunk_sizes():
    lib = snappy_amd.lib()
    for n in (0, 1, 65536, 1 << 20):
        assert lib.snappy_amd_max_frame_output_ex(n, 0) == 0
        assert lib.snappy_amd_max_frame_output_ex(n, 65537) == 0
        assert snappy_amd.max_frame_output(n, 0) == 0 and snappy_amd.max_frame_output(n, 65537) == 0
        assert lib.snappy_amd_max_frame_output_ex(n, 65536) == lib.snappy_amd_max_frame_output(n)
        assert snappy_amd.max_frame_output(n) == lib.snappy_amd_max_frame_output(n)


@pytest.mark.parametrize("R", fs.PLANT_R)
def test_threshold_plants_exist(R):
    found = fs.plants(R)
    assert sorted(found) == [-1, 0, 1], (R, sorted(found))
    for d, piece in found.items():
        assert len(piece) == R
        stream, table, kinds = fs.model(piece, R, True)
        assert kinds == ("C" if d < 0 else "S"), (R, d)
        assert stream[10] == (0 if d < 0 else 1)
        # a stored chunk: 8 + R bytes; a compressed one: 8 + P
        assert table == [10, 10 + 8 + (R if d >= 0 else R - R // 8 - 1)]
        assert fs.model(piece, R, False)[2] == "C"


@pytest.mark.parametrize("R", range(1, 17))
def test_pieces_of_at_most_16_bytes_are_always_stored(R):
    for piece in (bytes(R), fs.noise()[:R]):
        P = fs.stream_bytes(piece)
        assert P >= R + 2, (R, P)
        assert fs.is_stored(R, P)
        assert fs.model(piece, R, True)[2] == "S"
