"""Python mirror of the reference codec interface, bound to libsnappy_amd.so.

The reference (tturturiello/lightweight-snappy) exposes two C entry points,
``snappy_compress(FILE*, unsigned long long, FILE*)`` (src/snappy_compression.h:8)
and ``snappy_decompress(FILE*, FILE*)`` (src/snappy_decompression.h:15).  This
module offers the same two calls over Python binary file objects, the
in-memory buffer API, and the device-resident batch API (HBM pointers, used by
bench.py and the GPU parity tests).  Everything goes through the C ABI of
libsnappy_amd.so (include/snappy_amd.h), whose kernels run on the MI355X.
There is no CPU fallback: if the library is missing, every call raises.
"""
from __future__ import annotations

import ctypes
import os
from typing import BinaryIO, Optional, Tuple

try:  # share torch's HIP runtime (same SONAME) when torch is present
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is always present in this image
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SNAPPY_AMD_LIB") or os.path.join(HERE, "libsnappy_amd.so")

OK = 0
ERR_ARG = -1
ERR_HEADER = -2
ERR_TRUNCATED = -3
ERR_OFFSET = -4
ERR_OVERRUN = -5
ERR_CAPACITY = -6
ERR_DEVICE = -7
ERR_IO = -8
ERR_UNSUPPORTED = -9
ERR_TIMEOUT = -10
ERR_INDEX = -11
ERR_CHECKSUM = -12
ERR_DEPENDENT = -13  # range decode: a block of the range needs bytes of an earlier block
FRAME_NO_IDENTIFIER = 1  # compress_frame_*: this buffer continues a framed stream
FRAME_STORE = 2  # compress_frame_*: a chunk whose payload is not 1/8 smaller than its bytes is stored (type 01)
FRAME_IDENTIFIER = bytes.fromhex("ff060000734e61507059")
CONTAINER_HADOOP = 0  # Hadoop SnappyCodec blocks (.snappy files)
CONTAINER_XERIAL = 1  # snappy-java SnappyOutputStream chunks
CONTAINER_NO_HEADER = 1  # compress_container_*: this buffer continues a snappy-java stream
CONTAINER_HEADER = bytes.fromhex("82534e41505059000000000100000001")
CONTAINER_BLOCK = {CONTAINER_HADOOP: 131072, CONTAINER_XERIAL: 32768}  # the pieces of block=0
IDX_MAGIC = 0x3158444941504E53  # b"SNPAIDX1" as a little-endian u64

BLOCK = 65536
RECORD_MAX = 65536  # decoded bytes of one record of a record batch
LONG_RECORD_MAX = 1 << 30  # of one record of the long-record calls
SINGLE = 0
STREAMS = 1
NO_PREAMBLE = 1
OPT_SERIAL_INDEX = 1    # snappy_amd_set_option: one-wave index walk instead of K5p
OPT_K1R_EXTRA_LDS = 2   # extra dynamic LDS bytes per K1r unit (occupancy experiments)

_NAMES = {
    ERR_ARG: "bad argument",
    ERR_HEADER: "bad varint preamble",
    ERR_TRUNCATED: "truncated element",
    ERR_OFFSET: "copy offset out of range",
    ERR_OVERRUN: "element overruns declared length",
    ERR_CAPACITY: "output buffer too small",
    ERR_DEVICE: "HIP device error",
    ERR_IO: "I/O error",
    ERR_UNSUPPORTED: "unsupported",
    ERR_TIMEOUT: "block dependency wait timed out",
    ERR_INDEX: "sidecar index does not fit the stream",
    ERR_CHECKSUM: "chunk CRC-32C mismatch",
    ERR_DEPENDENT: "a block of the range needs an earlier block",
}

# every function include/*.h declares, with its ctypes signature
_c = ctypes
_SIGS = {
    "snappy_compress": (None, [_c.c_void_p, _c.c_ulonglong, _c.c_void_p]),
    "snappy_decompress": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "snappy_compress_bst": (_c.c_int, [_c.c_void_p, _c.c_ulonglong, _c.c_void_p]),
    "snappy_compress_file_indexed": (_c.c_int, [_c.c_void_p, _c.c_ulonglong, _c.c_void_p, _c.c_void_p]),
    "snappy_decompress_file_indexed": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "snappy_amd_last_status": (_c.c_int, []),
    "snappy_varint_encode": (_c.c_uint32, [_c.c_uint64, _c.c_void_p]),
    "snappy_varint_decode": (_c.c_uint32, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64)]),
    "snappy_max_compressed_length": (_c.c_size_t, [_c.c_size_t]),
    "snappy_compress_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "snappy_amd_build_config": (_c.c_char_p, []),
    "snappy_amd_bst_compress_file": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_void_p]),
    "snappy_compress_bst_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                              _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                            _c.POINTER(_c.c_size_t)]),
    "snappy_uncompressed_length": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64)]),
    "snappy_amd_create": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_void_p)]),
    "snappy_amd_destroy": (None, [_c.c_void_p]),
    "snappy_amd_set_stream": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    "snappy_amd_get_stream": (_c.c_void_p, [_c.c_void_p]),
    "snappy_amd_device_bytes": (_c.c_size_t, [_c.c_void_p]),
    "snappy_amd_trim": (_c.c_int, [_c.c_void_p]),
    "snappy_amd_num_units": (_c.c_size_t, [_c.c_size_t, _c.c_uint32, _c.c_int]),
    "snappy_amd_max_output": (_c.c_size_t, [_c.c_size_t, _c.c_uint32, _c.c_int]),
    "snappy_amd_compress_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_int,
                                              _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "snappy_amd_decompress_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                _c.c_uint32, _c.c_int, _c.c_void_p]),
    "snappy_amd_decompress_device_async": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                                      _c.c_uint32, _c.c_int, _c.c_void_p]),
    "snappy_amd_decompress_status": (_c.c_int, [_c.c_void_p]),
    "snappy_amd_compress_device_ex": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_int,
                                                 _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                                 _c.POINTER(_c.c_size_t)]),
    "snappy_amd_decompress_device_ex": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_uint32,
                                                   _c.c_int, _c.c_uint32, _c.c_uint64, _c.c_void_p, _c.c_int]),
    "snappy_amd_index_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                           _c.POINTER(_c.c_size_t)]),
    "snappy_amd_last_timings": (_c.c_int, [_c.c_void_p, _c.POINTER(_c.c_float), _c.POINTER(_c.c_float),
                                           _c.POINTER(_c.c_float)]),
    "snappy_amd_enable_timing": (_c.c_int, [_c.c_void_p, _c.c_int]),
    "snappy_amd_set_option": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int64]),
    "snappy_amd_host_set_device": (_c.c_int, [_c.c_int]),
    "snappy_amd_host_get_device": (_c.c_int, []),
    "snappy_amd_host_release": (_c.c_int, []),
    "snappy_amd_host_pool_size": (_c.c_size_t, []),
    "snappy_compress_buffer_multi": (_c.c_int, [_c.POINTER(_c.c_int), _c.c_int, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_buffer_multi": (_c.c_int, [_c.POINTER(_c.c_int), _c.c_int, _c.c_void_p, _c.c_size_t,
                                                  _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "snappy_amd_host_compress": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_uint64, _c.c_void_p, _c.c_size_t,
                                            _c.POINTER(_c.c_size_t)]),
    "snappy_amd_host_decompress": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                              _c.POINTER(_c.c_size_t)]),
    "snappy_amd_host_decompress_idx": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                  _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    # FILE* in, header value, FILE* out, FILE* sidecar (or NULL), bytes read (C stdio streams; the C host layer)
    "snappy_amd_host_compress_file": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_void_p, _c.c_void_p,
                                                 _c.POINTER(_c.c_uint64)]),
    # FILE* in, sidecar entries (or NULL) and their count, FILE* out
    "snappy_amd_host_decompress_file": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    # framing format
    "snappy_amd_crc32c_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                            _c.c_void_p]),
    "snappy_amd_max_frame_output": (_c.c_size_t, [_c.c_size_t]),
    "snappy_amd_compress_frame_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_void_p,
                                                    _c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "snappy_amd_max_frame_output_ex": (_c.c_size_t, [_c.c_size_t, _c.c_uint32]),
    "snappy_amd_compress_frame_device_ex": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_uint32,
                                                       _c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "snappy_compress_frame_buffer_ex": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_uint32, _c.c_void_p,
                                                   _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "snappy_compress_file_framed_ex": (_c.c_int, [_c.c_void_p, _c.c_ulonglong, _c.c_uint32, _c.c_uint32, _c.c_void_p]),
    "snappy_amd_frame_index_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                 _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_size_t)]),
    "snappy_amd_decompress_frame_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                      _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                      _c.POINTER(_c.c_size_t)]),
    "snappy_compress_frame_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_frame_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                  _c.POINTER(_c.c_size_t)]),
    "snappy_frame_uncompressed_length": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_uint64)]),
    # record batches
    "snappy_amd_max_records_output": (_c.c_size_t, [_c.c_size_t, _c.c_size_t]),
    "snappy_amd_max_records_scratch": (_c.c_size_t, [_c.c_size_t, _c.c_size_t]),
    "snappy_amd_compress_records_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                      _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p,
                                                      _c.POINTER(_c.c_size_t)]),
    "snappy_amd_records_length_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                    _c.c_void_p, _c.c_void_p]),
    "snappy_amd_decompress_records_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                        _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                        _c.c_void_p, _c.c_int]),
    # long records
    "snappy_amd_max_long_records_output": (_c.c_size_t, [_c.c_size_t, _c.c_size_t]),
    "snappy_amd_max_long_records_scratch": (_c.c_size_t, [_c.c_size_t, _c.c_size_t]),
    "snappy_amd_max_records_index": (_c.c_size_t, [_c.c_size_t, _c.c_size_t]),
    "snappy_amd_compress_long_records_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                           _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                           _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                           _c.POINTER(_c.c_size_t)]),
    "snappy_amd_records_index_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                   _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "snappy_amd_decompress_long_records_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                             _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                             _c.c_void_p, _c.c_void_p, _c.c_int]),
    # range decode
    "snappy_amd_decompress_ranges_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_size_t, _c.c_void_p,
                                                       _c.c_size_t, _c.c_uint32, _c.c_int, _c.c_void_p, _c.c_size_t,
                                                       _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_int]),
    "snappy_decompress_range_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_uint64,
                                                  _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_file_range": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p]),
    # range decode of framed streams
    "snappy_amd_frame_seek_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                _c.c_void_p, _c.POINTER(_c.c_size_t)]),
    "snappy_frame_tables": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                       _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_uint64)]),
    "snappy_amd_decompress_frame_ranges_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_size_t,
                                                             _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                             _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "snappy_decompress_frame_range_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_uint64, _c.c_size_t,
                                                        _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_file_frame_range": (_c.c_int, [_c.c_void_p, _c.c_uint64, _c.c_uint64, _c.c_void_p]),
    "snappy_compress_file_framed": (_c.c_int, [_c.c_void_p, _c.c_ulonglong, _c.c_void_p]),
    "snappy_decompress_file_framed": (_c.c_int, [_c.c_void_p, _c.c_void_p]),
    # Hadoop / snappy-java containers
    "snappy_amd_max_container_output": (_c.c_size_t, [_c.c_size_t, _c.c_uint32, _c.c_int]),
    "snappy_amd_compress_container_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_int,
                                                        _c.c_uint32, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                        _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_size_t),
                                                        _c.POINTER(_c.c_size_t)]),
    "snappy_amd_container_index_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p,
                                                     _c.c_void_p, _c.c_size_t, _c.POINTER(_c.c_size_t),
                                                     _c.POINTER(_c.c_size_t)]),
    "snappy_amd_decompress_container_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_int,
                                                          _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                          _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "snappy_compress_container_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_uint32, _c.c_int, _c.c_void_p,
                                                    _c.c_size_t, _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_container_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_size_t,
                                                      _c.POINTER(_c.c_size_t)]),
    "snappy_container_uncompressed_length": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int,
                                                        _c.POINTER(_c.c_uint64)]),
    "snappy_compress_file_container": (_c.c_int, [_c.c_void_p, _c.c_ulonglong, _c.c_uint32, _c.c_int, _c.c_void_p]),
    "snappy_decompress_file_container": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p]),
    # range decode of containers
    "snappy_amd_decompress_container_ranges_device": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_uint64, _c.c_size_t,
                                                                 _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p,
                                                                 _c.c_size_t, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "snappy_container_tables": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                           _c.POINTER(_c.c_size_t), _c.POINTER(_c.c_uint64)]),
    "snappy_decompress_container_range_buffer": (_c.c_int, [_c.c_void_p, _c.c_size_t, _c.c_int, _c.c_uint64,
                                                            _c.c_size_t, _c.c_void_p, _c.c_size_t,
                                                            _c.POINTER(_c.c_size_t)]),
    "snappy_decompress_file_container_range": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_uint64, _c.c_uint64,
                                                          _c.c_void_p]),
}
# the reference Buffer cursor helpers, in libsnappy_amd_compat.so (Buffer* is a
# struct of two pointers and a u32)
_COMPAT_SIGS = {
    "init_Buffer": (None, [_c.c_void_p, _c.c_uint]),
    "move_current": (None, [_c.c_void_p, _c.c_uint]),
    "reset": (None, [_c.c_void_p]),
}
COMPAT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libsnappy_amd_compat.so")

_lib: Optional[ctypes.CDLL] = None


class SnappyError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        super().__init__(f"{what}: error {code} ({_NAMES.get(code, 'unknown')})" if what else
                         f"error {code} ({_NAMES.get(code, 'unknown')})")


def lib() -> ctypes.CDLL:
    """Load libsnappy_amd.so (raises loudly if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C lightweight-snappy_amd)")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def compat_lib() -> ctypes.CDLL:
    """Load libsnappy_amd_compat.so (the reference's Buffer cursor helpers)."""
    if not os.path.exists(COMPAT_PATH):
        raise RuntimeError(f"{COMPAT_PATH} is missing: run __graft_entry__.build()")
    l = ctypes.CDLL(COMPAT_PATH)
    for name, (res, args) in _COMPAT_SIGS.items():
        fn = getattr(l, name)
        fn.restype = res
        fn.argtypes = args
    return l


def _check(rc: int, what: str) -> None:
    if rc != OK:
        raise SnappyError(rc, what)


def _buf(data) -> Tuple[ctypes.c_void_p, int, object]:
    mv = memoryview(data).cast("B")
    n = mv.nbytes
    if n == 0:
        return ctypes.c_void_p(0), 0, None
    if mv.readonly:
        keep = ctypes.create_string_buffer(bytes(mv), n)
    else:
        keep = (ctypes.c_uint8 * n).from_buffer(mv)
    return ctypes.cast(keep, ctypes.c_void_p), n, keep


def build_config() -> str:
    """The kernels' compile-time knobs (snappy_amd_build_config); a product
    library reports measurement=0 for both halves."""
    return lib().snappy_amd_build_config().decode()


# ---- varint (src/varint.c) ------------------------------------------------
def varint_encode(n: int) -> bytes:
    out = ctypes.create_string_buffer(16)
    k = lib().snappy_varint_encode(n, out)
    return out.raw[:k]


def varint_decode(data: bytes) -> Tuple[int, int]:
    """Returns (value, bytes consumed); consumed 0 means malformed."""
    v = ctypes.c_uint64(0)
    p, n, keep = _buf(data)
    k = lib().snappy_varint_decode(p, n, ctypes.byref(v))
    return v.value, k


# ---- in-memory API --------------------------------------------------------
def max_compressed_length(n: int) -> int:
    return lib().snappy_max_compressed_length(n)


def compress(data, header_value: Optional[int] = None) -> bytes:
    """One stream, byte-identical to the reference snappy_compress()."""
    p, n, keep = _buf(data)
    cap = max_compressed_length(n)
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    hv = n if header_value is None else header_value
    _check(lib().snappy_amd_host_compress(p, n, hv, out, cap, ctypes.byref(got)), "compress")
    return out.raw[: got.value]


def compress_bst(data) -> bytes:
    """The -b stream, byte-identical to the reference snappy_compress_bst()
    (src/snappy_compression_tree.c:291-306): host threads, no GPU."""
    p, n, keep = _buf(data)
    cap = max_compressed_length(n)
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_compress_bst_buffer(p, n, out, cap, ctypes.byref(got)), "compress_bst")
    return out.raw[: got.value]


def uncompressed_length(data) -> int:
    p, n, keep = _buf(data)
    v = ctypes.c_uint64(0)
    _check(lib().snappy_uncompressed_length(p, n, ctypes.byref(v)), "uncompressed_length")
    return v.value


def _declared_length(data, n: int) -> int:
    """The preamble's N, refused (as the library refuses it) when n bytes of
    stream cannot expand to it: at most 64 output bytes per 3-byte element."""
    N = uncompressed_length(data)
    if N // 22 > n:
        raise SnappyError(ERR_TRUNCATED, "decompress")
    return N


def decompress(data) -> bytes:
    p, n, keep = _buf(data)
    if n == 0:
        return b""
    N = _declared_length(data, n)
    out = ctypes.create_string_buffer(max(N, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_buffer(p, n, out, N, ctypes.byref(got)), "decompress")
    return out.raw[: got.value]


def compress_multi(data, devices) -> bytes:
    """snappy_compress_buffer_multi: one stream (== compress(data)) made on
    several devices, each compressing a contiguous range of blocks."""
    p, n, keep = _buf(data)
    devs = (ctypes.c_int * len(devices))(*devices)
    out = ctypes.create_string_buffer(max(max_compressed_length(n), 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_compress_buffer_multi(devs, len(devices), p, n, out, ctypes.byref(got)), "compress_multi")
    return out.raw[: got.value]


def decompress_multi(data, devices) -> bytes:
    """snappy_decompress_buffer_multi: decompress(data) over several devices."""
    p, n, keep = _buf(data)
    if n == 0:
        return b""
    N = _declared_length(data, n)
    devs = (ctypes.c_int * len(devices))(*devices)
    out = ctypes.create_string_buffer(max(N, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_buffer_multi(devs, len(devices), p, n, out, N, ctypes.byref(got)),
           "decompress_multi")
    return out.raw[: got.value]


def max_frame_output(n: int, chunk: int = BLOCK) -> int:
    """Capacity of a framed stream of n bytes in chunks of `chunk` bytes (0: no such chunk size)."""
    if not 0 <= chunk <= 0xFFFFFFFF:
        return 0
    return lib().snappy_amd_max_frame_output_ex(n, chunk)


def compress_frame(data, chunk: int = BLOCK, store: bool = False) -> bytes:
    """data in the Snappy framing format (framing_format.txt): the stream
    identifier, then one chunk with its CRC-32C per `chunk` bytes (1..65,536):
    compressed, or with store=True stored (type 01) where the compressed payload
    is not one eighth smaller than the chunk's bytes."""
    p, n, keep = _buf(data)
    if not 0 < chunk <= BLOCK:
        raise SnappyError(ERR_ARG, "compress_frame")
    cap = max_frame_output(n, chunk)
    out = ctypes.create_string_buffer(cap)
    got = ctypes.c_size_t(0)
    _check(lib().snappy_compress_frame_buffer_ex(p, n, chunk, FRAME_STORE if store else 0, out, cap, ctypes.byref(got)),
           "compress_frame")
    return out.raw[: got.value]


def frame_uncompressed_length(data) -> int:
    """Decoded bytes of a framed stream (the chunk walk on the host, no GPU)."""
    p, n, keep = _buf(data)
    v = ctypes.c_uint64(0)
    _check(lib().snappy_frame_uncompressed_length(p, n, ctypes.byref(v)), "frame_uncompressed_length")
    return v.value


def decompress_frame(data, cap: Optional[int] = None) -> bytes:
    """Decode a framed stream of any writer, checking every chunk's CRC-32C."""
    p, n, keep = _buf(data)
    if cap is None:
        cap = frame_uncompressed_length(data)
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_frame_buffer(p, n, out, cap, ctypes.byref(got)), "decompress_frame")
    return out.raw[: got.value]


def frame_tables(data):
    """(chunk table, seek table, decoded bytes) of a framed stream: the chunk walk
    on the host, no kernel.  Both tables are lists of data chunks + 1 entries."""
    p, n, keep = _buf(data)
    room = n // 8 + 2  # (a stream holds at most one data chunk per 8 bytes)
    chunks, starts = (ctypes.c_uint64 * room)(), (ctypes.c_uint64 * room)()
    nch, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
    _check(lib().snappy_frame_tables(p, n, chunks, starts, room, ctypes.byref(nch), ctypes.byref(total)), "frame_tables")
    return list(chunks[: nch.value + 1]), list(starts[: nch.value + 1]), total.value


def decompress_frame_range(data, start: int, length: int) -> bytes:
    """Bytes [start, start + length) of decompress_frame(data), CRC-checked: the
    chunk headers are walked on the host up to the range's last chunk and only the
    chunks the range touches are uploaded."""
    p, n, keep = _buf(data)
    if start < 0 or length < 0:
        raise SnappyError(ERR_ARG, "decompress_frame_range")
    out = ctypes.create_string_buffer(max(length, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_frame_range_buffer(p, n, start, length, out, length, ctypes.byref(got)),
           "decompress_frame_range")
    return out.raw[: got.value]


def container_format(format) -> int:
    """CONTAINER_HADOOP / CONTAINER_XERIAL from the constant or its name ("hadoop", "xerial")."""
    if isinstance(format, str):
        try:
            return {"hadoop": CONTAINER_HADOOP, "xerial": CONTAINER_XERIAL}[format]
        except KeyError:
            raise SnappyError(ERR_ARG, f"container format {format!r}") from None
    return int(format)


def max_container_output(n: int, block: int, format) -> int:
    return lib().snappy_amd_max_container_output(n, block, container_format(format))


def compress_container(data, format, block: int = 0) -> bytes:
    """data as a Hadoop SnappyCodec stream or a snappy-java SnappyOutputStream
    stream: one chunk per `block` input bytes (0: the format's default)."""
    fmt = container_format(format)
    p, n, keep = _buf(data)
    cap = max_container_output(n, block, fmt)
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_compress_container_buffer(p, n, block, fmt, out, cap, ctypes.byref(got)), "compress_container")
    return out.raw[: got.value]


def container_uncompressed_length(data, format) -> int:
    """Decoded bytes of a container stream (the header walk on the host, no GPU)."""
    p, n, keep = _buf(data)
    v = ctypes.c_uint64(0)
    _check(lib().snappy_container_uncompressed_length(p, n, container_format(format), ctypes.byref(v)),
           "container_uncompressed_length")
    return v.value


def decompress_container(data, format, cap: Optional[int] = None) -> bytes:
    """Decode a Hadoop or snappy-java container stream of any writer."""
    fmt = container_format(format)
    p, n, keep = _buf(data)
    if cap is None:
        cap = container_uncompressed_length(data, fmt)
    out = ctypes.create_string_buffer(max(cap, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_container_buffer(p, n, fmt, out, cap, ctypes.byref(got)), "decompress_container")
    return out.raw[: got.value]


def container_tables(data, format):
    """(payload pairs, output pairs, decoded bytes) of a container stream: the
    header walk on the host, no kernel.  Both tables are flat lists of (offset,
    length) pairs, one pair per chunk, as container_index_tensor gives them."""
    fmt = container_format(format)
    p, n, keep = _buf(data)
    room = n // 5 + 1  # (a container holds at most one chunk per 5 bytes)
    comp, outp = (ctypes.c_uint64 * (2 * room))(), (ctypes.c_uint64 * (2 * room))()
    nch, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
    _check(lib().snappy_container_tables(p, n, fmt, comp, outp, room, ctypes.byref(nch), ctypes.byref(total)),
           "container_tables")
    return list(comp[: 2 * nch.value]), list(outp[: 2 * nch.value]), total.value


def decompress_container_range(data, format, start: int, length: int) -> bytes:
    """Bytes [start, start + length) of decompress_container(data, format): the
    headers are walked on the host up to the range's last chunk and only the
    chunks the range touches are uploaded."""
    fmt = container_format(format)
    p, n, keep = _buf(data)
    if start < 0 or length < 0:
        raise SnappyError(ERR_ARG, "decompress_container_range")
    out = ctypes.create_string_buffer(max(length, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_container_range_buffer(p, n, fmt, start, length, out, length, ctypes.byref(got)),
           "decompress_container_range")
    return out.raw[: got.value]


def max_records_output(total_bytes: int, count: int) -> int:
    """Capacity the output of a compress_records call must have."""
    return lib().snappy_amd_max_records_output(total_bytes, count)


def max_records_scratch(total_bytes: int, count: int) -> int:
    """Upper bound of Codec.device_bytes() after a compress_records call."""
    return lib().snappy_amd_max_records_scratch(total_bytes, count)


def max_long_records_output(total_bytes: int, count: int) -> int:
    """Capacity the output of a compress_long_records call must have."""
    return lib().snappy_amd_max_long_records_output(total_bytes, count)


def max_long_records_scratch(total_bytes: int, count: int) -> int:
    """Upper bound of Codec.device_bytes() after a long-records call."""
    return lib().snappy_amd_max_long_records_scratch(total_bytes, count)


def max_records_index(total_bytes: int, count: int) -> int:
    """Entries that hold the block tables of `count` records of `total_bytes`."""
    return lib().snappy_amd_max_records_index(total_bytes, count)


def records_table_bases(lengths):
    """Where each record's block table starts in the packed tables: record i has
    ceil(L_i / 65536) + 1 entries -> list of count + 1 positions."""
    pos = [0]
    for n in lengths:
        pos.append(pos[-1] + (int(n) + BLOCK - 1) // BLOCK + 1)
    return pos


def read_index(data: bytes):
    """Sidecar index file (snappy_amd.h) -> (N, [entries])."""
    import struct
    if len(data) < 24:
        raise SnappyError(ERR_INDEX, "read_index")
    magic, n, count = struct.unpack_from("<QQQ", data, 0)
    # exactly `count` entries, no trailing bytes (the C reader refuses them too)
    if magic != IDX_MAGIC or len(data) != 24 + 8 * count:
        raise SnappyError(ERR_INDEX, "read_index")
    return n, list(struct.unpack_from(f"<{count}Q", data, 24))


def decompress_indexed(data, index_file: bytes) -> bytes:
    """decompress() with a sidecar index instead of the GPU index pass."""
    p, n, keep = _buf(data)
    if n == 0:
        return b""
    _, ent = read_index(index_file)
    arr = (ctypes.c_uint64 * max(len(ent), 1))(*ent)
    N = _declared_length(data, n)
    out = ctypes.create_string_buffer(max(N, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_amd_host_decompress_idx(p, n, arr, len(ent), out, N, ctypes.byref(got)), "decompress_indexed")
    return out.raw[: got.value]


def decompress_range(data, start: int, length: int, index_file: Optional[bytes] = None) -> bytes:
    """Bytes [start, start + length) of decompress(data).  With index_file (the
    sidecar file's bytes) only the compressed bytes of the blocks the range touches
    are uploaded; without it the stream is uploaded whole and indexed on the GPU."""
    p, n, keep = _buf(data)
    if index_file is not None:
        ip, ilen, ikeep = _buf(index_file)
        if ilen == 0:
            raise SnappyError(ERR_INDEX, "decompress_range")
    else:
        ip, ilen = None, 0
    if start < 0 or length < 0:
        raise SnappyError(ERR_ARG, "decompress_range")
    out = ctypes.create_string_buffer(max(length, 1))
    got = ctypes.c_size_t(0)
    _check(lib().snappy_decompress_range_buffer(p, n, ip, ilen, start, length, out, length, ctypes.byref(got)),
           "decompress_range")
    return out.raw[: got.value]


# ---- the reference's FILE*-level calls over Python binary files -------------
def snappy_compress(file_input: BinaryIO, input_size: int, file_compressed: BinaryIO) -> None:
    """snappy_compress (src/snappy_compression.c:414): reads file_input from its
    current position to EOF, writes varint(input_size) ++ blocks; an empty
    read writes nothing."""
    data = file_input.read()
    if not data:
        return
    file_compressed.write(compress(data, header_value=input_size))


def snappy_decompress(file_input: BinaryIO, file_decompressed: BinaryIO) -> int:
    """snappy_decompress (src/snappy_decompression.c:345); returns 0."""
    data = file_input.read()
    file_decompressed.write(decompress(data))
    return 0


# ---- device-resident batch API ------------------------------------------------
class Codec:
    """A device context: kernels run on `device`, on the current torch stream
    of that device when torch tensors are passed (or on the context stream)."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p(0)
        _check(lib().snappy_amd_create(device, ctypes.byref(h)), "snappy_amd_create")
        self._h = h
        self.device = device

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().snappy_amd_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr: int) -> None:
        _check(lib().snappy_amd_set_stream(self._h, ctypes.c_void_p(stream_ptr)), "set_stream")

    def device_bytes(self) -> int:
        """HBM bytes held as scratch by this context (grows to the largest call)."""
        return lib().snappy_amd_device_bytes(self._h)

    def trim(self) -> None:
        """Free the context's scratch (the next call allocates it again)."""
        _check(lib().snappy_amd_trim(self._h), "trim")

    def set_option(self, option: int, value: int) -> None:
        """snappy_amd_set_option: OPT_SERIAL_INDEX (1: one-wave index walk),
        OPT_K1R_EXTRA_LDS (extra dynamic LDS bytes per K1r unit)."""
        _check(lib().snappy_amd_set_option(self._h, option, value), "set_option")

    def enable_timing(self, on: bool = True) -> None:
        _check(lib().snappy_amd_enable_timing(self._h, 1 if on else 0), "enable_timing")

    def last_timings(self) -> Tuple[float, float, float]:
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        _check(lib().snappy_amd_last_timings(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "timings")
        return a.value, b.value, c.value

    @staticmethod
    def num_units(n: int, chunk: int, layout: int) -> int:
        return lib().snappy_amd_num_units(n, chunk, layout)

    @staticmethod
    def max_output(n: int, chunk: int, layout: int) -> int:
        return lib().snappy_amd_max_output(n, chunk, layout)

    # raw-pointer forms ---------------------------------------------------
    def compress_ptr(self, d_in: int, n: int, chunk: int, layout: int, d_out: int, d_offsets: int,
                     want_len: bool = True) -> Optional[int]:
        got = ctypes.c_size_t(0)
        rc = lib().snappy_amd_compress_device(self._h, ctypes.c_void_p(d_in), n, chunk, layout,
                                              ctypes.c_void_p(d_out), ctypes.c_void_p(d_offsets),
                                              ctypes.byref(got) if want_len else None)
        _check(rc, "compress_device")
        return got.value if want_len else None

    def decompress_ptr(self, d_comp: int, d_offsets: int, n: int, chunk: int, layout: int, d_out: int,
                       check: bool = True) -> None:
        if check:
            rc = lib().snappy_amd_decompress_device(self._h, ctypes.c_void_p(d_comp), ctypes.c_void_p(d_offsets),
                                                    n, chunk, layout, ctypes.c_void_p(d_out))
        else:
            rc = lib().snappy_amd_decompress_device_async(self._h, ctypes.c_void_p(d_comp),
                                                          ctypes.c_void_p(d_offsets), n, chunk, layout,
                                                          ctypes.c_void_p(d_out))
        _check(rc, "decompress_device")

    def compress_ptr_ex(self, d_in: int, n: int, chunk: int, layout: int, flags: int, header_value: int,
                        d_out: int, d_offsets: int, want_len: bool = True) -> Optional[int]:
        got = ctypes.c_size_t(0)
        rc = lib().snappy_amd_compress_device_ex(self._h, ctypes.c_void_p(d_in), n, chunk, layout, flags,
                                                 header_value, ctypes.c_void_p(d_out), ctypes.c_void_p(d_offsets),
                                                 ctypes.byref(got) if want_len else None)
        _check(rc, "compress_device_ex")
        return got.value if want_len else None

    def decompress_ptr_ex(self, d_comp: int, d_offsets: int, n: int, chunk: int, layout: int, flags: int,
                          header_value: int, d_out: int, check: bool = True) -> None:
        rc = lib().snappy_amd_decompress_device_ex(self._h, ctypes.c_void_p(d_comp), ctypes.c_void_p(d_offsets), n,
                                                   chunk, layout, flags, header_value, ctypes.c_void_p(d_out),
                                                   1 if check else 0)
        _check(rc, "decompress_device_ex")

    def decompress_status(self) -> int:
        return lib().snappy_amd_decompress_status(self._h)

    def index_ptr(self, d_comp: int, clen: int, d_offsets: int, max_units: int) -> int:
        n = ctypes.c_size_t(0)
        _check(lib().snappy_amd_index_device(self._h, ctypes.c_void_p(d_comp), clen, ctypes.c_void_p(d_offsets),
                                             max_units, ctypes.byref(n)), "index_device")
        return n.value

    # torch-tensor forms ----------------------------------------------------
    def _bind_stream(self):
        # torch's default stream is the legacy null stream (cuda_stream 0): set_stream(0)
        # selects the context's own stream, a blocking one, so it is ordered after it too
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def compress_tensor(self, x, chunk: int = BLOCK, layout: int = SINGLE):
        """x: contiguous uint8 CUDA tensor -> (payload tensor, offsets tensor)."""
        assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        n = x.numel()
        units = self.num_units(n, chunk, layout)
        out = torch.empty(max(self.max_output(n, chunk, layout), 16), dtype=torch.uint8, device=x.device)
        offs = torch.empty(units + 1, dtype=torch.int64, device=x.device)
        self._bind_stream()
        length = self.compress_ptr(x.data_ptr(), n, chunk, layout, out.data_ptr(), offs.data_ptr())
        return out[:length], offs

    def decompress_tensor(self, comp, offsets, n: int, chunk: int = BLOCK, layout: int = SINGLE, out=None):
        assert comp.is_cuda and comp.dtype == torch.uint8
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.uint8, device=comp.device)
        self._bind_stream()
        self.decompress_ptr(comp.data_ptr(), offsets.data_ptr(), n, chunk, layout, out.data_ptr())
        return out[:n]

    def decompress_ranges_tensor(self, comp, offsets, n: int, ranges, out=None, chunk: int = BLOCK,
                                 layout: int = SINGLE, comp_origin: int = 0, want_status: bool = True):
        """Decode the byte ranges `ranges` -- a list or array of (start, length,
        out_offset) -- of the stream whose full index is `offsets` (int64 CUDA
        tensor) and whose compressed bytes [comp_origin, comp_origin + comp.numel())
        are `comp`.  Range i lands at out[out_offset_i : out_offset_i + length_i];
        out=None allocates max(out_offset + length) bytes.  Returns (out, status): an int32 CUDA tensor of each range's status
        (self.last_ranges_status = the first failure), or (out, None) with
        want_status=False, which queues the work and reads nothing back."""
        import numpy as np
        assert comp.is_cuda and comp.dtype == torch.uint8 and comp.is_contiguous()
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous()
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 3))
        count = r.shape[0]
        if out is None:
            need = int((r[:, 1] + r[:, 2]).max()) if count else 0
            out = torch.empty(max(need, 1), dtype=torch.uint8, device=comp.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=comp.device) if want_status else None
        self._bind_stream()
        rc = lib().snappy_amd_decompress_ranges_device(
            self._h, ctypes.c_void_p(comp.data_ptr()), comp_origin, comp.numel(), ctypes.c_void_p(offsets.data_ptr()),
            n, chunk, layout, r.ctypes.data_as(ctypes.c_void_p), count, ctypes.c_void_p(out.data_ptr()), out.numel(),
            ctypes.c_void_p(status.data_ptr()) if want_status else None, 1 if want_status else 0)
        self.last_ranges_status = rc
        if rc in (ERR_DEVICE, ERR_ARG) and not (want_status and count and rc == ERR_ARG):
            raise SnappyError(rc, "decompress_ranges_device")
        return out, (status[:count] if want_status else None)

    def index_tensor(self, comp):
        """Block index of a SINGLE-layout stream (e.g. a reference .snp)."""
        units_max = (1 << 20)
        offs = torch.empty(units_max + 1, dtype=torch.int64, device=comp.device)
        self._bind_stream()
        n = self.index_ptr(comp.data_ptr(), comp.numel(), offs.data_ptr(), units_max + 1)
        units = (n + BLOCK - 1) // BLOCK
        return n, offs[: units + 1]

    # framing format ----------------------------------------------------------
    def crc32c_tensor(self, base, off_len, masked: bool = False):
        """CRC-32C of byte ranges of `base` (uint8 CUDA tensor): off_len is an
        int64 CUDA tensor of (offset, length) pairs -> int32 tensor of u32 bits."""
        assert base.is_cuda and base.dtype == torch.uint8 and off_len.is_cuda and off_len.dtype == torch.int64
        count = off_len.numel() // 2
        out = torch.empty(max(count, 1), dtype=torch.int32, device=base.device)
        self._bind_stream()
        _check(lib().snappy_amd_crc32c_device(self._h, ctypes.c_void_p(base.data_ptr()),
                                              ctypes.c_void_p(off_len.data_ptr()), count, 1 if masked else 0,
                                              ctypes.c_void_p(out.data_ptr())), "crc32c_device")
        return out[:count]

    def compress_frame_ptr(self, d_in: int, n: int, flags: int, d_out: int, d_chunks: int,
                           chunk: Optional[int] = None) -> int:
        """chunk None: compress_frame_device (65,536-byte chunks, FRAME_NO_IDENTIFIER only);
        else compress_frame_device_ex with that chunk size (FRAME_STORE too)."""
        got = ctypes.c_size_t(0)
        if chunk is None:
            _check(lib().snappy_amd_compress_frame_device(self._h, ctypes.c_void_p(d_in), n, flags,
                                                          ctypes.c_void_p(d_out), ctypes.c_void_p(d_chunks),
                                                          ctypes.byref(got)), "compress_frame_device")
        else:
            if not 0 <= chunk <= 0xFFFFFFFF:
                raise SnappyError(ERR_ARG, "compress_frame_device_ex")
            _check(lib().snappy_amd_compress_frame_device_ex(self._h, ctypes.c_void_p(d_in), n, chunk, flags,
                                                             ctypes.c_void_p(d_out), ctypes.c_void_p(d_chunks),
                                                             ctypes.byref(got)), "compress_frame_device_ex")
        return got.value

    def compress_frame_tensor(self, x, flags: int = 0, chunk: int = BLOCK):
        """x: contiguous uint8 CUDA tensor -> (framed stream tensor, chunk table tensor);
        chunks of `chunk` bytes, flags FRAME_NO_IDENTIFIER | FRAME_STORE."""
        assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        if not 0 < chunk <= BLOCK:
            raise SnappyError(ERR_ARG, "compress_frame_device_ex")
        n = x.numel()
        out = torch.empty(max_frame_output(n, chunk), dtype=torch.uint8, device=x.device)
        chunks = torch.empty((n + chunk - 1) // chunk + 1, dtype=torch.int64, device=x.device)
        self._bind_stream()
        length = self.compress_frame_ptr(x.data_ptr(), n, flags, out.data_ptr(), chunks.data_ptr(), chunk)
        return out[:length], chunks

    def frame_index_tensor(self, frame, max_chunks: Optional[int] = None):
        """Chunk table of a framed stream in HBM -> (decoded bytes, table tensor
        of data chunks + 1 entries).  A stream holds at most one data chunk per
        8 bytes, which bounds the table when max_chunks is not given."""
        assert frame.is_cuda and frame.dtype == torch.uint8 and frame.is_contiguous()
        if max_chunks is None:
            max_chunks = frame.numel() // 8 + 2
        chunks = torch.empty(max(max_chunks, 1), dtype=torch.int64, device=frame.device)
        nch, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._bind_stream()
        _check(lib().snappy_amd_frame_index_device(self._h, ctypes.c_void_p(frame.data_ptr()), frame.numel(),
                                                   ctypes.c_void_p(chunks.data_ptr()), max_chunks, ctypes.byref(nch),
                                                   ctypes.byref(n)), "frame_index_device")
        return n.value, chunks[: nch.value + 1]

    def decompress_frame_tensor(self, frame, chunks, n: int, out=None):
        """Decode the data chunks `chunks` names (compress_frame_tensor's or
        frame_index_tensor's table) into n bytes; raises on a CRC mismatch."""
        assert frame.is_cuda and frame.dtype == torch.uint8 and chunks.dtype == torch.int64
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.uint8, device=frame.device)
        got = ctypes.c_size_t(0)
        self._bind_stream()
        _check(lib().snappy_amd_decompress_frame_device(self._h, ctypes.c_void_p(frame.data_ptr()), frame.numel(),
                                                        ctypes.c_void_p(chunks.data_ptr()), chunks.numel() - 1,
                                                        ctypes.c_void_p(out.data_ptr()), n, ctypes.byref(got)),
               "decompress_frame_device")
        return out[: got.value]

    def frame_seek_tensor(self, frame, chunks):
        """Seek table of a framed stream in HBM from its chunk table (int64 CUDA
        tensor, data chunks + 1 entries) -> (decoded bytes, int64 CUDA tensor of
        as many entries: each data chunk's decoded position, then the total)."""
        assert frame.is_cuda and frame.dtype == torch.uint8 and frame.is_contiguous()
        assert chunks.is_cuda and chunks.dtype == torch.int64 and chunks.is_contiguous() and chunks.numel() >= 1
        starts = torch.empty(chunks.numel(), dtype=torch.int64, device=frame.device)
        n = ctypes.c_size_t(0)
        self._bind_stream()
        _check(lib().snappy_amd_frame_seek_device(self._h, ctypes.c_void_p(frame.data_ptr()), frame.numel(),
                                                  ctypes.c_void_p(chunks.data_ptr()), chunks.numel() - 1,
                                                  ctypes.c_void_p(starts.data_ptr()), ctypes.byref(n)),
               "frame_seek_device")
        return n.value, starts

    def decompress_frame_ranges_tensor(self, window, comp_origin: int, chunks, starts, ranges, out=None):
        """Decode the byte ranges `ranges` -- a list or array of (start, length,
        out_offset) -- of the framed stream whose bytes [comp_origin, comp_origin +
        window.numel()) are `window`, through its chunk table and seek table (or
        equally long contiguous sub-tables of both; int64 CUDA tensors).  Range i
        lands at out[out_offset_i : out_offset_i + length_i]; out=None allocates
        max(out_offset + length) bytes.  Returns (out, status): an int32 CUDA tensor
        of each range's status (self.last_ranges_status = the first failure)."""
        import numpy as np
        assert window.is_cuda and window.dtype == torch.uint8 and window.is_contiguous()
        for t in (chunks, starts):
            assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
        assert chunks.numel() == starts.numel() >= 1
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 3))
        count = r.shape[0]
        if out is None:
            need = int((r[:, 1] + r[:, 2]).max()) if count else 0
            out = torch.empty(max(need, 1), dtype=torch.uint8, device=window.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=window.device)
        self._bind_stream()
        rc = lib().snappy_amd_decompress_frame_ranges_device(
            self._h, ctypes.c_void_p(window.data_ptr()), comp_origin, window.numel(),
            ctypes.c_void_p(chunks.data_ptr()), ctypes.c_void_p(starts.data_ptr()), chunks.numel() - 1,
            r.ctypes.data_as(ctypes.c_void_p), count, ctypes.c_void_p(out.data_ptr()), out.numel(),
            ctypes.c_void_p(status.data_ptr()))
        self.last_ranges_status = rc
        if rc == ERR_DEVICE or (rc == ERR_ARG and not count):
            raise SnappyError(rc, "decompress_frame_ranges_device")
        return out, status[:count]

    # Hadoop / snappy-java containers -------------------------------------------
    def compress_container_tensor(self, x, format, block: int = 0, flags: int = 0, out=None, tables: bool = True):
        """x: contiguous uint8 CUDA tensor -> (container tensor, payload pairs,
        output pairs): the chunk tables are int64 tensors of (offset, length)
        pairs, one per chunk (None, None with tables=False).  `out` (a uint8 CUDA
        tensor, any alignment) takes the container; its size is the capacity."""
        assert x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous()
        fmt = container_format(format)
        n = x.numel()
        if out is None:
            out = torch.empty(max(max_container_output(n, block, fmt), 1), dtype=torch.uint8, device=x.device)
        b = block or CONTAINER_BLOCK.get(fmt, 1)
        chunks = (n + b - 1) // b
        comp = outp = None
        if tables:
            comp = torch.empty(2 * max(chunks, 1), dtype=torch.int64, device=x.device)
            outp = torch.empty(2 * max(chunks, 1), dtype=torch.int64, device=x.device)
        nch, got = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._bind_stream()
        _check(lib().snappy_amd_compress_container_device(
            self._h, ctypes.c_void_p(x.data_ptr()), n, block, fmt, flags, ctypes.c_void_p(out.data_ptr()), out.numel(),
            ctypes.c_void_p(comp.data_ptr() if tables else 0), ctypes.c_void_p(outp.data_ptr() if tables else 0),
            chunks, ctypes.byref(nch), ctypes.byref(got)), "compress_container_device")
        if tables:
            comp, outp = comp[: 2 * nch.value], outp[: 2 * nch.value]
        return out[: got.value], comp, outp

    def container_index_tensor(self, cont, format, max_chunks: Optional[int] = None, clen: Optional[int] = None):
        """Chunk tables of a container in HBM -> (decoded bytes, payload pairs,
        output pairs).  A container holds at most one chunk per 5 bytes, which
        bounds the tables when max_chunks is not given.  clen: walk only the
        first clen bytes of cont."""
        assert cont.is_cuda and cont.dtype == torch.uint8 and cont.is_contiguous()
        if clen is None:
            clen = cont.numel()
        if max_chunks is None:
            max_chunks = clen // 5 + 1
        comp = torch.empty(2 * max(max_chunks, 1), dtype=torch.int64, device=cont.device)
        outp = torch.empty(2 * max(max_chunks, 1), dtype=torch.int64, device=cont.device)
        nch, n = ctypes.c_size_t(0), ctypes.c_size_t(0)
        self._bind_stream()
        _check(lib().snappy_amd_container_index_device(self._h, ctypes.c_void_p(cont.data_ptr()), clen,
                                                       container_format(format), ctypes.c_void_p(comp.data_ptr()),
                                                       ctypes.c_void_p(outp.data_ptr()), max_chunks, ctypes.byref(nch),
                                                       ctypes.byref(n)), "container_index_device")
        return n.value, comp[: 2 * nch.value], outp[: 2 * nch.value]

    def decompress_container_tensor(self, cont, format, comp=None, outp=None, cap: Optional[int] = None, out=None,
                                    clen: Optional[int] = None):
        """Decode a container in HBM.  comp / outp: the chunk tables of
        compress_container_tensor or container_index_tensor, or both None: the
        call walks the container itself.  cap: the room for decoded bytes (the
        tables' extent, or the host does not know: pass it or `out`)."""
        assert cont.is_cuda and cont.dtype == torch.uint8 and cont.is_contiguous()
        assert (comp is None) == (outp is None)
        fmt = container_format(format)
        if clen is None:
            clen = cont.numel()
        if out is not None:
            cap = out.numel() if cap is None else cap
        elif cap is None:
            if comp is None:
                # a walk that stores nothing: ERR_CAPACITY only says that it found chunks
                n = ctypes.c_size_t(0)
                self._bind_stream()
                rc = lib().snappy_amd_container_index_device(self._h, ctypes.c_void_p(cont.data_ptr()), clen, fmt,
                                                             ctypes.c_void_p(0), ctypes.c_void_p(0), 0, None,
                                                             ctypes.byref(n))
                if rc != ERR_CAPACITY:
                    _check(rc, "container_index_device")
                cap = n.value
            else:
                cap = int((outp[0::2] + outp[1::2]).max().item()) if outp.numel() else 0
        if out is None:
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=cont.device)
        nch = 0 if comp is None else comp.numel() // 2
        got = ctypes.c_size_t(0)
        self._bind_stream()
        _check(lib().snappy_amd_decompress_container_device(
            self._h, ctypes.c_void_p(cont.data_ptr()), clen, fmt,
            ctypes.c_void_p(comp.data_ptr() if comp is not None else 0),
            ctypes.c_void_p(outp.data_ptr() if outp is not None else 0), nch, ctypes.c_void_p(out.data_ptr()), cap,
            ctypes.byref(got)), "decompress_container_device")
        return out[: got.value]

    def decompress_container_ranges_tensor(self, window, comp_origin: int, comp, outp, ranges, out=None):
        """Decode the byte ranges `ranges` -- a list or array of (start, length,
        out_offset) -- of the container whose bytes [comp_origin, comp_origin +
        window.numel()) are `window`, through its chunk tables (or any contiguous
        run of their pairs; int64 CUDA tensors, offsets absolute).  Range i lands at
        out[out_offset_i : out_offset_i + length_i]; out=None allocates
        max(out_offset + length) bytes.  Returns (out, status): an int32 CUDA tensor
        of each range's status (self.last_ranges_status = the first failure)."""
        import numpy as np
        assert window.is_cuda and window.dtype == torch.uint8 and window.is_contiguous()
        for t in (comp, outp):
            assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
        assert comp.numel() == outp.numel() and comp.numel() % 2 == 0
        r = np.ascontiguousarray(np.asarray(ranges, dtype=np.uint64).reshape(-1, 3))
        count = r.shape[0]
        if out is None:
            need = int((r[:, 1] + r[:, 2]).max()) if count else 0
            out = torch.empty(max(need, 1), dtype=torch.uint8, device=window.device)
        assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=window.device)
        nch = comp.numel() // 2
        self._bind_stream()
        rc = lib().snappy_amd_decompress_container_ranges_device(
            self._h, ctypes.c_void_p(window.data_ptr()), comp_origin, window.numel(),
            ctypes.c_void_p(comp.data_ptr() if nch else 0), ctypes.c_void_p(outp.data_ptr() if nch else 0), nch,
            r.ctypes.data_as(ctypes.c_void_p), count, ctypes.c_void_p(out.data_ptr()), out.numel(),
            ctypes.c_void_p(status.data_ptr()))
        self.last_ranges_status = rc
        if rc == ERR_DEVICE or (rc == ERR_ARG and not count):
            raise SnappyError(rc, "decompress_container_ranges_device")
        return out, status[:count]

    # record batches ------------------------------------------------------------
    def compress_records_tensor(self, base, off_len, out=None, want_status: bool = True, check: bool = False):
        """Compress the records of `base` (uint8 CUDA tensor) that off_len names
        (int64 CUDA tensor of (offset, length) pairs, lengths 0..65,536) ->
        (payload tensor, offsets tensor of count + 1, status tensor of count).
        A refused record has size 0 and its code in the status tensor; check=True
        raises SnappyError with the first refusal instead."""
        assert base.is_cuda and base.dtype == torch.uint8 and base.is_contiguous()
        assert off_len.is_cuda and off_len.dtype == torch.int64 and off_len.is_contiguous()
        count = off_len.numel() // 2
        if out is None:
            # (an upper bound of the accepted bytes without a read-back: each record min(length, 65,536))
            total = int(off_len.view(-1, 2)[:, 1].clamp(0, RECORD_MAX).sum().item()) if count else 0
            out = torch.empty(max_records_output(total, count), dtype=torch.uint8, device=base.device)
        offs = torch.empty(count + 1, dtype=torch.int64, device=base.device)
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=base.device) if want_status else None
        got = ctypes.c_size_t(0)
        self._bind_stream()
        rc = lib().snappy_amd_compress_records_device(
            self._h, ctypes.c_void_p(base.data_ptr()), base.numel(), ctypes.c_void_p(off_len.data_ptr()), count,
            ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(offs.data_ptr()),
            ctypes.c_void_p(status.data_ptr()) if want_status else None, ctypes.byref(got))
        self.last_records_status = rc
        # a refusal is reported per record; anything else (capacity, device, arguments) failed the call
        if rc != OK and (check or rc not in (ERR_UNSUPPORTED, ERR_ARG) or count == 0):
            raise SnappyError(rc, "compress_records_device")
        return out[: got.value], offs, (status[:count] if want_status else None)

    def records_length_tensor(self, comp, off_len):
        """The declared length of every record -> (int64 lengths, int32 status)."""
        assert comp.is_cuda and comp.dtype == torch.uint8 and off_len.is_cuda and off_len.dtype == torch.int64
        count = off_len.numel() // 2
        lens = torch.zeros(max(count, 1), dtype=torch.int64, device=comp.device)
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=comp.device)
        self._bind_stream()
        _check(lib().snappy_amd_records_length_device(self._h, ctypes.c_void_p(comp.data_ptr()), comp.numel(),
                                                      ctypes.c_void_p(off_len.data_ptr()), count,
                                                      ctypes.c_void_p(lens.data_ptr()),
                                                      ctypes.c_void_p(status.data_ptr())), "records_length_device")
        return lens[:count], status[:count]

    def decompress_records_tensor(self, comp, comp_off_len, out, out_off_len, want_status: bool = True,
                                  check: bool = False):
        """Decode record i of `comp` (comp_off_len pairs) into `out` at out_off_len[i]
        (both int64 CUDA tensors of (offset, length) pairs) -> int32 status tensor.
        check=True raises SnappyError with the first failing record's code."""
        assert comp.is_cuda and comp.dtype == torch.uint8 and out.is_cuda and out.dtype == torch.uint8
        assert comp_off_len.dtype == torch.int64 and out_off_len.dtype == torch.int64
        assert comp_off_len.numel() == out_off_len.numel()
        count = comp_off_len.numel() // 2
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=comp.device) if want_status else None
        self._bind_stream()
        rc = lib().snappy_amd_decompress_records_device(
            self._h, ctypes.c_void_p(comp.data_ptr()), comp.numel(), ctypes.c_void_p(comp_off_len.data_ptr()), count,
            ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(out_off_len.data_ptr()),
            ctypes.c_void_p(status.data_ptr()) if want_status else None, 1)
        self.last_records_status = rc
        if rc != OK and (check or rc in (ERR_DEVICE, ERR_ARG)):
            raise SnappyError(rc, "decompress_records_device")
        return status[:count] if want_status else None

    @staticmethod
    def _upload(data: bytes, dev):
        import numpy as np
        if not data:
            return torch.empty(0, dtype=torch.uint8, device=dev)
        return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)

    def compress_records(self, records) -> list:
        """list of bytes-like records (each 0..65,536 bytes) -> list of their raw
        Snappy streams: packed, uploaded, compressed in one call."""
        import numpy as np
        records = [bytes(r) for r in records]
        if not records:
            return []
        lens = np.array([len(r) for r in records], dtype=np.int64)
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        dev = torch.device("cuda", self.device)
        base = self._upload(b"".join(records), dev)
        off_len = torch.from_numpy(np.stack([offs, lens], axis=1).reshape(-1).copy()).to(dev)
        payload, o, _ = self.compress_records_tensor(base, off_len, check=True)
        o, p = o.cpu().numpy(), payload.cpu().numpy().tobytes()
        return [p[int(o[i]): int(o[i + 1])] for i in range(len(records))]

    def decompress_records(self, records) -> list:
        """list of raw Snappy streams -> list of their decoded bytes: one length
        call and one decode call; raises SnappyError with the first failing
        record's code."""
        import numpy as np
        records = [bytes(r) for r in records]
        if not records:
            return []
        clens = np.array([len(r) for r in records], dtype=np.int64)
        coffs = np.concatenate(([0], np.cumsum(clens)[:-1])).astype(np.int64)
        dev = torch.device("cuda", self.device)
        comp = self._upload(b"".join(records), dev)
        c_ol = torch.from_numpy(np.stack([coffs, clens], axis=1).reshape(-1).copy()).to(dev)
        lens, st = self.records_length_tensor(comp, c_ol)
        lens, st = lens.cpu().numpy(), st.cpu().numpy()
        bad = np.nonzero(st)[0]
        if bad.size:
            raise SnappyError(int(st[bad[0]]), f"decompress_records: record {int(bad[0])}")
        big = np.nonzero(lens > RECORD_MAX)[0]
        if big.size:
            raise SnappyError(ERR_UNSUPPORTED, f"decompress_records: record {int(big[0])}")
        ooffs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        out = torch.empty(max(int(lens.sum()), 1), dtype=torch.uint8, device=dev)[: int(lens.sum())]
        o_ol = torch.from_numpy(np.stack([ooffs, lens], axis=1).reshape(-1).copy()).to(dev)
        self.decompress_records_tensor(comp, c_ol, out, o_ol, want_status=False, check=True)
        flat = out.cpu().numpy().tobytes()
        return [flat[int(ooffs[i]): int(ooffs[i] + lens[i])] for i in range(len(records))]

    # long records (0 .. 2^30 bytes each, many blocks) ---------------------------
    def compress_long_records_tensor(self, base, off_len, out=None, want_status: bool = True, check: bool = False,
                                     want_index: bool = True, index=None):
        """compress_records_tensor for records of 0..2^30 bytes -> (payload tensor,
        offsets tensor of count + 1, status tensor of count, block tables).  The
        tables (int64 tensor; None with want_index=False) hold ceil(L/65536) + 1
        entries per record, packed in record order (one entry for a refused record)."""
        assert base.is_cuda and base.dtype == torch.uint8 and base.is_contiguous()
        assert off_len.is_cuda and off_len.dtype == torch.int64 and off_len.is_contiguous()
        count = off_len.numel() // 2
        if out is None or (want_index and index is None):
            # (an upper bound of the accepted bytes without a second read-back: each record min(length, cap))
            total = int(off_len.view(-1, 2)[:, 1].clamp(0, LONG_RECORD_MAX).sum().item()) if count else 0
            if out is None:
                out = torch.empty(max_long_records_output(total, count), dtype=torch.uint8, device=base.device)
            if want_index and index is None:
                index = torch.empty(max(max_records_index(total, count), 1), dtype=torch.int64, device=base.device)
        if not want_index:
            index = None
        offs = torch.empty(count + 1, dtype=torch.int64, device=base.device)
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=base.device) if want_status else None
        got = ctypes.c_size_t(0)
        self._bind_stream()
        rc = lib().snappy_amd_compress_long_records_device(
            self._h, ctypes.c_void_p(base.data_ptr()), base.numel(), ctypes.c_void_p(off_len.data_ptr()), count,
            ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(offs.data_ptr()),
            ctypes.c_void_p(index.data_ptr()) if index is not None else None,
            index.numel() if index is not None else 0,
            ctypes.c_void_p(status.data_ptr()) if want_status else None, ctypes.byref(got))
        self.last_records_status = rc
        # a refusal is reported per record; anything else (capacity, device, arguments) failed the call
        if rc != OK and (check or rc not in (ERR_UNSUPPORTED, ERR_ARG) or count == 0):
            raise SnappyError(rc, "compress_long_records_device")
        return out[: got.value], offs, (status[:count] if want_status else None), index

    def records_index_tensor(self, comp, comp_off_len, out_lens, index=None):
        """The block tables of the records of `comp` (comp_off_len pairs) whose
        decoded lengths are out_lens (int64 CUDA tensor of count lengths, or of
        (offset, length) pairs) -> (tables tensor, int32 status tensor)."""
        assert comp.is_cuda and comp.dtype == torch.uint8 and comp_off_len.is_cuda and comp_off_len.dtype == torch.int64
        assert out_lens.is_cuda and out_lens.dtype == torch.int64
        count = comp_off_len.numel() // 2
        if out_lens.numel() == count and count:
            out_lens = torch.stack([torch.zeros_like(out_lens.view(-1)), out_lens.view(-1)], dim=1).reshape(-1)
        assert out_lens.numel() == 2 * count
        out_lens = out_lens.contiguous()
        if index is None:
            total = int(out_lens.view(-1, 2)[:, 1].clamp(0, LONG_RECORD_MAX).sum().item()) if count else 0
            index = torch.empty(max(max_records_index(total, count), 1), dtype=torch.int64, device=comp.device)
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=comp.device)
        self._bind_stream()
        _check(lib().snappy_amd_records_index_device(
            self._h, ctypes.c_void_p(comp.data_ptr()), comp.numel(), ctypes.c_void_p(comp_off_len.data_ptr()), count,
            ctypes.c_void_p(out_lens.data_ptr()), ctypes.c_void_p(index.data_ptr()), index.numel(),
            ctypes.c_void_p(status.data_ptr())), "records_index_device")
        return index, status[:count]

    def decompress_long_records_tensor(self, comp, comp_off_len, out, out_off_len, index=None,
                                       want_status: bool = True, check: bool = False):
        """decompress_records_tensor for records of 0..2^30 bytes; index = the block
        tables (compress_long_records_tensor's or records_index_tensor's), or None:
        they are built in scratch -> int32 status tensor."""
        assert comp.is_cuda and comp.dtype == torch.uint8 and out.is_cuda and out.dtype == torch.uint8
        assert comp_off_len.dtype == torch.int64 and out_off_len.dtype == torch.int64
        assert comp_off_len.numel() == out_off_len.numel()
        assert index is None or (index.is_cuda and index.dtype == torch.int64)
        count = comp_off_len.numel() // 2
        status = torch.zeros(max(count, 1), dtype=torch.int32, device=comp.device) if want_status else None
        self._bind_stream()
        rc = lib().snappy_amd_decompress_long_records_device(
            self._h, ctypes.c_void_p(comp.data_ptr()), comp.numel(), ctypes.c_void_p(comp_off_len.data_ptr()), count,
            ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(out_off_len.data_ptr()),
            ctypes.c_void_p(index.data_ptr()) if index is not None else None,
            ctypes.c_void_p(status.data_ptr()) if want_status else None, 1)
        self.last_records_status = rc
        if rc != OK and (check or rc in (ERR_DEVICE, ERR_ARG)):
            raise SnappyError(rc, "decompress_long_records_device")
        return status[:count] if want_status else None

    def compress_long_records(self, records) -> list:
        """list of bytes-like records (each 0..2^30 bytes) -> list of their raw
        Snappy streams: packed, uploaded, compressed in one call."""
        import numpy as np
        records = [bytes(r) for r in records]
        if not records:
            return []
        lens = np.array([len(r) for r in records], dtype=np.int64)
        if int(lens.max()) > LONG_RECORD_MAX:
            raise SnappyError(ERR_UNSUPPORTED, f"compress_long_records: record {int(np.argmax(lens > LONG_RECORD_MAX))}")
        offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        dev = torch.device("cuda", self.device)
        base = self._upload(b"".join(records), dev)
        off_len = torch.from_numpy(np.stack([offs, lens], axis=1).reshape(-1).copy()).to(dev)
        payload, o, _, _ = self.compress_long_records_tensor(base, off_len, check=True, want_index=False)
        o, p = o.cpu().numpy(), payload.cpu().numpy().tobytes()
        return [p[int(o[i]): int(o[i + 1])] for i in range(len(records))]

    def decompress_long_records(self, records) -> list:
        """list of raw Snappy streams (each up to 2^30 decoded bytes) -> list of
        their decoded bytes: one length call and one decode call (the block tables
        are built in scratch); raises SnappyError with the first failing record's code."""
        import numpy as np
        records = [bytes(r) for r in records]
        if not records:
            return []
        clens = np.array([len(r) for r in records], dtype=np.int64)
        coffs = np.concatenate(([0], np.cumsum(clens)[:-1])).astype(np.int64)
        dev = torch.device("cuda", self.device)
        comp = self._upload(b"".join(records), dev)
        c_ol = torch.from_numpy(np.stack([coffs, clens], axis=1).reshape(-1).copy()).to(dev)
        lens, st = self.records_length_tensor(comp, c_ol)
        lens, st = lens.cpu().numpy(), st.cpu().numpy()
        bad = np.nonzero(st)[0]
        if bad.size:
            raise SnappyError(int(st[bad[0]]), f"decompress_long_records: record {int(bad[0])}")
        big = np.nonzero((lens > LONG_RECORD_MAX) | (lens < 0))[0]
        if big.size:
            raise SnappyError(ERR_UNSUPPORTED, f"decompress_long_records: record {int(big[0])}")
        ooffs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        out = torch.empty(max(int(lens.sum()), 1), dtype=torch.uint8, device=dev)[: int(lens.sum())]
        o_ol = torch.from_numpy(np.stack([ooffs, lens], axis=1).reshape(-1).copy()).to(dev)
        self.decompress_long_records_tensor(comp, c_ol, out, o_ol, want_status=False, check=True)
        flat = out.cpu().numpy().tobytes()
        return [flat[int(ooffs[i]): int(ooffs[i] + lens[i])] for i in range(len(records))]


def compress_records(records, device: int = 0) -> list:
    """Codec(device).compress_records(records) on a context of its own."""
    c = Codec(device)
    try:
        return c.compress_records(records)
    finally:
        c.close()


def decompress_records(records, device: int = 0) -> list:
    """Codec(device).decompress_records(records) on a context of its own."""
    c = Codec(device)
    try:
        return c.decompress_records(records)
    finally:
        c.close()


def compress_long_records(records, device: int = 0) -> list:
    """Codec(device).compress_long_records(records) on a context of its own
    (the records are checked first: an empty list needs no device)."""
    records = [bytes(r) for r in records]
    if not records:
        return []
    c = Codec(device)
    try:
        return c.compress_long_records(records)
    finally:
        c.close()


def decompress_long_records(records, device: int = 0) -> list:
    """Codec(device).decompress_long_records(records) on a context of its own."""
    records = [bytes(r) for r in records]
    if not records:
        return []
    if any(len(r) == 0 for r in records):
        raise SnappyError(ERR_HEADER, f"decompress_long_records: record {[len(r) for r in records].index(0)}")
    c = Codec(device)
    try:
        return c.decompress_long_records(records)
    finally:
        c.close()
