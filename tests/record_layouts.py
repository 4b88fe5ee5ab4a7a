"""Layouts of the record-form planted suites (test_k4_record_forms.py,
test_k1r_k2_record_forms.py), kept in one place so that both lay records out by
the same rules and a CPU test can assert what the layouts claim:

* sources: the records lie in one buffer whose first byte is `shift` = 0..3 bytes
  into a dword, the address order shuffled against the batch order, 0..7 filler
  bytes (0x5A) in front of each so that within every kernel class the k-th record
  of the batch stands at the absolute alignment (k + a class rotation) mod 4.  A
  group of records lies back to back (its first member carries the alignment):
  what follows a record in memory is then chosen by the caller.
* destinations: ranges of a 0xA5-filled buffer (16-byte aligned), the address
  order shuffled again, gaps of 1..40 sentinel bytes, within every family the k-th
  record at the residue (k + a family rotation) mod 16, or at the residue the
  caller names.
* the check: the whole output buffer against an image -- the records where they
  belong, the sentinel everywhere else; a record whose expected bytes are None
  (it fails while decoding, and its contract allows a partial write) has its own
  range left out, nothing else.
"""
import collections
import ctypes
import random

import numpy as np

SENT = 0xA5
FILL = 0x5A


def pack(groups, classes, seed: int, shift: int):
    """groups: lists of bytes (the members of one group lie back to back, in batch
    order); classes: one key per group, the kernel class of its first member.
    -> (blob, [(offset, length)] of every member in batch order)."""
    assert 0 <= shift < 4 and len(groups) == len(classes)
    rng = random.Random(seed)
    rot = {}
    seen = collections.Counter()
    want = []
    for cls in classes:
        rot.setdefault(cls, rng.randrange(4))
        want.append((seen[cls] + rot[cls]) % 4)
        seen[cls] += 1
    order = list(range(len(groups)))
    rng.shuffle(order)
    blob, at = bytearray(), [None] * len(groups)
    for g in order:
        pad = (want[g] - (shift + len(blob))) % 4 + 4 * rng.randrange(2)
        blob += bytes([FILL]) * pad
        at[g] = len(blob)
        for member in groups[g]:
            blob += member
    blob += bytes([FILL]) * rng.randrange(1, 8)
    descs = []
    for g, members in enumerate(groups):
        pos = at[g]
        for member in members:
            descs.append((pos, len(member)))
            pos += len(member)
    return bytes(blob), descs


def scatter(lens, families, seed: int, residues=None):
    """Output ranges for records of these decoded lengths -> ([(offset, length)] in
    batch order, buffer size).  residues: {record: its residue mod 16}, for the
    records whose residue the caller names."""
    assert len(lens) == len(families)
    rng = random.Random(seed)
    residues = residues or {}
    rot, seen, want = {}, collections.Counter(), []
    for i, fam in enumerate(families):
        rot.setdefault(fam, rng.randrange(16))
        want.append(residues.get(i, (seen[fam] + rot[fam]) % 16))
        seen[fam] += 1
    order = list(range(len(lens)))
    rng.shuffle(order)
    pos, descs = 0, [None] * len(lens)
    for i in order:
        gap = (want[i] - pos - 1) % 16 + 1
        gap += 16 * rng.randrange((40 - gap) // 16 + 1)
        assert 1 <= gap <= 40
        pos += gap
        descs[i] = (pos, lens[i])
        pos += lens[i]
    return descs, pos + rng.randrange(1, 41)


def source_alignments(descs, classes, shift: int):
    """{class: the absolute alignments mod 4 of its non-empty records}; classes: one key per record."""
    got = collections.defaultdict(set)
    for (o, ln), cls in zip(descs, classes):
        if ln:
            got[cls].add((shift + o) % 4)
    return dict(got)


def dest_residues(o_descs, families):
    """{family: the residues mod 16 of its non-empty output ranges}"""
    got = collections.defaultdict(set)
    for (o, ln), fam in zip(o_descs, families):
        if ln:
            got[fam].add(o % 16)
    return dict(got)


def shuffled_against_addresses(descs) -> bool:
    """The batch order is not the address order (nor its reverse)."""
    offs = [o for o, _ in descs]
    return len(offs) < 3 or (offs != sorted(offs) and offs != sorted(offs, reverse=True))


def gaps_of(o_descs, size: int):
    """The sentinel gaps in front of, between and behind the non-overlapping ranges."""
    spans = sorted((o, o + ln) for o, ln in o_descs)
    gaps, end = [], 0
    for a, b in spans:
        gaps.append(a - end)
        end = b
    return gaps + [size - end]


def image(size: int, o_descs, wants):
    """-> (the expected buffer, the bytes that are compared).  wants[i]: the
    record's bytes, or None: its own range is not compared."""
    img = np.full(size, SENT, dtype=np.uint8)
    care = np.ones(size, dtype=bool)
    for (o, ln), w in zip(o_descs, wants):
        if w is None:
            care[o:o + ln] = False
        else:
            assert len(w) == ln
            img[o:o + ln] = np.frombuffer(bytes(w), dtype=np.uint8) if not isinstance(w, np.ndarray) else w
    return img, care


def assert_image(got: np.ndarray, img: np.ndarray, care: np.ndarray, o_descs, what):
    assert got.size == img.size
    bad = np.flatnonzero((got != img) & care)
    if bad.size:
        b = int(bad[0])
        inside = [i for i, (o, ln) in enumerate(o_descs) if o <= b < o + ln]
        where = f"byte {b - o_descs[inside[0]][0]} of record {inside[0]}" if inside else "a sentinel byte"
        raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {b}: {where}, "
                             f"{int(got[b]):#x} for {int(img[b]):#x}")


# ---- the device side (torch is imported where a GPU test calls) --------------------
def to_device(blob: bytes, shift: int):
    """The blob in HBM, its first byte `shift` bytes into a dword."""
    import torch
    buf = torch.full((len(blob) + 8,), FILL, dtype=torch.uint8, device="cuda")
    view = buf[shift:shift + len(blob)]
    view.copy_(torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()))
    assert view.data_ptr() % 4 == shift
    return view


def sentinel_buffer(size: int):
    import torch
    out = torch.full((size,), SENT, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    return out


def dev_pairs(descs):
    import torch
    return torch.tensor([v for d in descs for v in d], dtype=torch.int64, device="cuda")


def decode_records_call(codec, comp, c_descs, out, o_descs, with_status=True):
    """snappy_amd_decompress_records_device, sync = 1 -> (rc, statuses; 77 where unwritten)"""
    import torch
    import snappy_amd
    count = len(c_descs)
    status = torch.full((max(count, 1),), 77, dtype=torch.int32, device="cuda")
    c_ol, o_ol = dev_pairs(c_descs), dev_pairs(o_descs)
    codec._bind_stream()
    rc = snappy_amd.lib().snappy_amd_decompress_records_device(
        codec._h, ctypes.c_void_p(comp.data_ptr()), comp.numel(), ctypes.c_void_p(c_ol.data_ptr()), count,
        ctypes.c_void_p(out.data_ptr()), out.numel(), ctypes.c_void_p(o_ol.data_ptr()),
        ctypes.c_void_p(status.data_ptr()) if with_status else None, 1)
    torch.cuda.synchronize()
    return rc, status.cpu().numpy()[:count]
