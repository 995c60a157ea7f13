"""Records for the coordinate sort's tests (ps_bam_sort_records): BAM records as far as the sort reads them -- block_size, ref and
pos in place, the rest of the bytes drawn -- and the order Python's own sorted() gives them, which is stable as the library's is."""
import struct

import numpy as np


def record(ref, pos, length, rng):
    """one record of `length` bytes in all (block_size first, at least 36)"""
    assert length >= 36
    return struct.pack("<iii", length - 4, ref, pos) + rng.integers(0, 256, length - 12, dtype=np.uint8).tobytes()


def python_sorted(records):
    """the third opinion: (ref as an unsigned number, pos as a signed one), input order among equals"""
    return b"".join(sorted(records, key=lambda r: (struct.unpack_from("<I", r, 4)[0], struct.unpack_from("<i", r, 8)[0])))


def mixed_lengths(n, rng):
    """lengths from 36 to 900, the short ones common; every residue mod 16 comes up within a few dozen records"""
    return [int(v) for v in np.where(rng.random(n) < 0.7, rng.integers(36, 260, n), rng.integers(36, 901, n))]


def random_records(n, rng, n_refs=5, unplaced=0.1, big_at=None):
    """n records with mixed lengths over a few references with many ties; a share of them unplaced (ref -1, pos -1), scattered;
    big_at: the index of one record of 70,000 bytes"""
    out = []
    lens = mixed_lengths(n, rng)
    for i in range(n):
        ref, pos = (-1, -1) if rng.random() < unplaced else (int(rng.integers(0, n_refs)), int(rng.integers(0, 400)))
        out.append(record(ref, pos, 70000 if i == big_at else lens[i], rng))
    return out
