"""Records for the name sort's tests (ps_bam_name_sort_records): BAM records as far as the sort reads them -- block_size, the name's
length at byte 12, the flag at byte 18, the name with its NUL at byte 36, the rest of the bytes drawn -- and two plain restatements:
the samtools rule as a comparator (digit runs compare as numbers), under Python's own sorted(), which is stable as the library's
sort is; and the row of csrc/ps_namesort.h, from which a test derives how many columns a call has to sort."""
import functools
import struct

import numpy as np


def record(name, flag, length, rng):
    """one record of `length` bytes in all (at least 36 + the name + its NUL), name: bytes without a NUL"""
    assert length >= 37 + len(name) and len(name) <= 254 and 0 not in name
    body = bytearray(rng.integers(0, 256, length - 4, dtype=np.uint8).tobytes())
    body[8] = len(name) + 1
    body[14:16] = struct.pack("<H", flag)
    body[32:32 + len(name) + 1] = name + b"\0"
    return struct.pack("<i", length - 4) + bytes(body)


def name_of(rec):
    return rec[36:36 + rec[12] - 1]


def flag_of(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def _digit(c):
    return 0x30 <= c <= 0x39


def name_cmp(a, b):
    """`samtools sort -n`: where both names have a digit, the two runs compare as numbers (leading zeros dropped, the longer
    one is larger, then digit by digit); anywhere else byte against byte; a name that ends first is smaller"""
    i = j = 0
    while i < len(a) and j < len(b):
        if _digit(a[i]) and _digit(b[j]):
            while i < len(a) and a[i] == 0x30:
                i += 1
            while j < len(b) and b[j] == 0x30:
                j += 1
            ei, ej = i, j
            while ei < len(a) and _digit(a[ei]):
                ei += 1
            while ej < len(b) and _digit(b[ej]):
                ej += 1
            if ei - i != ej - j:
                return -1 if ei - i < ej - j else 1
            if a[i:ei] != b[j:ej]:
                return -1 if a[i:ei] < b[j:ej] else 1
            i, j = ei, ej
        else:
            if a[i] != b[j]:
                return -1 if a[i] < b[j] else 1
            i += 1
            j += 1
    return 1 if i < len(a) else (-1 if j < len(b) else 0)


def record_cmp(x, y):
    c = name_cmp(name_of(x), name_of(y))
    return c if c else ((flag_of(x) >> 6) & 3) - ((flag_of(y) >> 6) & 3)          # first of pair before second


def python_sorted(records):
    """the third opinion: the rule above, then the pair bits, input order among equals"""
    return b"".join(sorted(records, key=functools.cmp_to_key(record_cmp)))


def key_words(longest):
    return (2 * longest + 3 + 3) // 4


def row(name, flag, W):
    """the row of W big-endian words: the key zero padded, the pair bits in the last byte"""
    key = bytearray()
    i = 0
    while i < len(name):
        if not _digit(name[i]):
            key.append(name[i])
            i += 1
            continue
        e = i
        while e < len(name) and _digit(name[e]):
            e += 1
        digits = name[i:e].lstrip(b"0")
        key += bytes([0x30, len(digits)]) + digits
        i = e
    assert len(key) <= 4 * W - 2
    key += bytes(4 * W - 1 - len(key)) + bytes([(flag >> 6) & 3])
    return struct.unpack(">%dI" % W, bytes(key))


def columns_that_differ(records):
    """(W, the number of columns in which two rows differ) of one call over these records"""
    W = key_words(max(len(name_of(r)) for r in records))
    rows = [row(name_of(r), flag_of(r), W) for r in records]
    return W, sum(1 for w in range(W) if len({r[w] for r in rows}) > 1)


_POOL = [b"r", b"r", b"read", b"a", b"ab", b"0", b"00", b"1", b"7", b"9", b"10", b"099", b"123456", b"/", b".", b":", b"-", b"_", b"#", b"+", b"\x7f", b"\x80", b"\xc3\xa9", b"\xff"]


def random_name(rng, max_len=40):
    """pieces of the pool strung together: digits next to separators, leading zeros, high bytes; many names come up more than once"""
    out = b""
    for _ in range(int(rng.integers(0, 7))):
        out += _POOL[int(rng.integers(0, len(_POOL)))]
    return out[:max_len]


def random_records(n, rng, lengths=None):
    """n records with names from random_name, any flag, and the given lengths (a name that needs more room gets it)"""
    out = []
    for i in range(n):
        name = random_name(rng)
        out.append(record(name, int(rng.integers(0, 4096)), max(37 + len(name), lengths[i] if lengths else 37 + len(name) + int(rng.integers(0, 60))), rng))
    return out
