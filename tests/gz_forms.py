"""The compressed forms of a text input that the library reads (csrc/ps_inflate.h), made with Python's zlib: plain gzip at a given
level, several members, a member header with every optional field, BGZF written from the specification (SAMv1 4.1: raw-deflate
blocks of at most 0xff00 bytes under an 18-byte header with the BC subfield, and the 28-byte end marker), and BGZF blocks followed
by a plain member.  Shared by tests/test_parser_gzip_cpu.py and tests/test_gpu_gzip_input.py."""
import gzip
import struct
import zlib

BGZF_EOF = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def _deflate(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def gz(data, level=6):
    return gzip.compress(data, level, mtime=0)


def members(data, cuts):
    """one member per span between the byte offsets `cuts` (an offset named twice gives an empty member)"""
    at = [0] + sorted(cuts) + [len(data)]
    return b"".join(gz(data[a:b]) for a, b in zip(at, at[1:]))


def full_header(data, level=6):
    """FEXTRA (two subfields, neither of them BC), FNAME, FCOMMENT and FHCRC, all set"""
    extra = b"XY" + struct.pack("<H", 3) + b"abc" + b"Zz" + struct.pack("<H", 0)
    head = bytes([31, 139, 8, 2 | 4 | 8 | 16, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", len(extra)) + extra + b"reads.fq\0" + b"a comment\0"
    head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + _deflate(data, level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def bgzf_block(data, level=6):
    assert len(data) <= 0xff00
    body = _deflate(data, level)
    total = 18 + len(body) + 8
    assert total <= 65536
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", total - 1) + body
            + struct.pack("<II", zlib.crc32(data), len(data)))


def bgzf(data, level=6, block=0xff00, eof=True):
    return b"".join(bgzf_block(data[a:a + block], level) for a in range(0, len(data), block)) + (BGZF_EOF if eof else b"")


def bgzf_then_gz(data, level=6):
    """BGZF blocks (end marker included) for the first part, one plain member for the rest: cut inside a block's worth, not at a record"""
    cut = len(data) * 3 // 5 + 7
    return bgzf(data[:cut], level) + gz(data[cut:], level)


FORMS = {
    "gz1": lambda d: gz(d, 1), "gz6": lambda d: gz(d, 6), "gz9": lambda d: gz(d, 9), "gz0": lambda d: gz(d, 0),
    "members": lambda d: members(d, [len(d) // 7 + 3, len(d) // 3 + 1, len(d) // 3 + 1, len(d) * 4 // 5 + 5]),      # five members, the third empty
    "header": full_header,
    "bgzf": bgzf,
    "bgzf_gz": bgzf_then_gz,
}


def forms(data):
    """name -> bytes of every valid form"""
    return {name: make(data) for name, make in FORMS.items()}
