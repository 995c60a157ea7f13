"""What the BGZF compression tests share (test_deflate_cpu.py, test_gpu_bgzf.py): the edge inputs, the zlib oracle for a run of
BGZF members, and the host build of the encoder (tests/deflate_check.cpp)."""
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
BLK = 0xff00
FIB = [1, 1]
while len(FIB) < 22:
    FIB.append(FIB[-1] + FIB[-2])              # 22 counts, sum 46,367: a plain Huffman tree over them is 21 deep


def edge_inputs():
    """name -> bytes, seeded: the smallest shapes at which the encoder can go wrong"""
    rng = np.random.default_rng(0xB62F)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    nib = lambda n: rng.integers(0, 16, n, dtype=np.uint8).tobytes()           # 4 bits of entropy per byte: dynamic Huffman wins
    out = {}
    for n in (0, 1, 2, 3, 4):
        out["n%d" % n] = rand(n)                                                # below and at the minimum match
    for n in (BLK - 1, BLK, BLK + 1):
        out["nib%d" % n] = nib(n)                                               # one block, then two
    out["three_blocks_17"] = nib(3 * BLK + 17)
    for n in (257, 258, 259, 260, BLK):
        out["rep%d" % n] = b"\x41" * n                                          # overlapping copies, the 258 cap and its chaining
    for p in (2, 3, 4):
        out["period%d" % p] = (bytes(range(97, 97 + p)) * 2000)[:5001]
    c = rand(32768)
    out["dist32768"] = c + c                                                    # the copy is exactly 32768 back
    c = rand(32769)
    out["dist32769"] = c + c[:4000]                                             # the nearest copy is one too far
    out["random_block"] = rand(BLK)
    out["all256"] = bytes(range(256))
    fib = np.concatenate([np.full(f, 40 + i, dtype=np.uint8) for i, f in enumerate(FIB)])
    shuffled = fib.copy()
    rng.shuffle(shuffled)
    out["fib_shuffled"] = shuffled.tobytes()
    # the same bytes in runs of rising length: almost everything is a match of length 258 at a short distance, a few literals per
    # value remain, and most of the 316 code lengths are zero -- the other arrangement of the code-length alphabet.  (Neither
    # arrangement reaches a depth limit through the matcher: deflate_check prints plain depths of 14 / 12 / 5 and 9 / 4 / 5.
    # runs_cl_depth8 below reaches the 7-bit limit; no input found reaches the 15-bit one, see test_deflate_cpu.py.)
    out["fib_runs"] = fib.tobytes()
    # runs of 1 to 599 equal bytes of random values: about 400 literal values are used a few times each, the matches are of many
    # lengths, and the code lengths that come of it are spread so unevenly that the plain tree of the code-length alphabet is
    # 8 deep: the limit to 7 is reached inside a real block (test_deflate_cpu.py asserts the depth deflate_check reports)
    r = np.random.default_rng(1)
    out["runs_cl_depth8"] = np.repeat(r.integers(0, 256, 400).astype(np.uint8), r.integers(1, 600, 400)).tobytes()[:BLK]
    # 64 bytes over two values: one chunk, so no match at all, and dynamic Huffman wins: a dynamic block without a distance symbol
    out["two_values_64"] = bytes(r.integers(0, 2, 64).astype(np.uint8) + 0x41)
    return out


def members(raw):
    """the gzip members of a BGZF byte string, cut by BSIZE"""
    out, at = [], 0
    while at < len(raw):
        assert raw[at:at + 4] == b"\x1f\x8b\x08\x04" and raw[at + 10:at + 16] == b"\x06\x00BC\x02\x00", at
        bsize = struct.unpack_from("<H", raw, at + 16)[0] + 1
        assert at + bsize <= len(raw)
        out.append(raw[at:at + bsize])
        at += bsize
    return out


def btype(member):
    return (member[18] >> 1) & 3


def check_members(raw, data):
    """zlib as the oracle: every member at most 65536 bytes, its payload one complete raw DEFLATE stream that inflates to the next
    at most 0xff00 bytes of data, CRC32 and ISIZE right; returns the members"""
    ms = members(raw)
    assert len(ms) == (len(data) + BLK - 1) // BLK
    for k, m in enumerate(ms):
        want = data[k * BLK:(k + 1) * BLK]
        assert len(m) <= 65536 and len(m) <= len(want) + 5 + 26
        d = zlib.decompressobj(-15)
        got = d.decompress(m[18:-8])
        assert d.eof and d.unused_data == b"" and got == want, k
        assert struct.unpack("<II", m[-8:]) == (zlib.crc32(want), len(want)), k
    return ms


def build_check(where, sanitize):
    """tests/deflate_check.cpp built by the host compiler from ps_deflate.h alone"""
    exe = os.path.join(str(where), "deflate_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.check_call([os.environ.get("CXX", "c++")] + flags + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC,
                                                                     os.path.join(ROOT, "tests", "deflate_check.cpp"), "-o", exe])
    return exe


def host_members(exe, data, where, mode="all"):
    """the host build's members of data and, per block, (BTYPE, stream bytes, depth of the three plain Huffman trees)"""
    src, dst = os.path.join(str(where), "in.bin"), os.path.join(str(where), "out.bgzf")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, src, dst, mode], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return open(dst, "rb").read(), [tuple(int(x) for x in l.split()) for l in r.stdout.splitlines()]


def zlib1_size(data):
    """what the library writes without the switch at level 1: zlib on the same block cuts, 26 bytes around every stream"""
    total = 0
    for at in range(0, len(data), BLK):
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        total += len(c.compress(data[at:at + BLK]) + c.flush()) + 26
    return total
