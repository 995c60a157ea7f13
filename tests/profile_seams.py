"""Inputs that put ps_error_profile_full and ps_error_profile on the seams of their own layout (csrc/ps_profile.hip), shared
by tests/test_profile_seams_cpu.py and tests/test_gpu_profile_seams.py:

  B1  k_qual_sd: chunks of 224 records, blocks of 64 read positions; n in {1, 223, 224, 225, 448, 449} records at
      max_read_len 64, 65 and 129, with records that book nothing (unmapped, QUAL '*'), and one file whose first 224
      records are all unmapped
  B2  k_profile: 2,048 blocks of 256 lanes, so lane 0 takes a second record at 524,289 records
  B3  the largest max_read_len of each entry (2,028 with -q, 2,254 without, 2,275 for ps_error_profile) and one more

Everything is built here from seeded generators over a reference this module makes itself.  Test infrastructure, not
product code."""
import random

import java_errorprofile as J

_rng = random.Random(31)
S1 = "".join(_rng.choice("ACGT") for _ in range(600))
G1 = "".join(_rng.choice("ACGT") for _ in range(2300))
REF = {"s1": S1.encode(), "g1": G1.encode()}
FA = ">s1\n%s\n>g1\n%s\n" % (S1, "\n".join(G1[i:i + 100] for i in range(0, 2300, 100)))
HEADER = "@SQ\tSN:s1\tLN:600\n@SQ\tSN:g1\tLN:2300\n"
QUALS = (2, 11, 25, 37, 41)                                                   # as order_records of test_error_profile_full_cpu


def sam_text(records):
    return HEADER + "".join("%s\t%d\t%s\t%d\t37\t%s\t*\t0\t0\t%s\t%s\n" % r for r in records)


# ---- B1

B1_N = (1, 223, 224, 225, 448, 449)
B1_MAX = (64, 65, 129)


def b1_records(n, max_len, lead_unmapped=0):
    """n records over s1: lengths from {1, 63, 64, 65, max - 1, max} or uniform in 1..max, both strands, a mismatch in
    every third; every 40th record unmapped and every 50th with QUAL '*' (both book nothing in .qualities); the first
    lead_unmapped records unmapped"""
    rng = random.Random(7919 * n + max_len + lead_unmapped)
    recs = []
    for r in range(n):
        L = min(max_len, rng.choice((1, 63, 64, 65, max_len - 1, max_len)) if rng.random() < 0.5 else rng.randint(1, max_len))
        pos = rng.randrange(1, 600 - L)
        seq = list(S1[pos - 1:pos - 1 + L])
        if r % 3 == 0:
            seq[rng.randrange(L)] = rng.choice("ACGT")
        qual = "*" if r % 50 == 49 else "".join(chr(33 + rng.choice(QUALS)) for _ in range(L))
        if r % 40 == 39 or r < lead_unmapped:
            recs.append(("q%d" % r, 4, "*", 0, "*", "".join(seq), qual))
        else:
            recs.append(("q%d" % r, 16 if rng.random() < 0.5 else 0, "s1", pos, "%dM" % L, "".join(seq), qual))
    return recs


B1_LEAD = (300, 65, 224)                                                      # n, max_read_len, leading unmapped records

# ---- B2

B2_BLOCKS, B2_LANES, B2_MAX = 2048, 256, 8
B2_N = B2_BLOCKS * B2_LANES + 1                                               # 524,289: the first count with a second grid pass
B2_BLOCK = 1000


def b2_block():
    """1,000 records of 4 bases over s1: 4M, 2M1I1M and 2M1D2M, both strands, some unmapped, some without QUAL"""
    rng = random.Random(524289)
    recs = []
    for r in range(B2_BLOCK):
        pos = rng.randrange(1, 590)
        kind = rng.random()
        if kind < 0.15:
            cig, seq = "2M1I1M", S1[pos - 1:pos + 1] + rng.choice("ACGT") + S1[pos + 1]
        elif kind < 0.3:
            cig, seq = "2M1D2M", S1[pos - 1:pos + 1] + S1[pos + 2:pos + 4]
        else:
            cig, seq = "4M", S1[pos - 1:pos + 3]
        if rng.random() < 0.2:
            seq = seq[:2] + rng.choice("ACGT") + seq[3:]
        qual = "*" if r % 97 == 0 else "".join(chr(33 + rng.choice(QUALS)) for _ in range(4))
        if r % 53 == 52:
            recs.append(("b%d" % r, 4, "*", 0, "*", seq, qual))
        else:
            recs.append(("b%d" % r, 16 if rng.random() < 0.5 else 0, "s1", pos, cig, seq, qual))
    return recs


def b2_text():
    """the first 289 records of the block, then the block 524 times: 524,289 records, about 20 MB"""
    block = b2_block()
    k, rest = divmod(B2_N, B2_BLOCK)
    body = "".join("%s\t%d\t%s\t%d\t37\t%s\t*\t0\t0\t%s\t%s\n" % r for r in block)
    return sam_text(block[:rest]) + body * k


def add_counts(block, k, prefix):
    """k * block + prefix for two results of J.counts without quality lists"""
    def comb(a, b):
        if isinstance(a, list):
            return [comb(x, y) for x, y in zip(a, b)]
        return k * a + b
    out = {key: comb(block[key], prefix[key]) for key in ("conv", "ins", "dele", "qpm_sum", "qpm_cnt")}
    out["qlists"] = block["qlists"]
    assert not any(block["qlists"]) and not any(prefix["qlists"])
    out["st"] = {key: k * v + prefix["st"][key] for key, v in block["st"].items()}
    return out


def b2_expected():
    """(files, stats) of b2_text() from the counts of its two small parts"""
    block = b2_block()
    k, rest = divmod(B2_N, B2_BLOCK)
    total = add_counts(J.counts(sam_text(block), REF, B2_MAX, False), k, J.counts(sam_text(block[:rest]), REF, B2_MAX, False))
    return J.render(total, B2_MAX, False), total["st"]


# ---- B3

B3_LIMITS = {2: 2028, 1: 2254, 0: 2275}                                       # quality mode (-q, no -q, ps_error_profile): largest max_read_len


def b3_records(length):
    """five records of `length` bases over g1 (2,300 bp), both strands, two mismatches each, one with QUAL '*', and a short one"""
    rng = random.Random(length)
    recs = []
    for r in range(5):
        pos = 1 + r * ((2300 - length) // 4)
        seq = list(G1[pos - 1:pos - 1 + length])
        for _ in range(2):
            seq[rng.randrange(length)] = rng.choice("ACGT")
        qual = "*" if r == 3 else "".join(chr(33 + rng.choice(QUALS)) for _ in range(length))
        recs.append(("m%d" % r, 16 if r % 2 else 0, "g1", pos, "%dM" % length, "".join(seq), qual))
    recs.append(("short", 0, "g1", 7, "30M", G1[6:36], "I" * 30))
    return recs
