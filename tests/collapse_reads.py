"""Reads for the collapsed-search tests (tests/test_collapse_cpu.py, tests/test_gpu_collapse.py): the pairs the grouping rule of
csrc/ps_collapse.h must keep apart, duplicated sets with stated multiplicities, the reference grouping (a dict keyed on length
and sequence text), and a FASTQ writer that gives every copy its own name and qualities."""
import numpy as np

_COMP = str.maketrans("ACGTN", "TGCAN")


def random_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def adversarial_reads(rng):
    """every read here is a different read, and each kind shares its packed words, or its bases, with its partner:
    a 30-base read and the 36-base read that continues it with As (bits behind a read's end are zero, A is code 0);
    A against N at bases 15, 16, 31 and 32 (an N is packed as a base code; 16 bases and 32 flags per word);
    a read and its reverse complement"""
    out = []
    x = random_seq(rng, 29) + "C"
    out += [x, x + "AAAAAA"]
    for p in (15, 16, 31, 32):
        r = random_seq(rng, 40)
        out += [r[:p] + "A" + r[p + 1:], r[:p] + "N" + r[p + 1:]]
    x = random_seq(rng, 40)
    while x == revcomp(x):
        x = random_seq(rng, 40)
    out += [x, revcomp(x)]
    return out


def with_multiplicities(distinct, mult, rng):
    """distinct[i] repeated mult[i] times, shuffled"""
    assert len(distinct) == len(mult)
    seqs = [s for s, m in zip(distinct, mult) for _ in range(m)]
    return [seqs[i] for i in rng.permutation(len(seqs))]


def groups_of(seqs):
    """the reference grouping: (length, sequence text) -> the indices of its copies, ascending"""
    g = {}
    for i, s in enumerate(seqs):
        g.setdefault((len(s), s), []).append(i)
    return g


def partition(rep_of):
    """the grouping a representative index states, as a set of index tuples"""
    g = {}
    for i, r in enumerate(rep_of):
        g.setdefault(int(r), []).append(i)
    return {tuple(v) for v in g.values()}


def check_groups_exact(seqs, rep_of):
    """every group is exact: the representative is a member (it names itself) and every member is the same read"""
    for i, r in enumerate(rep_of):
        r = int(r)
        assert 0 <= r < len(seqs) and int(rep_of[r]) == r, (i, r)
        assert seqs[i] == seqs[r], (i, r)


def write_fastq(path, seqs, rng):
    """every copy its own name and its own qualities: what makes duplicates differ comes after the search"""
    with open(path, "w") as f:
        for i, s in enumerate(seqs):
            q = "".join(chr(33 + v) for v in rng.integers(3, 41, len(s)))
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, q))
    return path
