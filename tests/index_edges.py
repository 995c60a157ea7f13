"""Edge texts for the index builder, the Occ addressing and the locate stage, with a third opinion on their index: a plain
sort of the suffixes (tests/test_index_edges_cpu.py: the oracle against it; tests/test_gpu_index_edges.py: the library
against both).  Nothing here calls the oracle or the library.

The fixture genomes are ordinary text: a handful of ties after round 0 of the suffix sorter, `primary` somewhere in the middle,
lengths that fall on a layout boundary only by chance, no read on the forward/reverse junction.  TEXTS aims at exactly those
places (every text at most 8192 bases, so seq_len <= 16384):
  * lengths around the 28-symbol key of round 0, the 32-row SA sample, the 192-symbol Occ block and the 4096-symbol tile of
    k_collect;
  * one or two symbols only (empty chunks in round 0; `primary` 1 or seq_len);
  * periodic texts, duplicated texts and texts that are their own reverse complement (T = fwd || revcomp(fwd) becomes a square):
    most of the text is still tied after round 0 and the doubling rounds run ~log2(n / 28) times;
  * N runs at both ends (the lrand48 fill), two contigs.

Text convention (index_props.py): n = 2 * l_pac, T$ has rows 0..n, SA[0] = n, `primary` = the row whose
SA is 0, the stored BWT leaves that row out."""
import numpy as np

BASES = "ACGT"
_COMP = str.maketrans("ACGT", "TGCA")
SA_INTV = 32
BLK_SYMS = 192
KEY_SYMS = 28                      # symbols that round 0 of the suffix sorter orders by


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _rand(rng, n, alphabet=BASES):
    return "".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), n))


class EdgeText:
    def __init__(self, name, contigs, kind):
        self.name = name
        self.contigs = contigs                     # [(contig name, ASCII string)]; may hold N
        self.kind = kind                           # "random": no repeat longer than chance allows

    @property
    def ascii(self):
        return "".join(s for _, s in self.contigs)

    @property
    def l_pac(self):
        return len(self.ascii)

    @property
    def has_n(self):
        return "N" in self.ascii

    def write_fasta(self, path, width=60):
        with open(path, "w") as f:
            for cname, s in self.contigs:
                f.write(">" + cname + "\n")
                for i in range(0, len(s), width):
                    f.write(s[i:i + width] + "\n")

    def __repr__(self):
        return "EdgeText(%s, %d)" % (self.name, self.l_pac)


RANDOM_LENGTHS = (1, 2, 13, 14, 15, 16, 17, 48, 96, 97, 2016, 2047, 2048, 2049, 4096)


def _make_texts():
    out = []
    for n in RANDOM_LENGTHS:                       # seq_len 26/28/30 around the key, multiples of 32, 192, 21 * 192, 4094/4096/4098, 8192
        out.append(EdgeText("rand%d" % n, [("r%d" % n, _rand(np.random.default_rng(0xED6E0000 + n), n))], "random"))
    for sym, n in (("A", 300), ("T", 300), ("C", 96), ("G", 97)):       # two empty chunks each; primary 1 / seq_len
        out.append(EdgeText("%s%d" % (sym, n), [("mono" + sym, sym * n)], "periodic"))
    out.append(EdgeText("AC1024", [("ac", "AC" * 1024)], "periodic"))
    out.append(EdgeText("ACGT1024", [("acgt", "ACGT" * 1024)], "periodic"))          # its own reverse complement: T = (ACGT)^2048
    x = _rand(np.random.default_rng(0xED6E1001), 1500)
    out.append(EdgeText("x_rcx", [("xrcx", x + revcomp(x))], "repeat"))                # its own reverse complement: T = (x rc(x))^2
    out.append(EdgeText("unit37x80", [("tandem", _rand(np.random.default_rng(0xED6E1002), 37) * 80)], "periodic"))
    out.append(EdgeText("x_x", [("xx", x + x)], "repeat"))
    out.append(EdgeText("x_x_two_contigs", [("xa", x), ("xb description", x)], "repeat"))
    out.append(EdgeText("noCG3000", [("at", _rand(np.random.default_rng(0xED6E1003), 3000, "AT"))], "two_symbols"))
    out.append(EdgeText("nruns2000", [("nn", "N" * 100 + _rand(np.random.default_rng(0xED6E1004), 1800) + "N" * 100)], "n_runs"))
    assert all(t.l_pac <= 8192 for t in out) and len({t.name for t in out}) == len(out)
    return out


TEXTS = _make_texts()
TEXT_BY_NAME = {t.name: t for t in TEXTS}
NAMES = [t.name for t in TEXTS]


def codes_of(s):
    """ACGT string -> codes 0..3 (4 for anything else)"""
    lut = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
        lut[ch | 0x20] = i
    return lut[np.frombuffer(s.encode(), dtype=np.uint8)]


def string_of(codes):
    return "".join(BASES[int(c)] for c in codes)


def unpack_pac(pac, l_pac):
    """forward codes out of a packed text (four bases per byte, the first in the high bits)"""
    pac = np.asarray(pac, dtype=np.uint8)
    i = np.arange(l_pac, dtype=np.int64)
    return ((pac[i >> 2] >> ((~i & 3) << 1)) & 3).astype(np.uint8)


def assert_pac_matches_fasta(fwd_codes, text):
    """the packed text is the FASTA wherever the FASTA holds a base (an N position holds a drawn one)"""
    want = codes_of(text.ascii)
    assert fwd_codes.size == want.size
    keep = want < 4
    assert np.array_equal(np.asarray(fwd_codes)[keep], want[keep])


# ------------------------------------------------------------------------------------------------ the plain reference ----
def plain_suffix_array(T):
    """suffix array of T$ (rows 0..n) by sorting the suffixes themselves as byte strings: a shorter prefix sorts first (the '$'
    rule), so row 0 is the empty suffix"""
    tb = np.asarray(T, dtype=np.uint8).tobytes()
    return np.array(sorted(range(len(tb) + 1), key=lambda i: tb[i:]), dtype=np.int64)


class PlainIndex:
    """everything the index holds, derived from the text and a suffix array of it"""

    def __init__(self, fwd_codes, sa=None):
        fwd = np.ascontiguousarray(fwd_codes, dtype=np.uint8)
        assert fwd.size > 0 and int(fwd.max()) < 4
        self.fwd = fwd
        self.l_pac = int(fwd.size)
        self.seq_len = n = 2 * self.l_pac
        self.T = T = np.concatenate([fwd, 3 - fwd[::-1]]).astype(np.uint8)
        self.sa = sa = plain_suffix_array(T) if sa is None else np.asarray(sa, dtype=np.int64)
        assert sa.size == n + 1
        self.primary = int(np.flatnonzero(sa == 0)[0])
        rows = np.flatnonzero(sa != 0)                                  # the '$' row is not stored
        self.bwt = T[sa[rows] - 1]
        cnt = np.bincount(T, minlength=4)[:4]
        self.L2 = [0] + [int(v) for v in np.cumsum(cnt)]
        onehot = np.stack([self.bwt == c for c in range(4)], axis=1).astype(np.int64)
        pre = np.concatenate([np.zeros((1, 4), dtype=np.int64), np.cumsum(onehot, axis=0)])
        self.n_blocks = n // BLK_SYMS + 1
        self.occ_blocks = pre[np.minimum(np.arange(self.n_blocks, dtype=np.int64) * BLK_SYMS, n)]    # Occ at every block boundary
        self.n_sa = (n + SA_INTV) // SA_INTV

    # the accessors test_gpu_parity._check_index asks an oracle index for
    def bwt_syms(self):
        return self.bwt

    def sa_samples(self):
        out = self.sa[::SA_INTV].astype(np.uint64)
        out[0] = np.uint64(0xFFFFFFFFFFFFFFFF)                            # row 0, the empty suffix: stands for -1
        assert out.size == self.n_sa
        return out

    def pac(self):
        out = np.zeros(self.l_pac // 4 + 1, dtype=np.uint8)
        i = np.arange(self.l_pac, dtype=np.int64)
        np.bitwise_or.at(out, i >> 2, (self.fwd << ((~i & 3) << 1)).astype(np.uint8))
        return out

    def lcp(self):
        """lcp[r] = common prefix of the suffixes of rows r - 1 and r (Kasai); lcp[0] = 0"""
        n, sa = self.seq_len, self.sa
        tb = self.T.tobytes()
        rank = np.empty(n + 1, dtype=np.int64)
        rank[sa] = np.arange(n + 1)
        rank, sal = rank.tolist(), sa.tolist()
        lcp = [0] * (n + 1)
        h = 0
        for i in range(n):
            j = sal[rank[i] - 1]                                          # rank[i] >= 1: row 0 is the empty suffix
            while i + h < n and j + h < n and tb[i + h] == tb[j + h]:
                h += 1
            lcp[rank[i]] = h
            if h:
                h -= 1
        return np.array(lcp, dtype=np.int64)

    def longest_repeat(self):
        """the longest common prefix of two suffixes of the text"""
        return int(self.lcp().max())

    def min_sa_rounds(self):
        """rounds the tie-only prefix doubling cannot do without: round 0 orders by KEY_SYMS symbols, the round with offset h
        by 2h, h = KEY_SYMS, 2 KEY_SYMS, ...; two suffixes with a common prefix of L symbols stay tied while 2h <= L"""
        L = self.longest_repeat()
        if L < KEY_SYMS:
            return 1
        return 2 + int(np.floor(np.log2(L / KEY_SYMS)))


def plain_index(fwd):
    """fwd: ACGT string or codes 0..3"""
    return PlainIndex(codes_of(fwd) if isinstance(fwd, str) else fwd)


def assert_index_equals_plain(plain, seq_len, primary, L2, bwt, sa_samples):
    """an index's numbers against the plain reference; SA sample 0 (the empty suffix) is never asked for"""
    assert int(seq_len) == plain.seq_len, "seq_len"
    assert int(primary) == plain.primary, "primary %d, plain sort %d" % (int(primary), plain.primary)
    assert [int(v) for v in L2] == plain.L2, "L2"
    bwt = np.asarray(bwt)
    assert bwt.size == plain.bwt.size, "BWT length"
    bad = np.flatnonzero(bwt != plain.bwt)
    assert bad.size == 0, "BWT differs at stored symbols %s" % bad[:5].tolist()
    sa_samples = np.asarray(sa_samples, dtype=np.uint64)
    ref = plain.sa_samples()
    assert sa_samples.size == ref.size, "number of SA samples"
    bad = np.flatnonzero(sa_samples[1:] != ref[1:]) + 1
    assert bad.size == 0, "SA samples differ at entries %s" % bad[:5].tolist()


# -------------------------------------------------------------------------------------------------------- edge reads ----
N_WINDOWS = 110
JUNCTION_EXACT, JUNCTION_SUB = "jx", "js"        # read name prefixes


def _other(rng, base):
    return BASES[(BASES.index(base) + 1 + int(rng.integers(0, 3))) & 3]


def edge_reads(fwd, seed):
    """FASTQ text: windows of 36 and 50 bases from either strand (0-2 substitutions, one in six with a 1-base insertion or
    deletion at least 8 bases from either end), windows flush with the ends of the text, reads as long as the text and longer,
    an all-N read, and reads across the forward/reverse junction (the last k bases of fwd + the first L - k of its reverse
    complement; names JUNCTION_EXACT* exact, JUNCTION_SUB* with one substitution)"""
    assert fwd and set(fwd) <= set(BASES)
    rng = np.random.default_rng(seed)
    rc = revcomp(fwd)
    T = fwd + rc
    n = len(fwd)
    reads = []

    def add(name, seq):
        if seq:
            reads.append((name, seq))

    for L in (36, 50):
        if n >= L:
            for w in range(N_WINDOWS):
                strand = int(rng.integers(0, 2))
                p = int(rng.integers(0, n - L + 1))
                s = list((fwd, rc)[strand][p:p + L])
                for _ in range(int(rng.integers(0, 3))):
                    q = int(rng.integers(0, L))
                    s[q] = _other(rng, s[q])
                tag = "s"
                if w % 6 == 5:
                    if int(rng.integers(0, 2)):
                        s.insert(int(rng.integers(8, L - 8 + 1)), BASES[int(rng.integers(0, 4))])
                        tag = "i"
                    else:
                        del s[int(rng.integers(8, L - 8))]
                        tag = "d"
                add("w%d_%d_%s%s%d" % (L, w, tag, "fr"[strand], p), "".join(s))
            for strand, src in enumerate((fwd, rc)):                      # flush with either end of the strand
                add("e%d_%s_first" % (L, "fr"[strand]), src[:L])
                add("e%d_%s_last" % (L, "fr"[strand]), src[n - L:])
            for k in (1, 5, L // 2, L - 1):
                j = fwd[n - k:] + rc[:L - k]
                add("%s%d_k%d" % (JUNCTION_EXACT, L, k), j)
                q = L // 3
                add("%s%d_k%d" % (JUNCTION_SUB, L, k), j[:q] + _other(rng, j[q]) + j[q + 1:])
        else:
            add("%s%d_T" % (JUNCTION_EXACT, L), T)
            add("%s%d_T1" % (JUNCTION_EXACT, L), T[1:])
    if n < 50:
        add("whole", fwd)
        add("whole_rc", rc)
        add("minus2", fwd[:-2])
        add("repeated36", (fwd * 36)[:36])
        add("polyA36", "A" * 36)
        add("T_plus6", T + (T * 6)[:6])
    add("allN", "N" * 36)
    return "".join("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq)) for name, seq in reads)


def sam_counts(records):
    """(mapped, unmapped, gapped, with XA:Z:) of SAM alignment lines"""
    mapped = unmapped = gapped = xa = 0
    for l in records:
        f = l.split("\t")
        if int(f[1]) & 4:
            unmapped += 1
        else:
            mapped += 1
            if "I" in f[5] or "D" in f[5]:
                gapped += 1
        if "\tXA:Z:" in l:
            xa += 1
    return mapped, unmapped, gapped, xa


def profile_matrix():
    """the suite's profile options: EXAMPLE_PROFILE with T->C 0.12; insertion rate 2.1e-5, deletion rate 5.9e-4, -X -1"""
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    return P


INS_RATE, DEL_RATE, X_ARG = 2.1e-5, 5.9e-4, -1
