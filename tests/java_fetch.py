"""FetchSequencesForBindingSites.fetchSequences and FetchSequencesForBEDFile.fetchSequences (the toolkit's
utils/pileupclusters/FetchSequencesForBindingSites.java:18-95 and FetchSequencesForBEDFile.java:17-99, the `fetch` and `fetchBed`
modes) restated in plain Python, one line at a time as the Java walks them: test infrastructure, the yardstick
ps_fetch_sequences is held to (tests/test_fetch_cpu.py works its answers out by hand against this file,
tests/test_gpu_fetch.py holds the library to it).  No JVM is at hand, so this is the Java as it is written, read line by
line, not pinned to the jar.

The bases come from the FASTA TEXT -- a contig is the graphic characters (0x21-0x7E) of its body lines, its name the first word
of its header -- and never from the index (.pac, .ann), which the library reads: the two meet only in the output.

fetch(fasta_text, sites_bytes, bed) returns (the bytes of the output file, the integer counters of ps_fetch_stats but
n_pieces).  Where include/parasuite_hip.h has the library fail -- an empty sites file, a data line with too few fields, a
start or end Integer.parseInt refuses -- this raises FetchError naming the 1-based line.  IndexedFastaSequenceFile
.getSubsequenceAt (htsjdk 1.128) throws a SAMException, which both classes catch and turn into an empty sequence, for
start > end + 1 (in Java ints), a contig it does not know and end > contig length, in this order; a start before base 1 is
empty too, by the library's rule (htsjdk would read bytes before the contig)."""
from java_benchmark import NumberFormatException, i32, java_split, parse_int, read_lines

INT_KEYS = ("n_lines", "n_sites", "n_reverse", "n_bases", "n_hole_bases", "n_inverted", "n_no_contig", "n_past_end", "n_before_start")
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


class FetchError(Exception):
    pass


def read_fasta(text):
    """contig name -> bases, from FASTA text (bytes); a name that comes twice keeps its first sequence"""
    contigs, name, body = {}, None, []
    for line in text.split(b"\n") + [b">"]:
        if line.startswith(b">"):
            if name is not None:
                contigs.setdefault(name, bytes(c for c in b"".join(body) if 0x21 <= c <= 0x7E))
            words = line[1:].split()
            name, body = (words[0] if words else b""), []
        elif name is not None:
            body.append(line)
    return contigs


def subsequence(contigs, chrom, start, end, st):
    """getSubsequenceAt(chrom, start, end).getBases(), or b"" where it throws; the reason is counted in st"""
    if start > i32(end + 1):
        st["n_inverted"] += 1
    elif chrom not in contigs:
        st["n_no_contig"] += 1
    elif end > len(contigs[chrom]):
        st["n_past_end"] += 1
    elif start < 1:
        st["n_before_start"] += 1
    else:
        return contigs[chrom][start - 1:end]
    return b""


def reverse_complement(seq):
    """SequenceUtil.reverseComplement: A, C, G, T of either case swapped, everything else kept"""
    return seq[::-1].translate(_COMPLEMENT)


def fetch(fasta_text, sites, bed):
    contigs = read_fasta(fasta_text)
    st = dict.fromkeys(INT_KEYS, 0)
    lines = read_lines(sites)
    if not lines:
        raise FetchError("the sites file is empty")
    out = [lines[0] + b"\n"]                                  # :26-28, in both classes
    st["n_lines"], st["n_sites"] = len(lines), len(lines) - 1
    for k, line in enumerate(lines[1:]):
        f = java_split(line, b"\t")
        if len(f) < (5 if bed else 12):
            raise FetchError("line %d has %d fields" % (k + 2, len(f)))
        c = 0 if bed else 1
        chrom = f[c]
        if bed and not chrom.startswith(b"chr"):
            chrom = b"chr" + chrom
        try:
            start, end = parse_int(f[c + 1]), parse_int(f[c + 2])
        except NumberFormatException:
            raise FetchError("line %d: start or end is not an int" % (k + 2))
        reverse = f[4] == b"-"
        st["n_reverse"] += reverse
        seq = subsequence(contigs, chrom, start, end, st)
        st["n_hole_bases"] += sum(1 for b in seq if b not in b"ACGTacgt")
        if reverse:
            seq = reverse_complement(seq)
        seq = seq.upper()
        st["n_bases"] += len(seq)
        if bed:
            out.append(b">" + f[3] + b"\n" + seq + b"\n")
        else:
            f[11] = seq
            out.append(b"\t".join(f) + b"\n")
    return b"".join(out), st
