"""CombineGenomeTranscript.combine (the toolkit's utils/postprocessing/CombineGenomeTranscript.java:36-666) restated in plain
Python, one transcript record at a time as the Java walks them: test infrastructure, the yardstick ps_combine_genome_transcript
is held to (tests/test_combine_cpu.py works its answers out by hand against this file, tests/test_gpu_combine.py holds the
library to it).  No JVM is at hand, so this is the Java as it is written, read line by line, not pinned to the jar.

Records are dicts as the independent BAM reader of tests/test_bam.py returns them (name, flag, ref, pos 0-based, mapq, bin,
nref, npos, tlen, cigar, seq, qual, tags); a file is (header text, [(reference name, length)], [record]).  parse_sam makes
one from SAM text.  The deviations of include/parasuite_hip.h are restated too: errors where the Java throws (CombineError),
a lifted start below base 1 counts as not located, the unsorted form."""
import re

STAT_KEYS = ("n_genome", "n_transcript", "n_unplaced", "n_unlocated", "n_missed_indel_splice", "n_groups", "n_groups_ambiguous",
             "n_no_contig", "n_mt_unplaced", "n_lifted", "n_spliced", "n_strand_flipped")
SEQ16 = "=ACMGRSVTWYHKDBN"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


class CombineError(Exception):
    pass


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return (base + (beg >> shift)) & 0xffff
    return 0


def cigar_ops(cigar):
    return [] if cigar == "*" else [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def ref_length(cigar):
    return sum(n for n, op in cigar_ops(cigar) if op in "MDN=X")


def parse_sam(text):
    """SAM text -> (header text, refs, records); bases as BAM stores them (upper case, what is no IUPAC code becomes N)"""
    head, refs, recs, ids = [], [], [], {}
    for line in text.split("\n"):
        if line.startswith("@"):
            head.append(line + "\n")
            if line.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in line.split("\t")[1:])
                ids[f["SN"]] = len(refs)
                refs.append((f["SN"], int(f["LN"])))
        elif line:
            f = line.split("\t")
            ref = -1 if f[2] == "*" else ids[f[2]]
            seq = f[9] if f[9] == "*" else "".join(c if c in SEQ16 else "N" for c in f[9].upper())
            pos = int(f[3]) - 1
            recs.append(dict(name=f[0], flag=int(f[1]), ref=ref, pos=pos, mapq=int(f[4]), bin=reg2bin(pos, pos + (ref_length(f[5]) or 1)),
                             nref=ref if f[6] == "=" else -1 if f[6] == "*" else ids[f[6]], npos=int(f[7]) - 1, tlen=int(f[8]),
                             cigar=f[5], seq=seq, qual="" if seq == "*" else f[10], tags=f[11:]))   # no SEQ: BAM holds no QUAL byte
    return "".join(head), refs, recs


def sort_order(text):
    first = text.split("\n", 1)[0]
    if not first.startswith("@HD"):
        return ""
    for f in first.split("\t")[1:]:
        if f.startswith("SO:"):
            return f[3:]
    return ""


def java_split(s, sep):
    """String.split: trailing empty strings are dropped; an empty string is one empty string"""
    out = s.split(sep)
    if s == "":
        return out
    while out and out[-1] == "":
        out.pop()
    return out


def parse_int(s, contig):
    if not re.fullmatch(r"[+-]?[0-9]{1,10}", s) or not -2 ** 31 <= int(s) < 2 ** 31:
        raise CombineError("transcript name %s has an exon position that is not a number" % contig)
    return int(s)


def exon_table(contig):
    """(fields, sorted starts, sorted ends): the two lists are sorted AS STRINGS, each on its own (Arrays.sort on String[])"""
    f = java_split(contig, "|")
    if len(f) < 6:
        raise CombineError("transcript name %s has fewer than six '|' fields" % contig)
    starts, ends = sorted(java_split(f[3], ";")), sorted(java_split(f[4], ";"))
    if len(starts) != len(ends):
        raise CombineError("transcript name %s lists %d exon starts and %d exon ends" % (contig, len(starts), len(ends)))
    return f, [parse_int(x, contig) for x in starts], [parse_int(x, contig) for x in ends]


def _word(n, op):
    return (n & 0x0fffffff, op)           # a BAM CIGAR word holds 28 bits of length


def lift(rec, strand, es, ee):
    """:192-518 -> (start or -1, list of (length, op), missed)"""
    aln_start = rec["pos"] + 1
    aln_end = 0 if rec["flag"] & 4 else aln_start + ref_length(rec["cigar"]) - 1
    read_len = 0 if rec["seq"] == "*" else len(rec["seq"])
    has_id = "I" in rec["cigar"] or "D" in rec["cigar"]
    own = [_word(n, op) for n, op in cigar_ops(rec["cigar"])]
    start, cigar, passed, missed = -1, [], 0, False
    if strand == "1":
        for i in range(len(es)):
            before = passed
            passed += ee[i] - es[i] + 1
            if aln_start <= passed and start == -1:
                start = es[i] + (aln_start - before) - 1
            if aln_end <= passed:
                if start >= es[i]:
                    cigar = list(own)
                else:
                    cigar.append(_word(aln_end - before, "M"))
                break
            elif start != -1:
                if has_id:
                    missed = True
                    break
                cigar.append(_word(ee[i] - start + 1 if start >= es[i] else ee[i] - es[i] + 1, "M"))
                if i < len(es) - 1:
                    intron = es[i + 1] - ee[i] - 1
                    if intron <= 0:
                        break
                    cigar.append(_word(intron, "N"))
                else:
                    break
    elif strand == "-1":
        end = -1
        for i in range(len(es) - 1, -1, -1):
            before = passed
            passed += ee[i] - es[i] + 1
            if aln_start <= passed and end == -1:
                end = ee[i] - (aln_start - before) + 1
            if aln_end <= passed:
                if end <= ee[i]:
                    cigar = list(own)
                    start = end - read_len + 1
                else:
                    if has_id:
                        missed = True
                        break
                    cigar.insert(0, _word(aln_end - before, "M"))
                    start = ee[i] - (aln_end - before) + 1
                break
            elif end != -1:
                if has_id:
                    missed = True
                    break
                cigar.insert(0, _word(end - es[i] + 1 if end < ee[i] else ee[i] - es[i] + 1, "M"))
                if i >= 1:
                    intron = es[i] - ee[i - 1] - 1
                    if intron <= 0:
                        break
                    cigar.insert(0, _word(intron, "N"))
                else:
                    break
    return start, cigar, missed


def revcomp(seq):
    return seq if seq == "*" else "".join(_COMP.get(c, c) for c in reversed(seq))


def header_sorted(text):
    if text.startswith("@HD"):
        first, rest = text.split("\n", 1)
        return "\t".join(f for f in first.split("\t") if not f.startswith("SO:")) + "\tSO:coordinate\n" + rest
    return "@HD\tVN:1.6\tSO:coordinate\n" + text


def combine(genome, transcript, sort_by_coordinate=False):
    """-> (header text, refs, records, stats)"""
    g_text, g_refs, g_recs = genome
    t_text, t_refs, t_recs = transcript
    if sort_order(t_text) != "queryname":
        raise CombineError("the transcript file is not sorted by read name")
    st = dict.fromkeys(STAT_KEYS, 0)
    st["n_genome"], st["n_transcript"] = len(g_recs), len(t_recs)
    g_id = {}
    for i, (name, _) in enumerate(g_refs):
        g_id.setdefault(name, i)
    out, tables = [dict(r) for r in g_recs], {}

    def flush(group):                       # printReadsToBamFile: group = [(record, start, cigar)] of the located records
        if not group["hits"]:
            return
        if any(s != group["hits"][0][1] for _, s, _ in group["hits"]):
            st["n_groups_ambiguous"] += 1
            return
        rec, start, cigar = group["hits"][group["primary"]]
        f = list(tables[rec["ref"]][0])
        if "chr" + f[2] not in g_id:
            st["n_no_contig"] += 1
            return
        if f[2] == "MT":
            f[2] = "M"
        new = dict(rec)
        new["ref"] = g_id.get("chr" + f[2], -1)
        if new["ref"] == -1:
            st["n_mt_unplaced"] += 1
        new["pos"] = start - 1
        new["cigar"] = "".join("%d%s" % w for w in cigar) or "*"
        new["bin"] = reg2bin(new["pos"], new["pos"] + (sum(n for n, op in cigar if op in "MDN=X") or 1))
        new["mapq"] = 10
        if f[5] == "-1":
            new["flag"] ^= 16
            new["seq"] = revcomp(rec["seq"])
            st["n_strand_flipped"] += 1
        out.append(new)
        st["n_lifted"] += 1

    name, group = None, dict(hits=[], primary=0)
    for rec in t_recs:
        if rec["ref"] < 0:
            st["n_unplaced"] += 1
            continue
        if rec["name"] != name:
            flush(group)
            group, name = dict(hits=[], primary=0), rec["name"]
            st["n_groups"] += 1
        if rec["ref"] not in tables:
            tables[rec["ref"]] = exon_table(t_refs[rec["ref"]][0])
        f, es, ee = tables[rec["ref"]]
        start, cigar, missed = lift(rec, f[5], es, ee)
        st["n_missed_indel_splice"] += missed
        if start < 1:                       # the Java: == -1; below base 1 see include/parasuite_hip.h, deviation (2)
            st["n_unlocated"] += 1
            continue
        if any(op == "N" for _, op in cigar):
            st["n_spliced"] += 1
        if not rec["flag"] & 0x100:
            group["primary"] = len(group["hits"])
        group["hits"].append((rec, start, cigar))
    flush(group)
    if sort_by_coordinate:
        out.sort(key=lambda r: (r["ref"] & 0xffffffff, r["pos"]))
        g_text = header_sorted(g_text)
    return g_text, list(g_refs), out, st


FIELDS = ("name", "flag", "ref", "pos", "mapq", "bin", "nref", "npos", "tlen", "cigar", "seq", "qual", "tags")


def same_records(got, exp):
    """field by field, tags included; returns the first difference or None"""
    if len(got) != len(exp):
        return "record count %d != %d" % (len(got), len(exp))
    for i, (a, b) in enumerate(zip(got, exp)):
        for k in FIELDS:
            if a[k] != b[k]:
                return "record %d (%s) field %s: %r != %r" % (i, b["name"], k, a[k], b[k])
    return None
