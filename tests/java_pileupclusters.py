"""Plain-Python restatement of PileupClusters.calculateReadPileups (PileupClusters.java:62-583, calculateClusterInformation
:585-673, SNPCalling.querySNP :49-69, StrandOrientation :48-56) -- the toolkit's `clust` mode -- for all six files it
writes, with this library's documented deviations where the Java throws (include/parasuite_hip.h, ps_pileup_clusters):

  - a T->C at read index >= 51 counts everywhere except the read-position flags (the Java's boolean[51] throws);
  - a VCF record whose first ALT allele is symbolic (<...>, breakends, '*') never matches;
  - a record on a contig the FASTA lacks, a record or a cluster-sequence fetch past its contig's end, and a mapped record
    with SEQ '*' raise ValueError (the Java throws there as well).

Two inputs make the restatement raise FixtureError instead, because the library only counts them: a HashMap bucket that
would take a 9th key (the Java resizes or makes a tree there; rule 6 of the model does not follow) and a CCR window that
starts before base 1 (htsjdk reads bytes before the contig).

HashMap<Integer,Integer> iteration order (:189, :206) is modelled, not run: bucket (p ^ p >>> 16) & (cap - 1), then the
order in which the key was first put since the map was last cleared.  `cap` is the table size of the one mutationMap
object, which clear() never shrinks: 16, doubled whenever the size passes 0.75 * cap.

Small inputs only: one Python loop per record and base.  Double.toString is the oracle's port (orc.java_double).  Test
infrastructure, not product code."""
import gzip

import orc

OUT_FILES = ("", ".ccr.fasta", ".ccr.tsv", ".report")                 # next to OUT
SITE_FILES = (".sitefrequency.tsv", ".sitepositions.tsv")              # next to the mapping file (:74-81)
_CODE = {ord(c): i for i, c in enumerate("ACGT")}
_CODE.update({ord(c): i for i, c in enumerate("acgt")})
_COMP = {ord(a): ord(b) for a, b in zip("ACGTacgt", "TGCAtgca")}

HEADER = ("ClusterID\tChr\tStart\tEnd\tStrand\t#reads\t#T2C\t#T2C sites\tT2C Fraction\tSeqenece\tCombStrand\tSeqLength\n")
CCR_HEADER = ("Protein_Group\tCluster ID\tStrand\tChromosome\tCluster_Begin\tCluster_End\tAnchor_FlankSeq_Begin\t"
              "Anchor_FlankSeq_End\tAnchor_FlankSeq\tAnchor_Position\tCluster_Clone_Count\tNumber_of_T2C_Positions\t"
              "T2C_Freq_at_Anchor_Position\tT2C_Fract_at_Anchor_Position\tT2C_Freq_Whole_Cluster\tT2C_Fract_Whole_Cluster\n")


class FixtureError(Exception):
    """the input leaves the model (a bucket of more than 8 keys, a CCR window before base 1)"""


def jd(v):
    return orc.java_double(v)


def _pos(b):                                   # calculateArrayPos, :690-721
    return _CODE.get(b, -1)


def _revcomp(a):                               # htsjdk SequenceUtil.reverseComplement: other bytes keep their value
    return bytes(_COMP.get(b, b) for b in reversed(a))


def cigar_ops(s):
    ops, n = [], 0
    for ch in s:
        if ch.isdigit():
            n = n * 10 + int(ch)
        else:
            ops.append((ch, n))
            n = 0
    return ops


def bucket(p, cap):
    h = p & 0xFFFFFFFF
    return (h ^ (h >> 16)) & (cap - 1)


class JMap:
    """HashMap<Integer,Integer> as far as the Java's use of mutationMap shows: values, table size, iteration order"""

    def __init__(self):
        self.cap, self.v, self.first, self.seq = 16, {}, {}, 0

    def put_count(self, k):
        if k in self.v:
            self.v[k] += 1
            return
        b = bucket(k, self.cap)
        if sum(1 for q in self.v if bucket(q, self.cap) == b) >= 8:
            raise FixtureError("a HashMap bucket would take a 9th key (position %d)" % k)
        self.v[k] = 1
        self.first[k] = self.seq
        self.seq += 1
        if len(self.v) > 0.75 * self.cap:      # ++size > threshold: resize (:655-660 through HashMap.putVal)
            self.cap *= 2

    def keys(self):                            # iteration order
        return sorted(self.v, key=lambda k: (bucket(k, self.cap), self.first[k]))

    def clear(self):
        self.v, self.first, self.seq = {}, {}, 0


def read_fasta(path):
    """{first word of the header: sequence bytes as stored}"""
    seqs, name, parts = {}, None, []
    for line in open(path, "rb"):
        line = line.rstrip(b"\r\n")
        if line.startswith(b">"):
            if name is not None:
                seqs[name] = b"".join(parts)
            name, parts = line[1:].split()[0].decode(), []
        else:
            parts.append(line)
    if name is not None:
        seqs[name] = b"".join(parts)
    return seqs


def read_vcf(data):
    """bytes of a VCF (plain or gzip'ed) -> set of (CHROM, POS) whose REF contains T and whose first ALT allele contains C"""
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    out = set()
    for line in data.decode().split("\n"):
        if not line or line.startswith("#"):
            continue
        f = line.rstrip("\r").split("\t")
        alt0 = f[4].split(",")[0].upper()
        if alt0.startswith("<") or "[" in alt0 or "]" in alt0 or alt0 == "*":
            continue
        if "T" in f[3].upper() and "C" in alt0:
            out.add((f[0], int(f[1])))
    return out


class Rec:
    def __init__(self, line):
        f = line.split("\t")
        self.flag, self.rname, self.start = int(f[1]), f[2], int(f[3])
        self.cigar_s = f[5]
        self.cigar = cigar_ops(f[5]) if f[5] != "*" else []
        self.seq = f[9].encode()
        span = sum(n for op, n in self.cigar if op in "MDN=X")
        self.end = self.start + span - 1                       # htsjdk getAlignmentEnd
        self.rev = bool(self.flag & 16)

    def blocks(self):                                          # htsjdk getAlignmentBlocks: (read start 0-based, ref start, length)
        rp, gp = 0, self.start
        for op, n in self.cigar:
            if op in "M=X":
                yield rp, gp, n
                rp += n
                gp += n
            elif op in "IS":
                rp += n
            elif op in "DN":
                gp += n


def _fetch(ref, chrom, a, b):                  # getSubsequenceAt(chrom, a, b), 1-based inclusive
    s = ref[chrom]
    if b > len(s):
        raise ValueError("fetch past the end of %s: %d > %d" % (chrom, b, len(s)))
    return s[a - 1:b]


def cluster(sam_text, ref, vcf_bytes, min_cov):
    """(files, stats, info): files maps each suffix of OUT_FILES and SITE_FILES to bytes; stats is the library's stats dict;
    info holds what the fixtures are checked by (tie counts, max cap)"""
    lines = sam_text.split("\n")
    so = None
    for l in lines:
        if l.startswith("@HD"):
            for t in l.split("\t")[1:]:
                if t.startswith("SO:"):
                    so = t[3:]
    if so != "coordinate":                                                  # :85-92
        raise ValueError("not sorted by coordinate (SO:%s)" % so)
    snps = read_vcf(vcf_bytes) if vcf_bytes else set()
    out, fasta, tsv = [HEADER], [], [CCR_HEADER]
    st = dict(n_records=0, n_unmapped=0, n_skipped_indel=0, n_kept=0, n_clusters=0, n_clusters_written=0, n_crosslinked=0,
              n_ccr=0, n_double_stranded=0, n_snp_hits=0, n_snv_sites=0, n_t2c_beyond_51=0, n_ccr_clipped=0,
              n_ccr_past_end=0, n_order_unmodelled=0)
    info = dict(ties_hashmap=0, max_cap=16, best_sites=[])
    allele_freq, allele_pos, n_xl, n_allele_pos = [], [0] * 51, 0, 0
    t_start, t_end, t_chr, t_bytes = 0, 0, "", b""
    n_reads = n_t2c = n_sites = 0
    mut, cov = JMap(), {}
    is_rev, t_rev = False, False                                             # StrandOrientation: True / False / None
    cluster_id, running_id = "", 1
    flags = [False] * 51

    def info_read(r):                                                        # calculateClusterInformation, :585-673
        nonlocal n_t2c, is_rev
        if not r.seq or r.seq == b"*":
            raise ValueError("mapped record without SEQ")
        rs, gs = b"", b""
        for rp, gp, n in r.blocks():
            if rp + n > len(r.seq):
                raise ValueError("CIGAR longer than SEQ")
            rs += r.seq[rp:rp + n]
            gs += _fetch(ref, r.rname, gp, gp + n - 1)
        if r.rev:
            rs, gs = _revcomp(rs), _revcomp(gs)
            is_rev = True                                                    # :610-612 (the object is never null)
        for i in range(len(rs)):
            p = r.end - i if r.rev else r.start + i
            if _pos(gs[i]) == 3 and _pos(rs[i]) == 1:
                n_t2c += 1
                if i < 51:
                    flags[i] = True
                else:
                    st["n_t2c_beyond_51"] += 1                               # deviation: boolean[51] throws
                mut.put_count(p)
            cov[p] = cov.get(p, 0) + 1

    def close():                                                             # :178-344
        nonlocal n_xl, n_allele_pos, n_sites
        frac_sum = 0.0
        if n_reads < min_cov:
            return
        n_sites = len(mut.v)
        info["max_cap"] = max(info["max_cap"], mut.cap)
        best_pos, best_val = -1, 0.0
        strip = t_chr[3:] if t_chr.startswith("chr") else t_chr              # SNPCalling.java:51-54
        keep = {}
        for k in mut.keys():                                                 # :189-199
            if (strip, k) in snps:
                st["n_snp_hits"] += 1
            else:
                keep[k] = mut.v[k]
            if mut.v[k] == 1:
                st["n_snv_sites"] += 1
        if n_sites > 0:
            order = [k for k in mut.keys() if k in keep]                     # clear + putAll keeps the model's order
            vals = []
            for k in order:                                                  # :206-222
                v = keep[k] / cov[k]
                if v >= best_val:
                    best_val, best_pos = v, k
                vals.append(v)
            if vals:
                m = max(vals)
                tied = [k for k, v in zip(order, vals) if v == m]
                if len(tied) > 1 and (best_pos != max(tied) or best_pos != max(tied, key=lambda k: mut.first[k])):
                    info["ties_hashmap"] += 1
            srt = sorted(vals, reverse=True)                                 # :223-224
            s = 0.0
            for v in srt:
                s += v
            if srt and s >= 0.2:                                             # :229-256
                for k in range(len(srt)):
                    if len(allele_freq) > k:
                        allele_freq[k] = allele_freq[k] + srt[k]
                    elif not allele_freq:
                        allele_freq.extend(srt)
                    else:
                        allele_freq.append(srt[k])
                n_xl += 1
                for j in range(51):
                    if flags[j]:
                        allele_pos[j] += 1
                        n_allele_pos += 1
            for v in srt:                                                    # :258-260
                frac_sum += v
            if best_pos > 0:                                                 # :262-315
                comb = strand_str(is_rev)
                if best_pos - 20 < 1:
                    raise FixtureError("CCR window before base 1 (best site %d)" % best_pos)
                if best_pos + 20 > len(ref[t_chr]):
                    ccr = b""                                                # SAMException caught at :276
                    st["n_ccr_past_end"] += 1
                else:
                    ccr = ref[t_chr][best_pos - 21:best_pos + 20]
                    if comb == "-":
                        ccr = _revcomp(ccr)
                ccr = ccr.decode().upper()
                fasta.append(">%s 20-anchor-20 %s:%s:%d-%d\n%s\n" % (cluster_id, t_chr, comb, best_pos - 20, best_pos + 20, ccr))
                tsv.append("Gene\t%s\t%s\t%s\t%d\t%d\t%d\t%d\t%s\t%d\t%d\t%d\t%d\t%s\t%d\t%s\n" % (
                    cluster_id, comb, t_chr, t_start, t_end, best_pos - 20, best_pos + 20, ccr, best_pos, n_reads, n_sites,
                    mut.v[best_pos], jd(best_val), n_t2c, jd(frac_sum)))
                st["n_ccr"] += 1
                info["best_sites"].append(best_pos)
        seq = _revcomp(t_bytes) if t_rev else t_bytes                        # :317-343
        out.append("%s\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%s\t%s\t%s\t%d\n" % (
            cluster_id, t_chr, t_start, t_end, "-" if t_rev else "+", n_reads, n_t2c, n_sites, jd(frac_sum), seq.decode(),
            strand_str(is_rev), len(seq)))
        st["n_clusters_written"] += 1

    for l in lines:
        if not l or l.startswith("@"):
            continue
        st["n_records"] += 1
        r = Rec(l)
        if r.flag & 4:                                                       # :146
            st["n_unmapped"] += 1
            continue
        if ("I" in r.cigar_s or "D" in r.cigar_s) and "N" in r.cigar_s:     # :152-157
            st["n_skipped_indel"] += 1
            continue
        if r.rname not in ref:
            raise ValueError("record on a contig the reference lacks: " + r.rname)
        if r.end > len(ref[r.rname]):
            raise ValueError("record past the end of " + r.rname)
        st["n_kept"] += 1
        if t_end - r.start < 5 or r.rname != t_chr:                          # :175-176
            close()
            t_start, t_end, t_chr = r.start, r.end, r.rname                  # :346-357
            n_reads, n_t2c, n_sites = 1, 0, 0
            is_rev = False
            mut.clear()
            cov = {}
            running_id += 1
            cluster_id = "cl_%d_%s" % (running_id, t_chr)
            flags = [False] * 51
            st["n_clusters"] += 1
            info_read(r)
            t_rev = is_rev
            t_bytes = b""                                                    # :367-414
            cbs = r.start
            for op, n in r.cigar:
                if op in "DM":
                    t_bytes += _fetch(ref, r.rname, cbs, cbs + n - 1)
                if op != "I":
                    cbs += n
        else:
            t_chr = r.rname                                                  # :416-499
            if r.end > t_end:
                cbs = r.start
                for op, n in r.cigar:
                    if cbs + n - 1 < t_end:
                        if op != "I":
                            cbs += n
                        continue
                    if op in "DM":
                        add = _fetch(ref, r.rname, cbs, cbs + n - 1)
                        ov = t_end - cbs + 1
                        t_bytes = t_bytes + add[ov:n] if ov > 0 else add + t_bytes
                    t_end = r.end
                    if op != "I":
                        cbs += n
            n_reads += 1
            info_read(r)
            if is_rev is not None and t_rev != is_rev:
                st["n_double_stranded"] += 1
                is_rev = None
    files = {"": "".join(out).encode(), ".ccr.fasta": "".join(fasta).encode(), ".ccr.tsv": "".join(tsv).encode()}
    files[".report"] = ("Double stranded clusters found: %d\nLoci found that are SNPs: 0\n%d insertion or deletion skipped\n"
                        "T-C mutations identified as SNPs: %d\nT-C mutations identified as SNVs (100%% T-C in 1 site): %d\n" % (
                            st["n_double_stranded"], st["n_skipped_indel"], st["n_snp_hits"], st["n_snv_sites"])).encode()
    files[".sitefrequency.tsv"] = "".join(jd(v / n_xl) + "\n" for v in allele_freq).encode()        # :531-538
    files[".sitepositions.tsv"] = "".join(jd(a / n_allele_pos if n_allele_pos else float("nan")) + "\n"
                                          for a in allele_pos).encode()                        # :539-545
    st["n_crosslinked"] = n_xl
    return files, st, info


def strand_str(v):                              # StrandOrientation.getStrandOrientation, :48-56
    return "+/-" if v is None else ("-" if v else "+")
