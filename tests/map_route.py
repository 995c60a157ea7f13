"""Data and the call-by-call restatement for the whole `map` mode (Main.java:249-420), shared by tests/test_map_route_cpu.py (the
oracle as the mapper) and tests/test_gpu_map_route.py (the library, against ps_map_route).

Data: the genome, transcripts and 6000 transcript reads of tests/combine_route.py, and in the same FASTQ 6000 reads `gen<i>` of
36-50 bases cut anywhere from the three contigs, either orientation, 60 % of them with one to three T turned to C in read
orientation (the PAR-CLIP signal the refine pass learns), then 1 % substitutions per base, constant quality; and a dozen trap
reads: names ending /1, /2, /1/2, lower-case bases, an IUPAC base, a read of N only.

Steps: route_by_steps() issues the calls a caller had to string together before ps_map_route existed, in Main.java's order,
with the library or the oracle as the mapper, and leaves the files Main.java names."""
import os
import shutil

import numpy as np

import combine_route as R

SEED = 0x6D6170
N_GEN = 6000
CASES = {                      # name -> (refine, transcripts, profile given)
    "stock": (False, False, False),
    "stock_transcripts": (False, True, False),
    "refine": (True, False, False),
    "refine_transcripts": (True, True, False),
    "refine_given_transcripts": (True, True, True),
}


def make_data(workdir, seed=SEED):
    data = R.make_data(workdir)
    rng = np.random.default_rng(seed)
    contigs = sorted(data["genome"])
    fq = os.path.join(workdir, "map_route_reads.fq")
    shutil.copyfile(data["fastq"], fq)
    names = []

    def genome_read(n):
        chrom = contigs[int(rng.integers(0, len(contigs)))]
        g = data["genome"][chrom]
        o = int(rng.integers(0, len(g) - n + 1))
        read = g[o:o + n]
        return R.revcomp(read) if rng.random() < 0.5 else read

    def junction_read(k):
        """40 bases across the first junction of transcript k, as the transcript FASTA holds them"""
        with open(data["transcripts_fa"], "rb") as f:
            recs = f.read().split(b">")[1:]
        head, _, body = recs[k].partition(b"\n")
        seq = body.replace(b"\n", b"")
        first_exon = int(head.split(b"|")[4].split(b";")[0]) - int(head.split(b"|")[3].split(b";")[0]) + 1
        if head.split(b"|")[5] == b"-1":                    # the FASTA holds the reverse complement: the first junction is at the far end
            at = len(seq) - first_exon
        else:
            at = first_exon
        return seq[at - 20:at + 20]

    with open(fq, "ab") as f:
        for i in range(N_GEN):
            n = int(rng.integers(36, 51))
            read = bytearray(genome_read(n))
            if rng.random() < 0.6:
                ts = [p for p in range(n) if read[p] == ord("T")]
                for p in rng.permutation(ts)[:int(rng.integers(1, 4))]:
                    read[int(p)] = ord("C")
            for p in np.nonzero(rng.random(n) < 0.01)[0]:
                read[int(p)] = b"ACGT"[(b"ACGT".index(read[int(p)]) + int(rng.integers(1, 4))) % 4]
            name = "gen%d" % i
            names.append(name)
            f.write(b"@" + name.encode() + b"\n" + bytes(read) + b"\n+\n" + b"I" * n + b"\n")
        iupac = bytearray(genome_read(44)); iupac[20] = ord("R")
        iupac_j = bytearray(junction_read(9)); iupac_j[5] = ord("Y")
        traps = [("trapA/1", genome_read(44)), ("trapB/2", genome_read(45)), ("trapC/1/2", genome_read(46)),
                 ("trapD/1", junction_read(3)), ("trapE/1/2", junction_read(4)), ("trapF/2/1", junction_read(5)),
                 ("trapG", genome_read(44).lower()), ("trapH", junction_read(6).lower()), ("trapI", bytes(iupac)),
                 ("trapJ", bytes(iupac_j)), ("trapN", b"N" * 40), ("trapK/3", junction_read(7))]
        for name, read in traps:
            f.write(b"@" + name.encode() + b" a comment\n" + read + b"\n+\n" + b"F" * len(read) + b"\n")
    data = dict(data)
    data["route_fastq"] = fq
    data["n_route_reads"] = data["n_reads"] + N_GEN + len(traps)
    data["gen_names"] = names
    data["trap_names"] = [t[0] for t in traps]
    return data


def strip_once(name):
    """what one parse of a FASTQ header leaves of a name: one trailing /1 or /2 removed (ps_reads.cpp)"""
    return name[:-2] if len(name) > 2 and name[-2:] in ("/1", "/2") else name


def all_names(data):
    """every name a record of the route may carry: once stripped in the genomic files, twice in the transcript file and the lifted records"""
    once = {strip_once(n) for n in list(data["truth"]) + data["gen_names"] + data["trap_names"]}
    return once | {strip_once(n) for n in once}


class LibMapper:
    """the library's own calls"""

    def __init__(self, threads=4):
        self.threads = threads

    def map(self, mm, ep, ip, ref, fq, out_bam, min_mapq):
        import capi
        return capi.ps_map_to_bam(self.threads, mm, ep, ip, ref, fq, out_bam, min_mapq=min_mapq)

    def profile(self, bam, ref, max_len):
        import capi
        capi.ps_error_profile(bam, ref, max_len, None)

    def combine(self, genome_bam, transcript_bam, out_bam):
        import capi
        return capi.ps_combine_genome_transcript(genome_bam, transcript_bam, out_bam, True, True, threads=self.threads)


class OrcMapper:
    """the oracle in the mapper's place: SAM text, then the library's host steps; the restatement tests/java_combine.py in the
    lift's place, whose result stays in memory (self.combined) instead of a file (no GPU)"""

    def __init__(self, threads=8):
        self.threads, self.idx, self.sam, self.combined = threads, {}, {}, None

    def map(self, mm, ep, ip, ref, fq, out_bam, min_mapq):
        import capi
        import orc
        if ref not in self.idx:
            self.idx[ref] = orc.Index.from_fasta(ref)
        if ep:
            P = [float(x) for x in open(ep).read().split()]
            ins, dele = [float(x) for x in open(ip).read().split()]
            opt = orc.profile_opt(P, ins, dele, int(mm))
        else:
            opt = orc.stock_opt(mm)
        sam = out_bam + ".orc.sam"
        self.idx[ref].map_fastq(opt, fq, sam, n_threads=self.threads)
        st = capi.ps_sam_to_bam(sam, out_bam, min_mapq=min_mapq, threads=4)
        with open(sam) as fi, open(sam + ".f", "w") as fo:        # what `samtools view -q` keeps, for the profile step
            for line in fi:
                if line.startswith("@") or int(line.split("\t", 5)[4]) >= min_mapq:
                    fo.write(line)
        os.remove(sam)
        self.sam[out_bam] = sam + ".f"
        return st

    def profile(self, bam, ref, max_len):
        import orc
        orc.error_profile(self.sam[bam], ref, max_len, bam)

    def combine(self, genome_bam, transcript_bam, out_bam):
        import java_combine as J
        from test_bam import read_bam
        text, refs, recs, st = J.combine(read_bam(genome_bam)[:3], read_bam(transcript_bam)[:3], sort_by_coordinate=True)
        self.combined = (text, refs, recs)
        return st

    def cleanup(self):
        for p in self.sam.values():
            if os.path.exists(p):
                os.remove(p)


def route_by_steps(mapper, data, prefix, refine=False, transcripts=False, error_profile=None, indel_profile=None, gm=10, tm=1,
                   bwa_mm="2", parasuite_mm="-1", max_read_len=101, threads=4):
    """Main.java:249-420 call by call; returns the stats of the single steps in ps_route_stats' shape"""
    import capi
    ref, fq, tfa = data["genome_fa"], data["route_fastq"], data["transcripts_fa"]
    weak_fq = prefix + ".unaligned.fastq"
    st = dict(n_reads=0, first=None, refine=None, transcript=None, extract=None, combine=None, unfiltered={})

    def genomic(mm, ep, ip, out, extract):
        m = mapper.map(mm, ep, ip, ref, fq, out, 0 if extract else gm)
        st["n_reads"] = m["n_in"]
        if extract:
            st["extract"] = capi.ps_extract_weak_reads(out, out + ".new", weak_fq, gm, threads=threads)
            os.replace(out + ".new", out)                                  # Main.java:305-306, 376-377
        s = capi.ps_bam_sort(out, out + ".sorted", threads=threads)         # Mapping.sortByCoordinateAndIndex
        os.replace(out + ".sorted", out)
        capi.ps_bam_index(out, threads=threads)
        return dict(n_in=m["n_in"], n_out=s["n_out"])

    ep, ip = error_profile, indel_profile
    last = None
    if not error_profile:
        last = prefix + ".BWA-genomic.bam"
        st["first"] = genomic(bwa_mm, None, None, last, transcripts and not refine)
        if refine:
            mapper.profile(last, ref, max_read_len)
            ep, ip = last + ".errorprofile", last + ".indelprofile"
    if refine:
        last = prefix + ".PARAsuite-genomic.bam"
        st["refine"] = genomic(parasuite_mm, ep, ip, last, transcripts)
    if transcripts:
        t_bam = prefix + (".PARAsuite-transcript.bam" if refine else ".BWA-transcript.bam")
        m = mapper.map(parasuite_mm if refine else bwa_mm, ep if refine else None, ip if refine else None, tfa, weak_fq, t_bam, tm)
        s = capi.ps_bam_sort(t_bam, t_bam + ".sorted", by_name=True, threads=threads)   # Mapping.sortByNameAndIndex
        os.replace(t_bam + ".sorted", t_bam)
        os.remove(weak_fq)
        st["transcript"] = dict(n_in=m["n_in"], n_out=s["n_out"])
        st["combine"] = mapper.combine(last, t_bam, prefix + ".combined.bam")
        last = prefix + ".combined.bam"
    if hasattr(mapper, "cleanup"):
        mapper.cleanup()
    st["mapping_file"] = last
    return st


def output_names(prefix, refine, transcripts, given):
    """the files of the issue's table"""
    out = []
    if not given:
        out += [prefix + ".BWA-genomic.bam", prefix + ".BWA-genomic.bam.bai"]
        if refine:
            out += [prefix + ".BWA-genomic.bam.errorprofile", prefix + ".BWA-genomic.bam.indelprofile"]
    if refine:
        out += [prefix + ".PARAsuite-genomic.bam", prefix + ".PARAsuite-genomic.bam.bai"]
    if transcripts:
        out += [prefix + (".PARAsuite-transcript.bam" if refine else ".BWA-transcript.bam"), prefix + ".combined.bam", prefix + ".combined.bam.bai"]
    return sorted(out)


def _key(r):
    return (r["flag"], r["ref"], r["pos"], r["cigar"], r["mapq"])


def route_counts(data, prefix, refine, n_weak, combined=None):
    """the figures the conditions are stated on, from the files a route left (transcripts given); combined: the combined
    mapping where no file holds it.  n_differ and n_rescued are counted on what the files hold, the records with MAPQ >= gm:
    n_differ = reads whose record (flag, reference, position, CIGAR, MAPQ) in <P>.BWA-genomic.bam is not their record in
    <P>.PARAsuite-genomic.bam, a read that only one of the two files holds included; n_rescued = reads only the second holds.
    A difference between two records that both stay below gm is not seen, so n_differ is a lower bound of the count over
    all records."""
    from test_bam import read_bam
    mode = "PARAsuite" if refine else "BWA"
    last = read_bam(prefix + ".%s-genomic.bam" % mode)
    transcript = read_bam(prefix + ".%s-transcript.bam" % mode)
    combined = combined or read_bam(prefix + ".combined.bam")
    c = dict(n_weak=n_weak)
    t_reads = [r for r in transcript[2] if r["name"].startswith("read")]
    lifted = R.check_lifted(data, combined[:3], t_reads)
    c.update(lifted)
    t_names = {r["name"] for r in transcript[2]}
    g_names = {r["name"] for r in last[2]}
    c["n_lifted_all"] = sum(1 for r in combined[2] if r["name"] in t_names and r["name"] not in g_names)
    R.assert_at_most_once(dict(truth=dict.fromkeys(all_names(data))), combined[2])
    key = [(r["ref"] & 0xffffffff, r["pos"]) for r in combined[2]]
    assert key == sorted(key)
    if refine:
        first = {r["name"]: _key(r) for r in read_bam(prefix + ".BWA-genomic.bam")[2]}
        kept = {r["name"]: _key(r) for r in last[2]}
        c["n_first_profiled"] = len(first)
        c["n_differ"] = sum(1 for n in set(first) | set(kept) if first.get(n) != kept.get(n))
        c["n_rescued"] = sum(1 for n in kept if n not in first)
        P = [float(x) for x in open(prefix + ".BWA-genomic.bam.errorprofile").read().split()]
        c["p_t_to_c"] = P[3 * 4 + 1]
    else:
        c["n_first_profiled"] = len(last[2])
    return c


def assert_route_conditions(c, refine):
    """conditions, not measurements: a run with less fails"""
    assert c["n_first_profiled"] >= 3000, c
    assert c["n_weak"] >= 1000, c
    R.assert_conditions(c)
    if refine:
        assert c["p_t_to_c"] >= 0.02, c
        assert c["n_differ"] >= 500, c
        assert c["n_rescued"] >= 300, c
