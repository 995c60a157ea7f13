"""The call-by-call restatement of the `map` mode with --unaligned, --ref-refine and the search options (Main.java:249-420), for
tests/test_map_route_flags_cpu.py (the oracle as the mapper) and tests/test_gpu_map_route_flags.py (the library, against
ps_map_route_opts).  Data and mappers are tests/map_route.py's; the steps are route_by_steps' pieces in Main.java's order.

The two deviations from the Java, as include/parasuite_hip.h states them:
  (1) refine, no transcripts, --unaligned: the Java leaves the .bai it wrote before the second extraction rewrote the BAM; here
      the BAM is indexed again, so the .bai is the one of the file as it ends up;
  (2) transcripts, --unaligned: the Java's second extraction (:382-388) runs on the already filtered BAM and overwrites
      <P>.unaligned.fastq with nothing before the transcript pass reads it; here that extraction is not made, and the file of the
      first extraction (:299-302 or :371-374) is kept instead of removed (:405-407)."""
import os

import map_route as M


class LibSearchMapper(M.LibMapper):
    """the library's own calls with search options: ps_map_opts + ps_sam_to_bam where LibMapper says ps_map_to_bam"""

    def __init__(self, search, threads=4):
        super().__init__(threads)
        self.search = search

    def map(self, mm, ep, ip, ref, fq, out_bam, min_mapq):
        import capi
        sam = out_bam + ".sam"
        capi.ps_map(self.threads, mm, ep, ip, ref, fq, sam, search=self.search)
        st = capi.ps_sam_to_bam(sam, out_bam, min_mapq=min_mapq, threads=self.threads)
        os.remove(sam)
        return st


def write_other_width(fasta, out, width=37):
    """the same sequences under another file name with another line width: a --ref-refine that differs by realpath only"""
    with open(fasta) as f, open(out, "w") as o:
        name, seq = None, []

        def flush():
            if name is not None:
                s = "".join(seq)
                o.write(name + "\n" + "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)))

        for line in f:
            line = line.rstrip("\n")
            if line.startswith(">"):
                flush()
                name, seq = line, []
            else:
                seq.append(line)
        flush()
    return out


def without_contig(fasta, out, drop):
    """the FASTA without the contig named `drop`"""
    with open(fasta) as f, open(out, "w") as o:
        keep = True
        for line in f:
            if line.startswith(">"):
                keep = line[1:].split()[0] != drop
            if keep:
                o.write(line)
    return out


def route_by_steps_flags(mapper, data, prefix, refine=False, transcripts=False, error_profile=None, indel_profile=None,
                         keep_unaligned=False, ref_refine=None, gm=10, tm=1, bwa_mm="2", parasuite_mm="-1", max_read_len=101, threads=4):
    """Main.java:249-420 call by call with keepUnaligned and referenceRefineFileName; returns the stats of the single steps"""
    import capi
    ref, fq, tfa = data["genome_fa"], data["route_fastq"], data["transcripts_fa"]
    unaligned = prefix + ".unaligned.fastq"
    st = dict(n_reads=0, first=None, refine=None, transcript=None, extract=None, combine=None)

    def extract(bam):
        st["extract"] = capi.ps_extract_weak_reads(bam, bam + ".new", unaligned, gm, threads=threads)
        os.replace(bam + ".new", bam)

    def genomic(mm, ep, ip, reference, out, min_mapq, extract_now):
        m = mapper.map(mm, ep, ip, reference, fq, out, min_mapq)           # Mapping.executeMapping
        st["n_reads"] = m["n_in"]
        if extract_now:
            extract(out)
        s = capi.ps_bam_sort(out, out + ".sorted", threads=threads)       # Mapping.sortByCoordinateAndIndex
        os.replace(out + ".sorted", out)
        capi.ps_bam_index(out, threads=threads)
        return dict(n_in=m["n_in"], n_out=s["n_out"])

    ep, ip = error_profile, indel_profile
    last = None
    if not error_profile:                                                  # isFirstMapping, :283-310
        last = prefix + ".BWA-genomic.bam"
        weak_now = transcripts and not refine
        st["first"] = genomic(bwa_mm, None, None, ref, last, 0 if weak_now else gm, weak_now)
    if refine:                                                             # :312-381
        ref = ref_refine or ref                                            # :318
        if not error_profile:
            mapper.profile(last, ref, max_read_len)                        # :327-334: against the refine reference
            ep, ip = last + ".errorprofile", last + ".indelprofile"
        last = prefix + ".PARAsuite-genomic.bam"
        st["refine"] = genomic(parasuite_mm, ep, ip, ref, last, 0 if (transcripts or keep_unaligned) else gm, transcripts)     # :354-357
    if keep_unaligned and not transcripts:                                 # :382-390; with transcripts: deviation (2)
        extract(last)
        capi.ps_bam_index(last, threads=threads)                           # deviation (1)
        (st["refine"] if refine else st["first"])["n_out"] = st["extract"]["n_kept"]
    if transcripts:                                                        # :392-416
        t_bam = prefix + (".PARAsuite-transcript.bam" if refine else ".BWA-transcript.bam")
        m = mapper.map(parasuite_mm if refine else bwa_mm, ep if refine else None, ip if refine else None, tfa, unaligned, t_bam, tm)
        s = capi.ps_bam_sort(t_bam, t_bam + ".sorted", by_name=True, threads=threads)
        os.replace(t_bam + ".sorted", t_bam)
        if not keep_unaligned:
            os.remove(unaligned)                                           # :405-407
        st["transcript"] = dict(n_in=m["n_in"], n_out=s["n_out"])
        st["combine"] = mapper.combine(last, t_bam, prefix + ".combined.bam")
        last = prefix + ".combined.bam"
    if hasattr(mapper, "cleanup"):
        mapper.cleanup()
    st["mapping_file"] = last
    return st


def output_names(prefix, refine, transcripts, given, keep_unaligned):
    return sorted(M.output_names(prefix, refine, transcripts, given) + ([prefix + ".unaligned.fastq"] if keep_unaligned else []))


def fastq_names(path):
    with open(path) as f:
        lines = f.read().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [l[1:] for l in lines[0:-1:4]]
