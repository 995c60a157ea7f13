"""The `map -t` route (Main.java:363-416) on the generated data of tests/combine_route.py WITHOUT a GPU: the oracle's
map_fastq in place of the GPU mapper, the host steps of the library (ps_sam_to_bam, ps_extract_weak_reads, ps_bam_sort) and
the restatement tests/java_combine.py in place of ps_combine_genome_transcript.  Holds the restatement to the truth the
generator knows (check (b) of tests/test_gpu_combine.py, which is independent of the restatement's own reading of the Java)
and confirms that the generator's parameters meet that check's conditions."""
import os

import combine_route as R
import java_combine as J


def test_route_with_the_oracle_mapper(tmp_path):
    import capi
    import orc
    from test_bam import read_bam
    d = str(tmp_path)
    data = R.make_data(d)
    p = lambda x: os.path.join(d, x)
    opt = orc.stock_opt("2")
    orc.Index.from_fasta(data["genome_fa"]).map_fastq(opt, data["fastq"], p("g.sam"), n_threads=8)
    capi.ps_sam_to_bam(p("g.sam"), p("g.bam"), min_mapq=0, threads=4)
    st = capi.ps_extract_weak_reads(p("g.bam"), p("g.kept.bam"), p("weak.fq"), 10, threads=4)
    assert st["n_records"] == data["n_reads"] and st["n_weak"] + st["n_kept"] == data["n_reads"] and st["n_weak"] > 1000
    orc.Index.from_fasta(data["transcripts_fa"]).map_fastq(opt, p("weak.fq"), p("t.sam"), n_threads=8)
    capi.ps_sam_to_bam(p("t.sam"), p("t.bam"), min_mapq=1, threads=4)
    capi.ps_bam_sort(p("t.bam"), p("t.byname.bam"), by_name=True, threads=4)
    genome, transcript = read_bam(p("g.kept.bam"))[:3], read_bam(p("t.byname.bam"))[:3]
    assert J.sort_order(transcript[0]) == "queryname" and len(transcript[1]) == data["n_transcripts"]
    text, refs, recs, st = J.combine(genome, transcript, sort_by_coordinate=True)
    assert st["n_genome"] == len(genome[2]) and st["n_lifted"] == len(recs) - len(genome[2]) > 0
    c = R.check_lifted(data, (text, refs, recs), transcript[2])
    print(st, c)
    assert c["n_lifted"] == st["n_lifted"]
    R.assert_conditions(c)
    R.assert_at_most_once(data, recs)
    key = [(r["ref"] & 0xffffffff, r["pos"]) for r in recs]
    assert key == sorted(key)
