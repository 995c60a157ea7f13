"""bin/parasuite on the GPU: the toolkit's walk-through -- simulate, map --refine -t, benchmark, error, comb, clust, fetch,
extractAligned, extract -- one fresh child per step, each step's files against what the corresponding capi call writes into a
second directory from the same inputs.  A child that ends by a signal or at its time limit fails the test, and nothing more is
started."""
import gzip
import os
import shutil
import subprocess

import pytest

import map_route as M
from test_capi_cpu import ROOT
from test_simulator_cpu import GOLDEN, PROFILE_FILES

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "para-suite_amd", "bin", "parasuite")


def run(limit, *argv):
    """one fresh child under its own time limit -> (exit status, stderr)"""
    try:
        r = subprocess.run([CLI] + [str(a) for a in argv], timeout=limit, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail("parasuite %s did not end within %d s: nothing more is started" % (argv[0], limit), pytrace=False)
    if r.returncode < 0:
        pytest.fail("parasuite %s ended by signal %d: nothing more is started\n%s" % (argv[0], -r.returncode, r.stderr[-2000:]), pytrace=False)
    assert r.stdout == "", r.stdout                       # messages go to stderr
    return r.returncode, r.stderr


def ok(limit, *argv):
    rc, err = run(limit, *argv)
    assert rc == 0, (argv, err[-2000:])
    return err


def same(a, b, names):
    """the named files of two directories: BAM record for record (header included), everything else byte for byte"""
    for n in names:
        x, y = open(os.path.join(a, n), "rb").read(), open(os.path.join(b, n), "rb").read()
        if n.endswith(".bam"):
            x, y = gzip.decompress(x), gzip.decompress(y)
        assert x == y, n


def test_walk_through(workdir):
    import capi
    d = os.path.join(workdir, "cli")
    a, b = os.path.join(d, "cli"), os.path.join(d, "capi")             # what the command writes; what the library calls write
    os.makedirs(a); os.makedirs(b)
    data = M.make_data(d)
    genome, transcripts = data["genome_fa"], data["transcripts_fa"]
    capi.ps_index(genome)
    capi.ps_index(transcripts)
    prof = [os.path.join(GOLDEN, f) for f in PROFILE_FILES]            # error profile, site frequency, site positions, qualities, indels
    A, B = (lambda n: os.path.join(a, n)), (lambda n: os.path.join(b, n))

    # simulate T OUT EP T2C T2CPOS QUAL INDEL BOUND --seed 7
    ok(120, "simulate", transcripts, A("sim"), prof[0], prof[1], prof[2], prof[3], prof[4], "0.6", "--seed", "7")
    st = capi.ps_simulate_reads(transcripts, B("sim"), prof[0], prof[1], prof[2], prof[3], prof[4], 0.6, seed=7)
    sim = ["sim" + s for s in (".fastq", ".clusters", "_snps.vsf", ".log", ".err")]
    same(a, b, sim)
    assert st["n_reads"] >= 300
    err = ok(120, "simulate", transcripts, A("clock"), prof[0], prof[1], prof[2], prof[3], prof[4], "0.6")      # the seed comes from the clock and is said
    seed = [l for l in err.splitlines() if l.startswith("parasuite simulate: --seed ")]
    assert len(seed) == 1 and int(seed[0].split()[-1]) > 0
    for s in (".fastq", ".clusters", "_snps.vsf", ".log", ".err"):
        os.remove(A("clock" + s))

    # map -q -r -t -o --refine
    ok(300, "map", "-q", A("sim.fastq"), "-r", genome, "-t", transcripts, "-o", A("m"), "--refine", "-p", "4", "-l", "60")
    capi.ps_map_route_opts(B("sim.fastq"), genome, B("m"), transcripts_fa=transcripts, threads=4, refine=True, max_read_len=60)
    mapped = [os.path.basename(f) for f in M.output_names("m", True, True, False)]
    assert sorted(os.listdir(a)) == sorted(sim + mapped)
    same(a, b, [f for f in mapped if not f.endswith(".bai")])

    # benchmark MAPPING OUT READS [--only-bound]
    ok(120, "benchmark", A("m.combined.bam"), A("bench.stats"), A("sim.fastq"), "--only-bound")
    bst = capi.ps_benchmark_reads(B("m.combined.bam"), B("bench.stats"), B("sim.fastq"))
    same(a, b, ["bench.stats"])
    assert bst["n_tp"] + bst["n_tn"] > 0

    # error MAPPING REF MAXLEN -q true: six files beside the mapping
    ok(120, "error", A("m.BWA-genomic.bam"), genome, "51", "-q", "true")
    shutil.copyfile(B("m.BWA-genomic.bam"), B("e.bam")); shutil.copyfile(A("m.BWA-genomic.bam"), A("e.bam"))
    capi.ps_error_profile_full(B("e.bam"), genome, 51, None, True)
    six = (".errorprofile", ".indelprofile", ".errorprofile.vcf", ".qualityPerMismatch", ".indels", ".qualities")
    for s in six:
        assert open(A("m.BWA-genomic.bam" + s), "rb").read() == open(B("e.bam" + s), "rb").read(), s
    assert os.path.getsize(A("m.BWA-genomic.bam.qualities")) > 0
    os.remove(A("e.bam"))

    # comb -g G -t T -o O: sorted, with its index
    ok(120, "comb", "-g", A("m.PARAsuite-genomic.bam"), "-t", A("m.PARAsuite-transcript.bam"), "-o", A("comb.bam"))
    capi.ps_combine_genome_transcript(B("m.PARAsuite-genomic.bam"), B("m.PARAsuite-transcript.bam"), B("comb.bam"), True, True, threads=4)
    same(a, b, ["comb.bam"])
    assert gzip.decompress(open(A("comb.bam"), "rb").read()) == gzip.decompress(open(A("m.combined.bam"), "rb").read())
    assert os.path.exists(A("comb.bam.bai"))

    # clust MAPPING REF OUT SNP_VCF MINCOV
    ok(120, "clust", A("comb.bam"), genome, A("clusters.tsv"), "", "2")
    cst = capi.ps_pileup_clusters(B("comb.bam"), genome, B("clusters.tsv"), None, 2)
    same(a, b, ["clusters.tsv", "clusters.tsv.ccr.fasta", "clusters.tsv.ccr.tsv", "clusters.tsv.report", "comb.bam.sitefrequency.tsv", "comb.bam.sitepositions.tsv"])
    assert cst["n_clusters_written"] >= 10

    # fetch -i SITES -r REF -o OUT on the cluster table
    ok(120, "fetch", "-i", A("clusters.tsv"), "-r", genome, "-o", A("fetched.tsv"))
    fst = capi.ps_fetch_sequences(genome, B("clusters.tsv"), B("fetched.tsv"), bed=False)
    same(a, b, ["fetched.tsv"])
    assert fst["n_bases"] > 0

    # extractAligned -a BAM -o OUT
    ok(60, "extractAligned", "-a", A("comb.bam"), "-o", A("names.txt"))
    nst = capi.ps_extract_read_names(B("comb.bam"), B("names.txt"))
    same(a, b, ["names.txt"])
    assert nst["n_records"] > 0 and open(A("names.txt")).readline().startswith("@SEQ_ID:")

    # extract -i BAM -o FASTQ -t THR on a copy of a BAM: the copy is replaced by the records it keeps
    shutil.copyfile(A("comb.bam"), A("x.bam")); shutil.copyfile(B("comb.bam"), B("x.bam"))
    ok(60, "extract", "-i", A("x.bam"), "-o", A("x.fq"), "-t", "30")
    xst = capi.ps_extract_weak_reads(B("x.bam"), B("x.kept.bam"), B("x.fq"), 30)
    os.replace(B("x.kept.bam"), B("x.bam"))
    same(a, b, ["x.bam", "x.fq"])
    assert xst["n_weak"] > 0 and xst["n_kept"] > 0 and not os.path.exists(A("x.bam.extract-tmp"))

    # one error per kind: the library's message on stderr, exit 1, nothing written
    before = sorted(os.listdir(a))
    for argv, what in ((("benchmark", A("none.bam"), A("no.stats"), A("sim.fastq")), "cannot open"),
                       (("map", "-q", A("none.fq"), "-r", genome, "-o", A("no")), "ps_map_route_opts: first pass:"),
                       (("map", "-q", A("sim.fastq"), "-r", genome, "-o", A("no"), "--parasuite-ep", A("m.BWA-genomic.bam.errorprofile")), "nothing to map"),
                       (("fetch", "-i", A("none.tsv"), "-r", genome, "-o", A("no.tsv")), "none.tsv"),
                       (("extractAligned", "-a", A("none.bam"), "-o", A("no.txt")), "cannot open"),
                       (("comb", "-g", A("none.bam"), "-t", A("m.PARAsuite-transcript.bam"), "-o", A("no.bam")), "none.bam")):
        rc, err = run(120, *argv)
        assert rc == 1 and what in err and ("parasuite %s: " % argv[0]) in err, (argv, err[-1000:])
    rc, err = run(60, "map", "--mode", "BT2", "-q", A("sim.fastq"), "-r", genome, "-o", A("no"))
    assert rc == 1 and "stays with the Java toolkit" in err and "[parasuite-hip]" not in err
    assert sorted(os.listdir(a)) == before
