"""ps_fetch_sequences on the GPU: the hand-worked cases of tests/test_fetch_cpu.py, byte for byte and counter for counter
what the restatement tests/java_fetch.py gives from the FASTA text; every site of a 37-base contig against every phase of the
packed strand and of the 16-byte store; sites around the store's and the workgroup's sizes on a longer contig; the stream cut
into pieces of awkward sizes; random genomes and sites; the cluster table ps_pileup_clusters writes; a gzip-named reference."""
import gzip
import os
import random

import pytest

import java_fetch as J
from test_fetch_cpu import CASES, ERRORS, GENOME, HEADER, row

pytestmark = pytest.mark.gpu


def _indexed(d, text, name="g.fa"):
    import capi
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, name)
    with open(fa, "wb") as f:
        f.write(text)
    capi.ps_index(fa)
    return fa


def _run(d, fa, sites, bed, tag="run"):
    """the library on a sites file -> (bytes of the output file, stats)"""
    import capi
    src, out = os.path.join(d, tag + ".sites"), os.path.join(d, tag + ".out")
    with open(src, "wb") as f:
        f.write(sites)
    if os.path.exists(out):
        os.remove(out)
    st = capi.ps_fetch_sequences(fa, src, out, bed)
    assert not os.path.exists(out + ".fetch-tmp")
    return open(out, "rb").read(), st


def _same_as_restatement(d, fa, fasta_text, sites, bed, tag="run"):
    exp_out, exp_st = J.fetch(fasta_text, sites, bed)
    out, st = _run(d, fa, sites, bed, tag)
    assert out == exp_out, (tag, bed)
    assert {k: st[k] for k in J.INT_KEYS} == exp_st
    return out, st


def both_modes(sites):
    """(chrom, start, end, reverse) with FASTA names that start with "chr" -> the cluster table (names as they are) and the BED
    file (names without "chr", which fetchBed puts back; the strand in field 4), each behind a header line"""
    tab = [HEADER] + [row(c, s, e, b"-" if r else b"+", cid=b"cl%d" % i) for i, (c, s, e, r) in enumerate(sites)]
    bed = [b"track name=sites"] + [b"\t".join([c[3:], str(s).encode(), str(e).encode(), b"site%d" % i, b"-" if r else b"+"]) for i, (c, s, e, r) in enumerate(sites)]
    return b"\n".join(tab) + b"\n", b"\n".join(bed) + b"\n"


# ---- the hand-worked cases

@pytest.fixture(scope="module")
def hand(workdir):
    d = os.path.join(workdir, "fetch_hand")
    return d, _indexed(d, GENOME)


@pytest.mark.parametrize("key", sorted(CASES))
def test_hand_worked_cases(hand, key):
    d, fa = hand
    sites, bed, exp_out, exp_st = CASES[key]
    out, st = _same_as_restatement(d, fa, GENOME, sites, bed, key)
    assert out == exp_out                                                 # the hand-written bytes
    assert {k: st[k] for k in J.INT_KEYS} == exp_st
    assert st["n_pieces"] == 1


@pytest.mark.parametrize("key", sorted(ERRORS))
def test_errors_leave_the_directory_as_it_was(hand, key):
    import capi
    d, fa = hand
    sites, bed, what = ERRORS[key]
    src = os.path.join(d, "err_" + key + ".sites")
    with open(src, "wb") as f:
        f.write(sites)
    before = sorted(os.listdir(d))
    with pytest.raises(capi.PsError, match=what) as e:
        capi.ps_fetch_sequences(fa, src, os.path.join(d, "err_" + key + ".out"), bed)
    assert "err_" + key + ".sites" in str(e.value)                        # the file is named
    assert sorted(os.listdir(d)) == before


def test_file_errors(hand, tmp_path):
    import capi
    d, fa = hand
    src = str(tmp_path / "s.tsv")
    with open(src, "wb") as f:
        f.write(CASES["holes_both_strands"][0])
    for out, what in ((src, "one of the inputs"), (fa + ".pac", "one of the inputs"), (fa + ".ann", "one of the inputs"), (fa, "one of the inputs")):
        with pytest.raises(capi.PsError, match=what):
            capi.ps_fetch_sequences(fa, src, out, False)
    assert open(src, "rb").read() == CASES["holes_both_strands"][0]
    with pytest.raises(capi.PsError, match="nothing_here.fa.ann"):        # a missing index
        capi.ps_fetch_sequences(str(tmp_path / "nothing_here.fa"), src, str(tmp_path / "o"), False)
    with pytest.raises(capi.PsError, match="missing.tsv"):
        capi.ps_fetch_sequences(fa, str(tmp_path / "missing.tsv"), str(tmp_path / "o"), True)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["s.tsv"]
    # the FASTA itself is not opened: the index alone serves
    os.rename(fa, fa + ".away")
    try:
        out, _ = _run(d, fa, CASES["holes_both_strands"][0], False, "no_fasta")
    finally:
        os.rename(fa + ".away", fa)
    assert out == CASES["holes_both_strands"][2]


# ---- the edge genome

def edge_genome():
    """one: 1 base.  n_only: five N.  mix: 37 bases, holes at 1-3, a lone R at 18, nnn at 35-37, soft-masked bases between.
    long: 1,031 bases with a soft-masked stretch and N runs of 5, 6, 7 and 9 bases that begin at each of the four phases of the
    4-bases-per-byte packing (the contig starts at base 43 of the packed strand).  Its header carries an annotation."""
    rng = random.Random(20240611)
    mix = "NNN" + "ACgtTGcaACGTAC" + "R" + "gatTACAGATtaCAGT" + "nnn"
    assert len(mix) == 37 and mix[17] == "R"
    body = [rng.choice("ACGT") for _ in range(1031)]
    body[300:420] = [c.lower() for c in body[300:420]]
    for at, n in ((101, 5), (202, 6), (515, 7), (768, 9)):                # (43 + at) % 4 == 0, 1, 2, 3
        body[at:at + n] = "N" * n
    assert sorted((43 + at) % 4 for at in (101, 202, 515, 768)) == [0, 1, 2, 3]
    body = "".join(body)
    lines = "\n".join(body[i:i + 70] for i in range(0, 1031, 70))
    text = ">chrone\nG\n>chrn_only\nNNNNN\n>chrmix\n%s\n%s\n>chrlong soft-masked in part, with four N runs\n%s\n" % (mix[:20], mix[20:], lines)
    return text.encode()


@pytest.fixture(scope="module")
def edge(workdir):
    d = os.path.join(workdir, "fetch_edge")
    text = edge_genome()
    return d, _indexed(d, text), text


def mix_sites():
    """every (start, end) with 1 <= start <= end + 1 <= 38 on both strands: 1,482 sites"""
    return [(b"chrmix", s, e, r) for s in range(1, 39) for e in range(s - 1, 38) for r in (False, True)]


def test_every_site_of_a_short_contig(edge):
    d, fa, text = edge
    sites = mix_sites()
    assert len(sites) == 1482
    tab, bed = both_modes(sites)
    out, st = _same_as_restatement(d, fa, text, tab, False, "mix_tab")
    assert st["n_sites"] == 1482 and st["n_reverse"] == 741 and st["n_hole_bases"] > 0
    assert st["n_inverted"] == st["n_no_contig"] == st["n_past_end"] == st["n_before_start"] == 0
    _, st_bed = _same_as_restatement(d, fa, text, bed, True, "mix_bed")
    assert st_bed["n_bases"] == st["n_bases"] == 2 * sum(e - s + 1 for _, s, e, r in sites if r)


def test_sites_around_the_store_and_the_workgroup(edge):
    d, fa, text = edge
    sites = [(b"chrlong", s, s + n - 1, r) for n in (15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1031) for s in range(1, 6) for r in (False, True)]
    sites += [(b"chrone", 1, 1, False), (b"chrone", 1, 1, True), (b"chrn_only", 1, 5, True), (b"chrn_only", 2, 4, False), (b"chrone", 1, 2, False)]
    tab, bed = both_modes(sites)
    _, st = _same_as_restatement(d, fa, text, tab, False, "long_tab")
    assert st["n_past_end"] == 2 * 4 + 1                                  # 1,031 bases from starts 2-5 on both strands; chrone 1-2
    _same_as_restatement(d, fa, text, bed, True, "long_bed")


def test_more_sites_in_a_workgroup_than_are_staged(edge):
    """sites of 0, 1 and 2 bases by turns: one workgroup's 4 KiB of the stream hold about 4,000 of them, beyond the 1,024 whose
    offsets it stages, so its lanes bisect the whole table's offsets in place"""
    d, fa, text = edge
    sites = [(b"chrlong", 1 + i % 1000, i % 1000 + i % 3, i % 7 == 0) for i in range(9000)]
    tab, bed = both_modes(sites)
    _, st = _same_as_restatement(d, fa, text, tab, False, "short_tab")
    assert st["n_bases"] == 9000 and st["n_past_end"] == 0
    _same_as_restatement(d, fa, text, bed, True, "short_bed")


def test_pieces_do_not_change_the_output(edge, monkeypatch):
    d, fa, text = edge
    tab, _ = both_modes(mix_sites())
    exp_out, exp_st = J.fetch(text, tab, False)
    n_pieces = {}
    for piece in (16, 48, 4096, None):
        if piece is None:
            monkeypatch.delenv("PS_FETCH_PIECE")
        else:
            monkeypatch.setenv("PS_FETCH_PIECE", str(piece))
        out, st = _run(d, fa, tab, False, "piece_%s" % piece)
        assert out == exp_out, piece
        assert {k: st[k] for k in J.INT_KEYS} == exp_st
        assert st["n_pieces"] == (-(-st["n_bases"] // piece) if piece else 1)
        n_pieces[piece] = st["n_pieces"]
    assert n_pieces[16] != n_pieces[None] and n_pieces[16] > n_pieces[48] > n_pieces[4096] > 1
    monkeypatch.setenv("PS_FETCH_PIECE", "16")                            # an empty stream is one piece
    for sites in (HEADER + b"\n", CASES["inverted"][0]):
        out, st = _run(d, fa, sites, False, "piece_empty")
        assert st["n_bases"] == 0 and st["n_pieces"] == 1 and out == J.fetch(text, sites, False)[0]
    monkeypatch.setenv("PS_FETCH_PIECE", "17")                            # rounded up to 32
    _, st = _run(d, fa, tab, False, "piece_17")
    assert st["n_pieces"] == -(-st["n_bases"] // 32)


# ---- random genomes and sites

def fuzz_genome(rng):
    """20 contigs of 1-3,000 bases, soft-masked in part, with holes of random IUPAC letters in either case"""
    out, contigs = [], []
    for c in range(20):
        n = rng.choice((1, 2, 3, 17, 64, 3000)) if c < 6 else rng.randint(1, 3000)
        body = [rng.choice("ACGT") if rng.random() < 0.7 else rng.choice("acgt") for _ in range(n)]
        for _ in range(rng.randint(0, 6)):
            at, ch = rng.randrange(n), rng.choice("NNNnRYKMSWBDHVrykm")
            k = rng.choice((1, 1, 2, 3, 4, 5, 8, 40))
            body[at:at + k] = ch * min(k, n - at)
        body, name = "".join(body), "chr%d" % (c + 1)
        width = rng.choice((50, 60, 61, 3000))
        out.append(">%s%s\n%s\n" % (name, rng.choice(("", " an annotation", "\tv1")), "\n".join(body[i:i + width] for i in range(0, n, width))))
        contigs.append((name.encode(), n))
    return "".join(out).encode(), contigs


def fuzz_sites(rng, contigs, n_sites):
    """a tenth of the sites invalid in each of the four ways: start > end + 1, an unknown contig, an end past the contig, a
    start before base 1"""
    sites = []
    for _ in range(n_sites):
        name, n = rng.choice(contigs)
        s = rng.randint(1, n)
        e = min(n, s - 1 + rng.choice((0, 1, 2, 15, 16, 17, 41, 41, 41, rng.randint(0, 3000))))
        kind = rng.random()
        if kind < 0.1:
            s, e = e + rng.randint(2, 5), s - 1
        elif kind < 0.2:
            name = rng.choice((b"chr21", b"chrUn", name + b"_x", b"chrX"))
        elif kind < 0.3:
            e = n + rng.randint(1, 50)
        elif kind < 0.4:
            s = rng.randint(-40, 0)
        sites.append((name, s, e, rng.random() < 0.5))
    return sites


def test_random_genome_and_sites(workdir):
    rng = random.Random(0xF37C4)
    text, contigs = fuzz_genome(rng)
    d = os.path.join(workdir, "fetch_fuzz")
    fa = _indexed(d, text)
    sites = fuzz_sites(rng, contigs, 3000)
    tab, bed = both_modes(sites)
    _, st = _same_as_restatement(d, fa, text, tab, False, "fuzz_tab")
    assert min(st[k] for k in ("n_inverted", "n_no_contig", "n_past_end", "n_before_start")) >= 200 and st["n_hole_bases"] > 0
    _, st_bed = _same_as_restatement(d, fa, text, bed, True, "fuzz_bed")
    assert {k: st_bed[k] for k in J.INT_KEYS if k != "n_lines"} == {k: st[k] for k in J.INT_KEYS if k != "n_lines"}


# ---- after `clust`

def test_cluster_table_end_to_end(workdir):
    """the table ps_pileup_clusters writes goes through `fetch` as it is"""
    import capi
    from test_gpu_pileup_clusters import ragged_sam
    d = os.path.join(workdir, "fetch_e2e")
    sam_text, contig = ragged_sam(5150)
    text = (">chrR\n" + contig + "\n").encode()
    fa = _indexed(d, text)
    sam, table = os.path.join(d, "m.sam"), os.path.join(d, "clusters.tsv")
    with open(sam, "w") as f:
        f.write(sam_text)
    cl = capi.ps_pileup_clusters(sam, fa, table, None, 3, os.path.join(d, "sites"))
    sites = open(table, "rb").read()
    assert cl["n_clusters_written"] >= 20 and sites.count(b"\n") == cl["n_clusters_written"] + 1
    out, st = _same_as_restatement(d, fa, text, sites, False, "e2e")
    assert st["n_sites"] == cl["n_clusters_written"] and st["n_bases"] > 0 and st["n_inverted"] == st["n_no_contig"] == st["n_past_end"] == 0
    lines = [l.split(b"\t") for l in out.split(b"\n")[1:-1]]
    assert all(len(f) == 12 and len(f[11]) == int(f[3]) - int(f[2]) + 1 for f in lines)


def test_gzip_named_reference(workdir):
    d = os.path.join(workdir, "fetch_gz")
    fa = _indexed(d, gzip.compress(GENOME), "genome.fa.gz")
    assert os.path.exists(fa + ".ann") and os.path.exists(fa + ".pac")
    for key in ("holes_both_strands", "bed_chr_prefix"):
        sites, bed, exp_out, exp_st = CASES[key]
        out, st = _run(d, fa, sites, bed, key)
        assert out == exp_out and {k: st[k] for k in J.INT_KEYS} == exp_st
