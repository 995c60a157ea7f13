"""GPU tier of the search options (include/parasuite_hip.h: ps_search_opts): the product through ps_ctx_set_search and the staged
calls, through ps_map_opts and through `bin/bwa aln ... / samse -n ...`, against the CPU oracle under the same options -- hit-list
lengths, the first hit lists, @SQ lines and SAM line by line (test_gpu_parity._compare), in the fuzz also ps_batch_hits.

One genome for the module: simulate.example_genome() with a 12 x 37 tandem repeat, a 60-mer in 6 copies and a 60-mer in 3 copies
planted in it, indexed once.  Every deterministic case maps 4,096 reads in one launch (PS_ORDER_MIN: the effort order engages):
the reads built for the case, padded with simulated ones.

A test that ignored the option must not pass: every case also asserts that the ORACLE's SAM under the option differs from the
oracle's SAM under the defaults in at least `differ` records (the reference against itself, not the code under test).  Three options
change next to nothing on any input tried -- -i 0 (1-5 records), -d 0 and -d 200 (none): those are compared for equality only."""
import os
import subprocess

import numpy as np
import pytest

from conftest import sam_records
from test_capi_cpu import ROOT
from test_gpu_option_edges import _first_launch
from test_gpu_parity import _compare
from test_search_opts_cpu import FIELDS, FLAG, draw_options, opts, orc_fields

pytestmark = pytest.mark.gpu

N_READS = 4096
L = 50
TANDEM_AT, UNIT, COPIES = 50000, 37, 12
SIX_AT = [60000, 70000, 80000, 90000, 100000, 110000]
THREE_AT = [120000, 130000, 140000]


def planted_genome():
    import simulate as S
    (name, asc), = S.example_genome()
    asc = asc.copy()
    for t in range(COPIES):
        asc[TANDEM_AT + UNIT * t:TANDEM_AT + UNIT * (t + 1)] = asc[48000:48000 + UNIT]
    for at in SIX_AT[1:]:
        asc[at:at + 60] = asc[SIX_AT[0]:SIX_AT[0] + 60]
    for at in THREE_AT[1:]:
        asc[at:at + 60] = asc[THREE_AT[0]:THREE_AT[0] + 60]
    return [(name, asc)]


# ---- reads ----------------------------------------------------------------------------------------------------------------------
def _oriented(read, rng):
    return read if rng.random() < 0.5 else (3 - read[::-1]).astype(np.uint8)


def _window(fwd, rng, span):
    while True:
        p = int(rng.integers(150000, 200000))                 # plain sequence: behind the planted copies, in front of the second N run
        if (fwd[p:p + span] < 4).all():
            return p


def reads_two_gaps(fwd, n, rng):
    """one deleted reference base and one inserted base 20 bases apart: two gap opens, CIGARs of 5 operations"""
    out = np.empty((n, L), dtype=np.uint8)
    for r in range(n):
        p = _window(fwd, rng, L + 8)
        a = int(rng.integers(10, 16))
        ins = np.uint8((int(fwd[p + a + 21]) + 1 + int(rng.integers(0, 3))) & 3)
        read = np.concatenate([fwd[p:p + a], fwd[p + a + 1:p + a + 21], [ins], fwd[p + a + 21:p + L]])
        out[r] = _oriented(read.astype(np.uint8), rng)
    return out


def reads_gap4(fwd, n, rng):
    """a 4-base deletion or insertion in the middle"""
    out = np.empty((n, L), dtype=np.uint8)
    for r in range(n):
        p = _window(fwd, rng, L + 8)
        a = int(rng.integers(18, 30))
        if r & 1:
            read = np.concatenate([fwd[p:p + a], fwd[p + a + 4:p + L + 4]])
        else:
            read = np.concatenate([fwd[p:p + a], rng.integers(0, 4, 4).astype(np.uint8), fwd[p + a:p + L - 4]])
        out[r] = _oriented(read.astype(np.uint8), rng)
    return out


def reads_from_copies(fwd, n, rng, places):
    """50-mers out of repeated sequence, a third of them with one mismatch; places: (start, bases to choose the offset from)"""
    out = np.empty((n, L), dtype=np.uint8)
    for r in range(n):
        at, room = places[r % len(places)]
        p = at + int(rng.integers(0, room))
        read = fwd[p:p + L].copy()
        if r % 3 == 0:
            j = int(rng.integers(5, L - 5))
            read[j] = (read[j] + 1 + rng.integers(0, 3)) & 3
        out[r] = _oriented(read, rng)
    return out


class World:
    """the module's genome, both indexes and the read sets with the oracle's default answer, each made once"""

    def __init__(self, workdir):
        import capi
        import orc
        import simulate as S
        self.dir = os.path.join(workdir, "sopts")
        os.makedirs(self.dir, exist_ok=True)
        self.genome = planted_genome()
        self.fa = os.path.join(self.dir, "planted.fa")
        S.write_fasta(self.fa, self.genome)
        self.oix = orc.Index.from_fasta(self.fa)
        self.fwd = self.oix.forward_codes()
        self.ctx = capi.Ctx.build(self.fa, save_files=True)   # the index files: ps_map_opts and bin/bwa load them
        self.sets = {}

    def reads(self, name):
        """name -> (fastq path, the oracle's SAM records under the default options)"""
        import orc
        import simulate as S
        if name in self.sets:
            return self.sets[name]
        rng = np.random.default_rng(sum(name.encode()))
        sim = S.simulate_reads(self.genome, N_READS, L, seed=900 + len(name), indel_scale=40, n_frac=0.002)
        special = {"sim": None,
                   "two_gaps": lambda: reads_two_gaps(self.fwd, 300, rng),
                   "gap4": lambda: reads_gap4(self.fwd, 300, rng),
                   "repeats": lambda: reads_from_copies(self.fwd, 300, rng, [(TANDEM_AT, UNIT * COPIES - L - UNIT), (SIX_AT[2], 10)]),
                   "three": lambda: reads_from_copies(self.fwd, 300, rng, [(a, 10) for a in THREE_AT])}[name]
        if special:
            sp = special()
            sim["codes"][:sp.shape[0]] = sp                  # the built reads in front, simulated ones behind: 4,096 in all
        fq = os.path.join(self.dir, name + ".fq")
        S.write_fastq(fq, sim)
        osam = os.path.join(self.dir, name + ".default.orc.sam")
        self.oix.map_fastq(orc.stock_opt("0.04"), fq, osam, n_threads=8)
        self.sets[name] = (fq, sam_records(osam))
        return self.sets[name]


@pytest.fixture(scope="module")
def world(workdir):
    w = World(workdir)
    yield w
    w.ctx.close()


def _differ(a, b, head=None):
    """records that differ, among the first `head` (the built reads) or among all"""
    assert len(a) == len(b) == N_READS
    return sum(1 for x, y in zip(a[:head], b[:head]) if x != y)


def _tag(flags):
    return "-".join("%s%s" % kv for kv in flags.items())


# read set, options, records of the oracle's SAM that must differ from its default answer (None: equality only, see the docstring), the
# first `head` records only where the case is about the built reads
CASES = [
    ("sim", dict(o=0), 100, None),
    ("sim", dict(i=12), 100, None),
    ("sim", dict(m=50), 100, None),
    ("sim", dict(l=20), 100, None),
    ("sim", dict(l=20, k=0), 100, None),
    ("sim", dict(l=1000), 100, None),
    ("sim", dict(R=0), 100, None),
    ("sim", dict(o=2, e=3, l=24, k=1, M=4, O=9, E=2), 100, None),
    ("two_gaps", dict(o=2), 100, 300),
    ("gap4", dict(e=5), 100, 300),
    ("gap4", dict(e=8), 100, 300),
    ("repeats", dict(n=10), 100, 300),
    ("repeats", dict(n=20), 100, 300),
    ("repeats", dict(R=1), 100, 300),
    ("repeats", dict(R=4), 100, 300),
    ("repeats", dict(R=300, n=20), 100, 300),
    ("three", dict(n=0), 100, 300),
    ("two_gaps", dict(M=1, O=1, E=1), 5, None),              # score tables move few records on any input: on this set 18 and 9
    ("two_gaps", dict(M=5, O=6, E=1), 5, None),
    ("sim", dict(i=0), None, None),
    ("sim", dict(d=0), None, None),
    ("sim", dict(d=200), None, None),
]


@pytest.mark.parametrize("reads,flags,differ,head", CASES, ids=[c[0] + ":" + _tag(c[1]) for c in CASES])
def test_option_identical_to_oracle(world, monkeypatch, capfd, reads, flags, differ, head):
    import orc
    fq, default = world.reads(reads)
    d = opts(**flags)
    tag = reads + "_" + _tag(flags)
    world.ctx.set_stock("0.04")
    world.ctx.set_search(**d)
    monkeypatch.setenv("PS_VERBOSE", "1")
    capfd.readouterr()
    try:
        b = _compare(world.ctx, world.oix, orc.stock_opt("0.04", **orc_fields(d)), fq, world.dir, tag)
    finally:
        world.ctx.set_search(None)
    # the launch is the one the case is about: all 4,096 reads, on the wide stack exactly where launch_is_wide says so (gap limits that
    # add up to more than 7 -- at most 3 opens fit the 3 differences of -n 0.04 at 50 bp -- or -R from 255 on)
    o = orc_fields(d)
    n_first, wide = _first_launch(capfd.readouterr().err)
    assert n_first == N_READS and wide == (min(o["max_gapo"], 3) + o["max_gape"] > 7 or o["max_top2"] >= 255)
    if flags == dict(m=50):
        assert b.timing()["n_overflow_tier1"] > 0               # the narrow tier hands the reads that reach -m on
    under = sam_records(os.path.join(world.dir, tag + ".orc.sam"))
    n = _differ(under, default, head)
    print("%s: the oracle's SAM differs from its default answer in %d of %d records" % (tag, n, head or N_READS))
    if differ is not None:
        assert n >= differ


def test_two_gap_reads_are_unmapped_by_default_and_have_five_operations(world):
    """what the -o 2 case is built on, read off the oracle"""
    import orc
    fq, default = world.reads("two_gaps")
    assert all(int(l.split("\t")[1]) & 4 for l in default[:300])
    osam = os.path.join(world.dir, "two_gaps_check.orc.sam")
    world.oix.map_fastq(orc.stock_opt("0.04", **orc_fields(opts(o=2))), fq, osam, n_threads=8)
    cig = [l.split("\t")[5] for l in sam_records(osam)[:300]]
    assert sum(1 for c in cig if sum(c.count(op) for op in "MID") == 5) >= 250, cig[:5]


# ---- the other two routes -------------------------------------------------------------------------------------------------------
ROUTE_CASES = [("sim", dict(o=2, e=3, l=24, k=1, M=4, O=9, E=2)), ("repeats", dict(n=10, R=4))]


@pytest.mark.parametrize("reads,flags", ROUTE_CASES, ids=[c[0] + ":" + _tag(c[1]) for c in ROUTE_CASES])
def test_ps_map_opts_and_the_shim(world, reads, flags):
    import capi
    import orc
    fq, default = world.reads(reads)
    d = opts(**flags)
    tag = "route_" + reads + "_" + _tag(flags)
    osam = os.path.join(world.dir, tag + ".orc.sam")
    world.oix.map_fastq(orc.stock_opt("0.04", **orc_fields(d)), fq, osam, n_threads=8)
    exp = sam_records(osam)
    assert _differ(exp, default) >= 100
    out = os.path.join(world.dir, tag + ".map.sam")
    capi.ps_map(4, "0.04", None, None, world.fa, fq, out, search=d)
    assert sam_records(out) == exp
    bwa = os.path.join(ROOT, "para-suite_amd", "bin", "bwa")
    sai, out2 = os.path.join(world.dir, tag + ".sai"), os.path.join(world.dir, tag + ".bwa.sam")
    aln = [a for f in "oeidlkmMOER" for a in ("-" + f, str(d[FLAG[f]]))]
    subprocess.run([bwa, "aln", "-t", "4", "-n", "0.04"] + aln + [world.fa, fq, "-f", sai], check=True, timeout=300)
    subprocess.run([bwa, "samse", "-n", str(d["max_alt_hits"]), world.fa, sai, fq, "-f", out2], check=True, timeout=300)
    assert sam_records(out2) == exp


def test_shim_refusals_exit_1(world, workdir):
    bwa = os.path.join(ROOT, "para-suite_amd", "bin", "bwa")
    fq, _ = world.reads("sim")
    sai = os.path.join(world.dir, "refused.sai")
    for args, named in ((["-N"], "-N"), (["-q", "20"], "-q 20"), (["-o", "8"], "max_gap_opens")):
        r = subprocess.run([bwa, "aln"] + args + [world.fa, fq, "-f", sai], stderr=subprocess.PIPE, text=True, timeout=60)
        assert r.returncode == 1 and named in r.stderr and not os.path.exists(sai), (args, r.stderr)


# ---- rejections -----------------------------------------------------------------------------------------------------------------
def test_out_of_range_options_are_refused_before_any_launch(world, monkeypatch, capfd):
    import capi
    fq, _ = world.reads("sim")
    monkeypatch.setenv("PS_VERBOSE", "1")
    capfd.readouterr()
    for flags, field, limit in ((dict(o=8), "max_gap_opens", "0 to 7"), (dict(e=16), "max_gap_extensions", "at most 15"),
                                (dict(d=256), "max_del_occ", "0 to 255")):
        with pytest.raises(capi.PsError, match=field + r".*" + limit):
            world.ctx.set_search(**opts(**flags))
        with pytest.raises(capi.PsError, match=field + r".*" + limit):
            capi.ps_map(4, "0.04", None, None, world.fa, fq, os.path.join(world.dir, "refused.sam"), search=opts(**flags))
    assert not os.path.exists(os.path.join(world.dir, "refused.sam"))      # refused before the pass began
    try:
        world.ctx.set_stock("0.04")
        world.ctx.set_search(**opts(M=40, O=60, E=30))            # every field a byte; together past PS_MAX_BUCKETS: the batch call's error
        with pytest.raises(capi.PsError, match="PS_MAX_BUCKETS.*at most 128"):
            world.ctx.batch_from_fastq(fq)
        with pytest.raises(capi.PsError, match="PS_MAX_BUCKETS.*at most 128"):
            capi.ps_map(4, "0.04", None, None, world.fa, fq, os.path.join(world.dir, "refused.sam"), search=opts(M=40, O=60, E=30))
    finally:
        world.ctx.set_search(None)
    assert "launch" not in capfd.readouterr().err


def test_search_options_survive_set_stock_on_the_device(world):
    """ps_ctx_set_search, then ps_ctx_set_stock: the batch searches with both"""
    import orc
    fq, default = world.reads("two_gaps")
    d = opts(o=2)
    world.ctx.set_search(**d)
    world.ctx.set_stock("0.04")
    try:
        _compare(world.ctx, world.oix, orc.stock_opt("0.04", **orc_fields(d)), fq, world.dir, "order_two_gaps")
    finally:
        world.ctx.set_search(None)
    assert _differ(sam_records(os.path.join(world.dir, "order_two_gaps.orc.sam")), default) >= 300


# ---- fuzz -----------------------------------------------------------------------------------------------------------------------
HIT_FIELDS = ("pos", "type", "strand", "mapq", "n_mm", "n_gapo", "n_gape", "ref_shift", "score", "c1", "c2", "n_cigar", "n_multi")


@pytest.fixture(scope="module")
def fuzz_reads(world):
    """512 reads: some of every built kind, the rest simulated"""
    import simulate as S
    rng = np.random.default_rng(4242)
    sim = S.simulate_reads(world.genome, 512, L, seed=4243, indel_scale=40, n_frac=0.002)
    parts = [reads_two_gaps(world.fwd, 40, rng), reads_gap4(world.fwd, 40, rng),
             reads_from_copies(world.fwd, 40, rng, [(TANDEM_AT, UNIT * COPIES - L - UNIT), (SIX_AT[2], 10)]),
             reads_from_copies(world.fwd, 40, rng, [(a, 10) for a in THREE_AT])]
    sp = np.concatenate(parts)
    sim["codes"][:sp.shape[0]] = sp
    fq = os.path.join(world.dir, "fuzz.fq")
    S.write_fastq(fq, sim)
    return fq


@pytest.mark.parametrize("case", range(40))
def test_fuzz_all_twelve_fields(world, fuzz_reads, case):
    import orc
    d = draw_options(np.random.default_rng(77000 + case))
    tag = "fuzz%d" % case
    print(tag, " ".join("%s=%d" % (f, d[f]) for f in FIELDS))
    world.ctx.set_stock("0.04")
    world.ctx.set_search(**d)
    try:
        b = _compare(world.ctx, world.oix, orc.stock_opt("0.04", **orc_fields(d)), fuzz_reads, world.dir, tag)
    finally:
        world.ctx.set_search(None)
    hits = world.oix.map_fastq(orc.stock_opt("0.04", **orc_fields(d)), fuzz_reads, os.path.join(world.dir, tag + ".hits.orc.sam"), n_threads=8,
                               want_hits=512)["hits"]
    got = b.hits()
    exp_type = [h.type for h in hits]
    assert got["type"].tolist() == exp_type
    for r in np.nonzero(exp_type)[0]:
        h = hits[r]
        assert [int(got[f][r]) for f in HIT_FIELDS] == [int(getattr(h, f)) for f in HIT_FIELDS], (r, d)
        assert got["cigar"][r].tolist() == list(h.cigar), (r, d)
