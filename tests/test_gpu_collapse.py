"""GPU tier: the collapsed search (ps_ctx_set_collapse / PS_COLLAPSE; csrc/ps_collapse.h, ps_collapse.hip) -- the identical reads of a
bin are searched once and the result is copied to the others.  Every output must stay what it is without the feature, so the
reference is the CPU oracle (test_gpu_parity._compare: hit-list lengths, the first hit lists, @SQ lines, SAM line by line), and the
groups handed to the caller are held against a Python dict keyed on (length, sequence text)."""
import os
import re
import subprocess
import threading

import numpy as np
import pytest

import collapse_reads as R
from conftest import sam_records
from test_gpu_option_edges import _profile, _write_profile_files, repeat_genome
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INS, DEL = 2.1e-5, 5.9e-4


def _sim_seqs(genome, n, L, seed, min_len=None, exact=False):
    """n DIFFERENT simulated PAR-CLIP reads as text (T->C 0.12, indels, 0.2 % N); exact: stretches of the genome as they are"""
    import simulate as S
    drawn = n + n // 8 + 16                                   # two draws may give the same read: the first n different ones
    if exact:
        sim = S.simulate_reads(genome, drawn, L, seed=seed, bound=0.0, profile=np.eye(4), min_len=min_len)
    else:
        sim = S.simulate_reads(genome, drawn, L, seed=seed, profile=_profile(), indel_scale=6.0, n_frac=0.002, min_len=min_len)
    lut = np.frombuffer(b"ACGTN", dtype=np.uint8)
    seqs = list(dict.fromkeys(lut[np.minimum(sim["codes"][i, :sim["lens"][i]], 4)].tobytes().decode() for i in range(drawn)))[:n]
    assert len(seqs) == n
    return seqs


def _open(fa, x=5, collapse=1, stock=None):
    import capi
    ctx = capi.Ctx.build(fa)
    if stock is None:
        ctx.set_profile(_profile(), INS, DEL, x)
    else:
        ctx.set_stock(stock)
    ctx.set_collapse(collapse)
    return ctx


def _run_sam(ctx, fq, out):
    b = ctx.batch_from_fastq(fq)
    b.run(4)
    b.write_sam(out)
    return b, sam_records(out)


def _check_groups(b, seqs, complete=True):
    want = R.groups_of(seqs)
    dup = b.duplicate_of()
    assert len(dup) == len(seqs)
    R.check_groups_exact(seqs, dup)
    if complete:
        assert R.partition(dup) == {tuple(v) for v in want.values()}
    return want, dup


@pytest.fixture(scope="module")
def dup6000(example, workdir):
    """6,000 reads from 729 different ones: one group of 1,500, one of 257, fifteen each of 63, 64 and 65, the rest 1, 2 or 3 copies,
    and the pairs the grouping rule must keep apart (collapse_reads.adversarial_reads); 36-50 bp ragged, 0.2 % N, shuffled"""
    rng = np.random.default_rng(6000)
    mult = [1500, 257] + [63, 64, 65] * 15 + [1, 2, 3] * 223 + [1]
    distinct = _sim_seqs(example["genome"], len(mult), 50, seed=7101, min_len=36)
    adv = R.adversarial_reads(rng)
    distinct += adv
    mult += [1 + (i % 3) for i in range(len(adv))]
    assert len(set(distinct)) == len(distinct) == 729 and sum(mult) == 6000
    seqs = R.with_multiplicities(distinct, mult, rng)
    fq = R.write_fastq(os.path.join(workdir, "collapse6000.fq"), seqs, rng)
    return dict(seqs=seqs, fq=fq, groups=R.groups_of(seqs))


def test_identity_against_the_oracle(example, workdir, dup6000, monkeypatch):
    import orc
    seqs, want = dup6000["seqs"], dup6000["groups"]
    opt = orc.profile_opt(_profile(), INS, DEL, 5)
    ctx = _open(example["fa"])
    try:
        b = _compare(ctx, example["orc_index"], opt, dup6000["fq"], workdir, "collapse6000")
        ci = b.collapse_info()
        print(ci)
        assert ci["n_reads"] == 6000 and ci["n_groups"] == len(want) == 729 and ci["n_searched"] == ci["n_groups"]
        assert ci["largest"] == 1500 and ci["n_multi"] == sum(1 for v in want.values() if len(v) > 1)
        assert 1 <= ci["n_bins_collapsed"] <= ci["n_bins"]
        _check_groups(b, seqs)
        # 16 keys for 729 different reads: the comparison in full is what separates them; identical reads may end in two groups
        monkeypatch.setenv("PS_COLLAPSE_HASH_BITS", "4")
        b = _compare(ctx, example["orc_index"], opt, dup6000["fq"], workdir, "collapse6000_bits4")
        ci = b.collapse_info()
        print(ci)
        assert ci["n_searched"] >= len(want) and ci["n_searched"] == ci["n_groups"] and ci["n_searched"] < 6000
        _check_groups(b, seqs, complete=False)
    finally:
        ctx.close()


def test_tie_break_stream_and_tiers(workdir):
    """-X 12 on diverged repeat copies, every read eight times: reads with several best-score intervals draw from the tie-break
    stream (one stream in input order: the copies draw one after the other), reads with more than 8 intervals go to the larger tiers,
    where only the representatives are searched"""
    import orc
    import simulate as S
    g = repeat_genome()
    fa = os.path.join(workdir, "collapse_repeats.fa")
    S.write_fasta(fa, g)
    rng = np.random.default_rng(4096)
    distinct = _sim_seqs(g, 512, 50, seed=6001)
    seqs = R.with_multiplicities(distinct, [8] * 512, rng)
    fq = R.write_fastq(os.path.join(workdir, "collapse_repeats.fq"), seqs, rng)
    ctx = _open(fa, x=12)
    try:
        b = _compare(ctx, orc.Index.from_fasta(fa), orc.profile_opt(_profile(), INS, DEL, 12), fq, workdir, "collapse_repeats")
        sai = orc.read_sai(os.path.join(workdir, "collapse_repeats.orc.sai"))      # the reference's own hit lists show what was tested
        assert len(sai) == 4096
        ties = sum(1 for x in sai if len(x) >= 2 and int(x[1]["score"]) == int(x[0]["score"]))
        wide = sum(1 for x in sai if len(x) > 8)
        print("oracle: reads with several best-score intervals", ties, "with more than 8 intervals", wide)
        assert ties >= 20 and wide >= 20
        ci, tm = b.collapse_info(), b.timing()
        print(ci)
        assert 0 < ci["n_overflow_searched"] < ci["n_overflow_reads"]
        assert ci["n_overflow_reads"] == tm["n_overflow_tier1"] + tm["n_overflow_tier2"]         # the old counters keep counting reads
        assert ci["n_groups"] == 512 and ci["n_searched"] == 512
        _check_groups(b, seqs)
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def u_and_d(example, workdir):
    """U: 2,048 different reads; D: U four times over, shuffled"""
    rng = np.random.default_rng(2048)
    u = _sim_seqs(example["genome"], 2048, 50, seed=7301, min_len=36)
    d = R.with_multiplicities(u, [4] * 2048, rng)
    return dict(u=u, d=d, fq_u=R.write_fastq(os.path.join(workdir, "collapse_u.fq"), u, rng),
                fq_d=R.write_fastq(os.path.join(workdir, "collapse_d.fq"), d, rng))


def test_the_work_really_fell(example, u_and_d):
    """the counting kernel (ps_ctx_set_stats) counts what ran.  Stock costs: every launch here takes the same path whatever its
    size (under profile costs a launch of 4,096 reads or more spares entries by an estimate that smaller launches do not make)"""
    nodes = {}
    for tag, fq, collapse in (("U", u_and_d["fq_u"], 0), ("D on", u_and_d["fq_d"], 1), ("D off", u_and_d["fq_d"], 0)):
        ctx = _open(example["fa"], stock="0.04", collapse=collapse)
        try:
            ctx.set_stats(True)
            b = ctx.batch_from_fastq(fq)
            b.search()
            nodes[tag] = b.kstats(1)["nodes"]
            ci = b.collapse_info()
            assert ci["n_searched"] == (2048 if tag != "D off" else 8192) and ci["n_reads"] == (2048 if tag == "U" else 8192)
        finally:
            ctx.close()
    print(nodes)
    assert nodes["U"] > 0
    assert nodes["D on"] == nodes["U"]
    assert nodes["D off"] == 4 * nodes["U"]


def test_declined_without_duplicates(example, workdir, u_and_d):
    sams = {}
    for collapse in (1, 0):
        ctx = _open(example["fa"], collapse=collapse)
        try:
            b, sams[collapse] = _run_sam(ctx, u_and_d["fq_u"], os.path.join(workdir, "collapse_u_%d.sam" % collapse))
            ci = b.collapse_info()
            assert ci["n_searched"] == ci["n_reads"] == 2048 and ci["n_bins_collapsed"] == 0
            if collapse:
                assert ci["n_groups"] == 2048 and ci["n_multi"] == 0 and ci["largest"] == 1 and ci["n_bins"] >= 1
                assert b.duplicate_of().tolist() == list(range(2048))
            else:
                import capi
                assert ci["n_groups"] == 0 and ci["n_bins"] == 0 and ci["ms_collapse"] == 0
                with pytest.raises(capi.PsError, match="collapse off"):
                    b.duplicate_of()
        finally:
            ctx.close()
    assert sams[1] == sams[0] and len(sams[1]) == 2048


@pytest.mark.parametrize("tag", ["one_read", "65_copies", "4097_one_pair"])
def test_edges(example, workdir, tag):
    import orc
    rng = np.random.default_rng(len(tag))
    if tag == "one_read":
        seqs = _sim_seqs(example["genome"], 1, 50, seed=7501)
    elif tag == "65_copies":
        seqs = _sim_seqs(example["genome"], 1, 50, seed=7502) * 65
    else:
        u = _sim_seqs(example["genome"], 4096, 50, seed=7503, min_len=36)
        seqs = R.with_multiplicities(u, [2] + [1] * 4095, rng)
    fq = R.write_fastq(os.path.join(workdir, "collapse_%s.fq" % tag), seqs, rng)
    ctx = _open(example["fa"])
    try:
        b = _compare(ctx, example["orc_index"], orc.profile_opt(_profile(), INS, DEL, 5), fq, workdir, "collapse_" + tag)
        ci = b.collapse_info()
        assert ci["n_reads"] == len(seqs) and ci["n_searched"] == len(set(seqs)) == ci["n_groups"]
        _check_groups(b, seqs)
    finally:
        ctx.close()


def test_more_reads_than_one_wave_per_sort_chunk(example, workdir):
    """140,000 reads: more than PS_SORT_MAX_WG x 64 = 131,072, so every one of the 2,048 chunks of the sort, of the heads and of the
    compaction holds more than one wave's worth and every kernel takes the carries of chunks in front of it from more than 64 of them.
    Exact 36-bp reads, stock -n 0; collapse on against collapse off of the same build (the off path is held to the oracle by the
    tests above and by the rest of the suite; the oracle itself would take longer here than a test should)"""
    rng = np.random.default_rng(140000)
    u = _sim_seqs(example["genome"], 9000, 36, seed=7601, exact=True)
    mult = rng.multinomial(140000 - 9000, np.full(9000, 1 / 9000.0)) + 1
    seqs = R.with_multiplicities(u, [int(m) for m in mult], rng)
    assert len(seqs) == 140000
    fq = R.write_fastq(os.path.join(workdir, "collapse_140k.fq"), seqs, rng)
    sams = {}
    for collapse in (1, 0):
        ctx = _open(example["fa"], stock="0", collapse=collapse)
        try:
            b, sams[collapse] = _run_sam(ctx, fq, os.path.join(workdir, "collapse_140k_%d.sam" % collapse))
            if collapse:
                ci = b.collapse_info()
                print(ci)
                assert ci["n_reads"] == 140000 and ci["n_searched"] == ci["n_groups"] == 9000 and ci["largest"] == int(mult.max())
                _check_groups(b, seqs)
        finally:
            ctx.close()
    assert len(sams[1]) == 140000
    assert all(not int(l.split("\t")[1]) & 4 for l in sams[0])        # exact reads: every one is placed
    bad = [i for i in range(140000) if sams[1][i] != sams[0][i]]
    assert not bad, (len(bad), sams[1][bad[0]], sams[0][bad[0]])


def test_file_level_ps_map_and_the_shim(example, workdir, dup6000, monkeypatch, capfd):
    """PS_COLLAPSE=1 reaches ps_map and the argv shim through the search's knobs; the input cut into pieces (the groups are per bin of
    a piece, the tie-break stream is carried from piece to piece): the SAM file is byte for byte the one without the knob"""
    import capi
    rng = np.random.default_rng(7)
    fq = os.path.join(workdir, "collapse_file.fq")
    with open(fq, "w") as f:                                  # long names: 3 MB of FASTQ, three pieces of 1 MB
        for i, s in enumerate(dup6000["seqs"]):
            f.write("@r%d_%s\n%s\n+\n%s\n" % (i, "x" * 400, s, "".join(chr(33 + v) for v in rng.integers(3, 41, len(s)))))
    assert os.path.getsize(fq) > (5 << 20) // 2
    fa = example["fa"]
    if not os.path.exists(fa + ".bwt"):
        capi.ps_index(fa)
    ep, ip = _write_profile_files(workdir, _profile(), INS, DEL)
    monkeypatch.setenv("PS_CHUNK_MB", "1")
    monkeypatch.setenv("PS_VERBOSE", "1")
    out = {}
    for knob in ("1", None):
        if knob:
            monkeypatch.setenv("PS_COLLAPSE", knob)
        else:
            monkeypatch.delenv("PS_COLLAPSE")
        path = os.path.join(workdir, "collapse_file_%s.sam" % knob)
        capfd.readouterr()
        capi.ps_map(4, "5", ep, ip, fa, fq, path)
        err = capfd.readouterr().err
        assert len(re.findall(r"piece (\d+) on device 0 worker (\d+)", err)) >= 3, err
        assert ("collapsed search:" in err) == bool(knob)
        out[knob] = open(path, "rb").read()
    assert out["1"] == out[None] and out["1"].count(b"\n") > 6000
    bwa = os.path.join(ROOT, "para-suite_amd", "bin", "bwa")
    env = dict(os.environ, PS_COLLAPSE="1")                   # the argv route: `parasuite` only records its arguments, `samse` maps
    sai, path = os.path.join(workdir, "collapse_shim.sai"), os.path.join(workdir, "collapse_shim.sam")
    subprocess.run([bwa, "parasuite", "-t", "4", "-X", "5", "-p", ep, "-g", ip, fa, fq, "-f", sai], check=True, timeout=300, env=env)
    r = subprocess.run([bwa, "samse", fa, sai, fq, "-f", path], check=True, timeout=300, env=env, stderr=subprocess.PIPE, text=True)
    assert "collapsed search:" in r.stderr, r.stderr
    assert sam_records(path) == sam_records(os.path.join(workdir, "collapse_file_None.sam"))


class _OneAtATime:
    """the context with its batches created one after the other, and the oracle (one tie-break generator per process) with its runs
    one after the other; the four stages of the two batches run from both threads at once"""

    def __init__(self, obj):
        self.obj, self.lock = obj, threading.Lock()

    def batch_from_fastq(self, fq):
        with self.lock:
            return self.obj.batch_from_fastq(fq)

    def map_fastq(self, *a, **kw):
        with self.lock:
            return self.obj.map_fastq(*a, **kw)


def test_two_lanes_both_collapsed(example, workdir, dup6000):
    """two batches on two lanes, driven from two threads: each lane has its own collapse scratch"""
    import orc
    rng = np.random.default_rng(2)
    seqs2 = R.with_multiplicities(_sim_seqs(example["genome"], 900, 50, seed=7801, min_len=36), [5] * 900, rng)
    jobs = [("collapse_lane0", dup6000["fq"], dup6000["seqs"]),
            ("collapse_lane1", R.write_fastq(os.path.join(workdir, "collapse_lane1.fq"), seqs2, rng), seqs2)]
    ctx = _open(example["fa"])
    try:
        ctx.set_lanes(2)
        shared, oix, opt, got, err = _OneAtATime(ctx), _OneAtATime(example["orc_index"]), orc.profile_opt(_profile(), INS, DEL, 5), {}, []

        def lane(tag, fq):
            try:
                got[tag] = _compare(shared, oix, opt, fq, workdir, tag)
            except BaseException as e:               # noqa: BLE001
                err.append((tag, e))

        th = [threading.Thread(target=lane, args=(tag, fq)) for tag, fq, _ in jobs]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        for tag, _, seqs in jobs:
            ci = got[tag].collapse_info()
            assert ci["n_reads"] == len(seqs) and ci["n_searched"] == len(set(seqs))
            _check_groups(got[tag], seqs)
    finally:
        ctx.close()
