"""GPU parity at the edges of the search's option ranges (include/parasuite_hip.h, ps_map): the product through its C ABI
against the CPU oracle -- hit-list lengths, the first hit lists, @SQ lines and SAM line by line (test_gpu_parity._compare).

Where the code path changes inside the accepted ranges (make_model in ps_model.h, launch_is_wide, run_search):
  - profile -X 0: no difference affordable, so no hand-out order; -X 5 and 7: narrow, order and estimate cap on; -X 8 and up:
    more than 64 score buckets, the wide stack; -X 10 and up: a budget whose effort model would not fit a CU's LDS (wide
    launches skip the order); -X 15: the largest budget;
  - -X -1: 7 differences up to 189 bp (narrow), 8 from 190 bp (wide), 9 at 250 bp; a ragged 36-250 bp launch is wide as a
    whole, short reads included;
  - stock -n 16 (63 buckets, narrow), 17 (66, wide), 37 (126, the largest); -n 0.04 at 250 bp;
  - out of range: -X 16, -n 38 (129 buckets) and a 251-bp read are errors.
Every deterministic case maps >= 4096 reads in one launch, so that the effort and order kernels run with default settings, and
shows that it tested something: its first-tier launch is wide exactly when the case says so, and the oracle's own hits (the
reference, not the code under test) number at least 100, at least 100 of them with a difference where the budget allows one."""
import os
import re

import numpy as np
import pytest

from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

N_READS = 4096              # PS_ORDER_MIN: the smallest launch that runs the effort and order kernels by default
LAUNCH = re.compile(r"backtrack launch: (\d+) reads x (\d+) bp, stack (\d+)( \(wide\))?")


def _profile():
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87          # a PAR-CLIP like T->C rate
    return P


def sim_fastq(genome, path, n_reads, L, seed, min_len=None):
    """simulated PAR-CLIP reads: T->C 0.12, indels, 0.2 % N"""
    import simulate as S
    S.write_fastq(path, S.simulate_reads(genome, n_reads, L, seed=seed, profile=_profile(), indel_scale=6.0, n_frac=0.002,
                                         min_len=min_len))
    return path


def repeat_genome(seed=91):
    """four repeat families of 40 copies each (300 bp, every copy 2 % diverged on its own, 50-bp spacers) and a plain contig: a
    read of a family matches many copies within a difference or two, each copy its own hit interval"""
    import simulate as S
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(4):
        unit = S.make_contig(300, rng, [], softmask_frac=0.0)
        for _ in range(40):
            cp = unit.copy()
            mut = rng.random(cp.size) < 0.02
            cp[mut] = S.BASES[rng.integers(0, 4, int(mut.sum()))]
            parts += [cp, S.make_contig(50, rng, [], softmask_frac=0.0)]
    return [("rep", np.concatenate(parts)), ("flat", S.make_contig(20000, rng, [], softmask_frac=0.0))]


def _first_launch(err):
    m = LAUNCH.findall(err)
    assert m, err
    n, _, _, w = m[0]
    return int(n), bool(w)


def _oracle_counts(sai):
    hit = sum(1 for x in sai if len(x))
    diff = sum(1 for x in sai if len(x) and int(x[0]["n_mm"]) + int(x[0]["n_gapo"]) + int(x[0]["n_gape"]) > 0)
    return hit, diff


def _check_case(err, sai, wide, budget):
    n, w = _first_launch(err)
    assert n >= N_READS and w == wide, (n, w, wide)
    hit, diff = _oracle_counts(sai)
    print("first launch %d reads%s; oracle: %d reads with a hit, %d with a difference" % (n, " (wide)" if w else "", hit, diff))
    assert hit >= 100
    if budget:
        assert diff >= 100


@pytest.fixture(scope="module")
def ctx_example(example):
    import capi
    c = capi.Ctx.build(example["fa"])
    yield c
    c.close()


# tag, cost model, its argument, read length, shortest read (ragged), wide, environment
CASES = [
    ("X0", "profile", 0, 50, None, False, {}),
    ("X5", "profile", 5, 50, None, False, {}),
    ("X7", "profile", 7, 50, None, False, {}),
    ("X8", "profile", 8, 50, None, True, {}),
    ("X9", "profile", 9, 50, None, True, {}),
    ("X10", "profile", 10, 50, None, True, {}),
    ("X12", "profile", 12, 50, None, True, {}),
    ("X15", "profile", 15, 50, None, True, {}),
    ("X7_cap_bias8", "profile", 7, 50, None, False, {"PS_CAP_BIAS": "8"}),     # every estimate 8 units low: restarts at the largest narrow budget
    ("Xm1_189bp", "profile", -1, 189, None, False, {}),
    ("Xm1_190bp", "profile", -1, 190, None, True, {}),
    ("Xm1_250bp", "profile", -1, 250, None, True, {}),
    ("Xm1_ragged_36_250bp", "profile", -1, 250, 36, True, {}),
    ("n16", "stock", "16", 50, None, False, {}),
    ("n17", "stock", "17", 50, None, True, {}),
    ("n37", "stock", "37", 50, None, True, {}),
    ("n0.04_250bp", "stock", "0.04", 250, None, False, {}),
]


@pytest.mark.parametrize("tag,mode,arg,L,min_len,wide,env", CASES, ids=[c[0] for c in CASES])
def test_option_edge_identical_to_oracle(ctx_example, example, workdir, monkeypatch, capfd, tag, mode, arg, L, min_len, wide, env):
    import orc
    fq = sim_fastq(example["genome"], os.path.join(workdir, "edge_%s.fq" % tag), N_READS, L, seed=5000 + L + (min_len or 0), min_len=min_len)
    if mode == "stock":
        ctx_example.set_stock(arg)
        opt = orc.stock_opt(arg)
    else:
        ctx_example.set_profile(_profile(), 2.1e-5, 5.9e-4, arg)
        opt = orc.profile_opt(_profile(), 2.1e-5, 5.9e-4, arg)
    monkeypatch.setenv("PS_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    _compare(ctx_example, example["orc_index"], opt, fq, workdir, "edge_" + tag)
    err = capfd.readouterr().err
    _check_case(err, orc.read_sai(os.path.join(workdir, "edge_%s.orc.sai" % tag)), wide, arg != 0)


def test_wide_launch_escalates_tiers(workdir, monkeypatch, capfd):
    """-X 12 (wide from the first tier) on a genome of tandem and dispersed copies: reads with more hit intervals than the first
    tier holds (8) go to the next tier, and the results still equal the oracle's"""
    import capi
    import orc
    import simulate as S
    g = repeat_genome()
    fa = os.path.join(workdir, "edge_repeats.fa")
    S.write_fasta(fa, g)
    fq = sim_fastq(g, os.path.join(workdir, "edge_repeats.fq"), N_READS, 50, seed=6001)
    ctx = capi.Ctx.build(fa)
    try:
        ctx.set_profile(_profile(), 2.1e-5, 5.9e-4, 12)
        monkeypatch.setenv("PS_VERBOSE", "1")
        capfd.readouterr()
        b = _compare(ctx, orc.Index.from_fasta(fa), orc.profile_opt(_profile(), 2.1e-5, 5.9e-4, 12), fq, workdir, "edge_repeats")
        err = capfd.readouterr().err
        sai = orc.read_sai(os.path.join(workdir, "edge_repeats.orc.sai"))
        _check_case(err, sai, True, True)
        assert sum(1 for x in sai if len(x) > 8) >= 20                   # on the oracle: reads that outgrow the first tier's hit list
        assert b.timing()["n_overflow_tier1"] > 0
    finally:
        ctx.close()


def _write_profile_files(workdir, P, ins, dele):
    ep, ip = os.path.join(workdir, "edge.errorprofile"), os.path.join(workdir, "edge.indelprofile")
    with open(ep, "w") as f:
        for row in P:
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    with open(ip, "w") as f:
        f.write(repr(float(ins)) + "\t" + repr(float(dele)))
    return ep, ip


def test_out_of_range_options_are_errors(ctx_example, example, workdir):
    """-X 16 and stock -n 38 (129 score buckets, PS_MAX_BUCKETS = 128) and a 251-bp read (PS_MAX_LEN = 250): an error that names
    the limit, from the batch API and from ps_map -- never a launch"""
    import capi
    fq = sim_fastq(example["genome"], os.path.join(workdir, "edge_reject.fq"), 200, 50, seed=6101)
    fq251 = os.path.join(workdir, "edge_251.fq")
    seq = "".join("ACGT"[i % 4] for i in range(251))
    with open(fq251, "w") as f:
        f.write("@r251\n" + seq + "\n+\n" + "I" * 251 + "\n")
    fa = example["fa"]
    if not os.path.exists(fa + ".bwt"):
        capi.ps_index(fa)
    ep, ip = _write_profile_files(workdir, _profile(), 2.1e-5, 5.9e-4)
    ctx_example.set_profile(_profile(), 2.1e-5, 5.9e-4, 16)
    with pytest.raises(capi.PsError, match="PS_MAX_BUCKETS"):
        ctx_example.batch_from_fastq(fq)
    ctx_example.set_stock("38")
    with pytest.raises(capi.PsError, match="PS_MAX_BUCKETS"):
        ctx_example.batch_from_fastq(fq)
    ctx_example.set_stock("0.04")
    with pytest.raises(capi.PsError, match="PS_MAX_LEN"):
        ctx_example.batch_from_fastq(fq251)
    out = os.path.join(workdir, "edge_reject.sam")
    for mm, e, i, reads, limit in (("16", ep, ip, fq, "PS_MAX_BUCKETS"), ("38", None, None, fq, "PS_MAX_BUCKETS"),
                                   ("0.04", None, None, fq251, "PS_MAX_LEN")):
        with pytest.raises(capi.PsError, match=limit):
            capi.ps_map(4, mm, e, i, fa, reads, out)


def test_ps_map_argv_profile_x10(example, workdir, monkeypatch, capfd):
    """the argv path the Java runs (`-X 10` with profile files) on 4096 reads: one wide first-tier launch, SAM == oracle"""
    import capi
    import orc
    from conftest import sam_records
    P, ins, dele = _profile(), 2.1e-5, 5.9e-4
    ep, ip = _write_profile_files(workdir, P, ins, dele)
    fq = sim_fastq(example["genome"], os.path.join(workdir, "edge_argv.fq"), N_READS, 50, seed=6201)
    fa = example["fa"]
    if not os.path.exists(fa + ".bwt"):
        capi.ps_index(fa)
    out, osam, osai = (os.path.join(workdir, "edge_argv" + s) for s in (".sam", ".orc.sam", ".orc.sai"))
    monkeypatch.setenv("PS_VERBOSE", "1")
    capfd.readouterr()
    capi.ps_map(8, "10", ep, ip, fa, fq, out)
    err = capfd.readouterr().err
    example["orc_index"].map_fastq(orc.profile_opt(P, ins, dele, 10), fq, osam, sai_out=osai, n_threads=8)
    _check_case(err, orc.read_sai(osai), True, True)
    g, o = sam_records(out), sam_records(osam)
    assert len(g) == len(o) == N_READS
    bad = [i for i in range(len(g)) if g[i] != o[i]]
    assert not bad, (len(bad), g[bad[0]], o[bad[0]])


def test_edge_range_fuzz(monkeypatch):
    """tests/fuzz_parity.py with ranges="edges" (profile -X 4..15, stock -n 5..37, reads up to 250 bp, ragged ones too), every
    launch through the effort block (PS_ORDER_MIN=1).  Seed 21's forty cases take the oracle at most 0.4 s each on 8 threads."""
    import fuzz_parity
    monkeypatch.setenv("PS_ORDER_MIN", "1")
    assert fuzz_parity.run(40, 21, ranges="edges") == 40
