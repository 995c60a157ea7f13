"""GPU tier: the index builder (ps_index.hip), the Occ addressing (ps_core.h) and the locate stage (ps_samse.hip) on the edge texts
of tests/index_edges.py -- what the fixture genomes leave to chance or never reach:

  * the doubling rounds of the suffix sorter with most of the text still tied (periodic, one-symbol, duplicated and
    self-reverse-complementary texts), round 0 on texts shorter than its 28-symbol key and with empty chunks;
  * `primary` at 1 and at seq_len; seq_len on the boundaries of the 192-symbol Occ block, the 32-row SA sample and the 4096-symbol
    tile of k_collect; the jump table deeper than the text warrants;
  * reads on the forward/reverse junction, reads as long as the text and longer.

Every index is held against a plain sort of the suffixes (index_edges.plain_index) AND against the oracle's index; every SAM
against the oracle's on the same files.  Each case is one build of a text of at most 8192 bases and two small batches."""
import os

import numpy as np
import pytest

import index_edges as IE
from conftest import sam_records
from test_gpu_parity import _check_index, _compare

pytestmark = pytest.mark.gpu

MODES = ("stock", "profile")
DEFAULT_TIERS = dict(pool_cap=[16384, 65535, 2000064], aln_cap=[8, 256, 65536], bt_blocks=0)


def _set_mode(ctx, mode):
    """the context's options and the oracle's for the same cost model"""
    import orc
    if mode == "stock":
        ctx.set_stock("0.04")
        return orc.stock_opt("0.04")
    P = IE.profile_matrix()
    ctx.set_profile(P, IE.INS_RATE, IE.DEL_RATE, IE.X_ARG)
    return orc.profile_opt(P, IE.INS_RATE, IE.DEL_RATE, IE.X_ARG)


def _fasta(name, workdir):
    d = os.path.join(workdir, "edges_gpu")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, name + ".fa")
    if not os.path.exists(fa):
        IE.TEXT_BY_NAME[name].write_fasta(fa)
    return fa


def _case(name, workdir, ctx):
    """a built context with the plain reference, the oracle's index and the edge reads of its text"""
    import orc
    text = IE.TEXT_BY_NAME[name]
    fa = _fasta(name, workdir)
    fwd = IE.unpack_pac(ctx.fetch(2), text.l_pac)            # an N position holds a drawn base: the text is what was packed
    IE.assert_pac_matches_fasta(fwd, text)
    if not text.has_n:
        assert np.array_equal(fwd, IE.codes_of(text.ascii))
    fq = fa[:-3] + ".fq"
    with open(fq, "w") as f:
        f.write(IE.edge_reads(IE.string_of(fwd), seed=1000 + IE.NAMES.index(name)))
    return dict(name=name, text=text, fa=fa, fq=fq, dir=os.path.dirname(fa), ctx=ctx, plain=IE.plain_index(fwd), oix=orc.Index.from_fasta(fa))


@pytest.fixture(scope="module", params=IE.NAMES)
def case(request, workdir):
    import capi
    ctx = capi.Ctx.build(_fasta(request.param, workdir))
    yield _case(request.param, workdir, ctx)
    ctx.close()


def test_index_against_plain_sort_and_oracle(case):
    ctx, plain, name = case["ctx"], case["plain"], case["name"]
    info = ctx.info()
    _check_index(ctx, plain)
    _check_index(ctx, case["oix"])
    syms, cnts = ctx.bwt_syms()
    IE.assert_index_equals_plain(plain, info.seq_len, info.primary, list(info.L2), syms, ctx.sa_samples())
    assert info.n_blocks == plain.n_blocks and info.n_sa == plain.n_sa
    assert np.array_equal(cnts.astype(np.int64), plain.occ_blocks)
    n = plain.seq_len
    sa = ctx.sa_lookup(np.arange(1, n + 1, dtype=np.uint64))                    # every row, either side of primary included
    bad = np.flatnonzero(sa.astype(np.int64) != plain.sa[1:]) + 1
    assert bad.size == 0, ("sa_lookup differs at rows", bad[:5].tolist(), "primary", plain.primary)
    r = ctx.index_check()
    assert r["rows"] == n + 1 and r["bad_symbols"] == 0 and r["bad_samples"] == 0, r
    L = plain.longest_repeat()
    print("EDGE_INDEX %s seq_len=%d primary=%d sa_rounds=%d min_rounds=%d longest_repeat=%d longest_arc=%d" % (
        name, info.seq_len, info.primary, info.sa_rounds, plain.min_sa_rounds(), L, r["longest_arc"]))
    if L >= IE.KEY_SYMS:                                                         # the doubling loop really ran (a lower bound)
        assert info.sa_rounds >= 2 + int(np.floor(np.log2(L / IE.KEY_SYMS))), (info.sa_rounds, L)
    if name in ("A300", "C96"):
        assert info.primary == 1
    if name in ("T300", "G97"):
        assert info.primary == info.seq_len


@pytest.mark.parametrize("mode", MODES)
def test_edge_reads_match_oracle(case, mode):
    ctx, name, text = case["ctx"], case["name"], case["text"]
    opt = _set_mode(ctx, mode)
    tag = "%s_%s" % (name, mode)
    _compare(ctx, case["oix"], opt, case["fq"], case["dir"], tag)
    rec = sam_records(os.path.join(case["dir"], tag + ".gpu.sam"))
    info = ctx.info()
    print("EDGE_READS %s %s seq_len=%d primary=%d sa_rounds=%d mapped=%d unmapped=%d gapped=%d xa=%d" % (
        (name, mode, info.seq_len, info.primary, info.sa_rounds) + IE.sam_counts(rec)))
    exact = [l for l in rec if l.startswith(IE.JUNCTION_EXACT)]
    assert len(exact) >= 2
    if text.kind == "random" and text.l_pac >= 48:          # no repeat: a read on the junction has nowhere else to go
        assert [int(l.split("\t")[1]) for l in exact] == [4] * len(exact)


def test_small_tiers_on_a_duplicated_text(workdir):
    """x + x as two contigs, every window twice in the text: a first search tier of 64 stack entries and 2 hits per read
    (stack growth inside the launch, larger tiers where that is not enough) must give the same output as the default tiers"""
    import capi
    ctx = capi.Ctx.build(_fasta("x_x_two_contigs", workdir))
    c = _case("x_x_two_contigs", workdir, ctx)
    assert ctx.info().n_contigs == 2
    out = {}
    try:
        for mode in MODES:
            opt = _set_mode(ctx, mode)
            for tag, tiers in (("default", DEFAULT_TIERS), ("small", dict(pool_cap=[64, 4096, 2000064], aln_cap=[2, 64, 65536]))):
                ctx.set_tiers(**tiers)
                t = "tiers_%s_%s" % (mode, tag)
                b = _compare(ctx, c["oix"], opt, c["fq"], c["dir"], t)
                print("EDGE_TIERS %s %s overflow_tier1=%d overflow_tier2=%d" % (mode, tag, b.timing()["n_overflow_tier1"], b.timing()["n_overflow_tier2"]))
                out[mode, tag] = open(os.path.join(c["dir"], t + ".gpu.sam")).read()
            assert out[mode, "default"] == out[mode, "small"]
    finally:
        ctx.set_tiers(**DEFAULT_TIERS)
        ctx.close()


def _jump_levels_for(seq_len):
    """ps_core.h: jump_levels_for"""
    k = 0
    while k < 14 and (seq_len >> (2 * k)) >= 48:
        k += 1
    return k


@pytest.mark.parametrize("name", ["A300", "ACGT1024", "rand2048"])
def test_jump_table_depth_does_not_change_results(name, workdir, monkeypatch):
    """no table, the depth the text warrants and 6 levels (deeper than that for these texts): the same SAM, the oracle's"""
    import capi
    fa = _fasta(name, workdir)
    want = _jump_levels_for(2 * IE.TEXT_BY_NAME[name].l_pac)
    assert 0 < want < 6
    sams = {}
    for setting, levels in (("0", 0), (None, want), ("6", 6)):
        if setting is None:
            monkeypatch.delenv("PS_JUMP_LEVELS", raising=False)
        else:
            monkeypatch.setenv("PS_JUMP_LEVELS", setting)
        ctx = capi.Ctx.build(fa)
        try:
            assert ctx.info().jump_levels == levels
            c = _case(name, workdir, ctx)
            for mode in MODES:
                tag = "jump%d_%s_%s" % (levels, name, mode)
                _compare(ctx, c["oix"], _set_mode(ctx, mode), c["fq"], c["dir"], tag)
                sams[levels, mode] = sam_records(os.path.join(c["dir"], tag + ".gpu.sam"))
        finally:
            ctx.close()
    monkeypatch.delenv("PS_JUMP_LEVELS", raising=False)
    for mode in MODES:
        assert sams[0, mode] == sams[want, mode] == sams[6, mode]


def test_reference_without_a_base_is_refused(workdir):
    """headers and no base: the build fails on the host, names the file and leaves no index files"""
    import capi
    d = os.path.join(workdir, "edges_gpu_empty")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "headers_only.fa")
    with open(fa, "w") as f:
        f.write(">chrEmpty\n>chrAlsoEmpty with a description\n\n")
    with pytest.raises(capi.PsError, match="headers_only.fa"):
        capi.Ctx.build(fa)
    with pytest.raises(capi.PsError, match="headers_only.fa"):
        capi.Ctx.build(fa, save_files=True)
    with pytest.raises(capi.PsError, match="headers_only.fa"):
        capi.ps_index(fa)
    assert sorted(os.listdir(d)) == ["headers_only.fa"]
