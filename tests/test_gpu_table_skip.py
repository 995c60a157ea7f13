"""GPU: the table skip of the search kernel (ps_narrow.h, nt_skip) against the same kernel with the skip switched off (PS_SKIP=0)
and against the oracle.  An entry inside the jump table's levels crosses the barren steps in front of it in one iteration: the
hits must not know, the counting kernel must see fewer iterations and the same pushes and pops."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("k", "l", "n_mm", "n_gapo", "n_gape", "n_ins", "n_del", "score")


@pytest.fixture(scope="module")
def ctx_mid(mid):
    import capi
    return capi.Ctx.build(mid["fa"])


def _tc_profile(t2c=0.12):
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = t2c, 1.0 - t2c - P[3, 0] - P[3, 2]
    return P


@pytest.fixture(scope="module")
def launches(mid, workdir):
    """the two launches: 4,096 PAR-CLIP reads of 50 bp, and 2,048 ragged reads of 8-36 bp (some end inside the table's levels)"""
    import simulate as S
    out = {}
    for name, kw in (("fixed50", dict(n_reads=4096, read_len=50, seed=11)), ("ragged", dict(n_reads=2048, read_len=36, min_len=8, seed=12))):
        sim = S.simulate_reads(mid["genome"], profile=_tc_profile(), indel_scale=1.0, n_frac=0.002, **kw)
        fq = os.path.join(workdir, "skip_%s.fq" % name)
        S.write_fastq(fq, sim)
        out[name] = (fq, sim)
    return out


def _search(ctx, fq, monkeypatch, skip, stats=False):
    monkeypatch.setenv("PS_ORDER_MIN", "1")                  # the order indirection and the estimate are live in launches this small
    if skip:
        monkeypatch.delenv("PS_SKIP", raising=False)
    else:
        monkeypatch.setenv("PS_SKIP", "0")
    if stats:
        monkeypatch.setenv("PS_STATS_JUMP", "1")             # the counting kernel WITH the jump table: without one there is nothing to skip
    ctx.set_stats(stats)
    try:
        b = ctx.batch_from_fastq(fq)
        b.search()
    finally:
        ctx.set_stats(False)
        monkeypatch.delenv("PS_STATS_JUMP", raising=False)
    return b


@pytest.mark.parametrize("name", ["fixed50", "ragged"])
def test_hits_do_not_know_about_the_skip(ctx_mid, mid, launches, monkeypatch, name):
    import orc
    fq, sim = launches[name]
    P = _tc_profile()
    ctx_mid.set_profile(P, 2.1e-5, 5.9e-4, -1)
    opt = orc.profile_opt(P, 2.1e-5, 5.9e-4, -1)
    on, off = _search(ctx_mid, fq, monkeypatch, True), _search(ctx_mid, fq, monkeypatch, False)
    n_on, n_off = on.n_aln(), off.n_aln()
    assert np.array_equal(n_on, n_off)
    for r in range(on.n):
        assert on.alns(r).tobytes() == off.alns(r).tobytes(), r
    oix = mid["orc_index"]
    for r in range(500):                                      # the oracle, on a sample
        n, ref = oix.aln_one(opt, sim["codes"][r, :sim["lens"][r]], cap=64)
        got = [tuple(int(a[f]) for f in FIELDS) for a in on.alns(r)]
        assert n == n_on[r] and got == [tuple(a[f] for f in FIELDS) for a in ref], r
    if name == "ragged":
        assert (sim["lens"] < 10).any() and n_on[sim["lens"] < 10].max() > 0      # hits inside the table's levels (ten on this genome)


@pytest.mark.parametrize("name", ["fixed50", "ragged"])
def test_fewer_iterations_same_pushes_and_pops(ctx_mid, launches, monkeypatch, name):
    fq, _ = launches[name]
    ctx_mid.set_profile(_tc_profile(), 2.1e-5, 5.9e-4, -1)
    ks_on = _search(ctx_mid, fq, monkeypatch, True, stats=True).kstats(1)
    ks_off = _search(ctx_mid, fq, monkeypatch, False, stats=True).kstats(1)
    print(name, "iters with the skip %d, without %d; pushes %d / %d, pops %d / %d" %
          (ks_on["iters"], ks_off["iters"], ks_on["pushes"], ks_off["pushes"], ks_on["pops"], ks_off["pops"]))
    assert ks_on["pushes"] == ks_off["pushes"] and ks_on["pops"] == ks_off["pops"]
    assert ks_on["iters"] < ks_off["iters"]
