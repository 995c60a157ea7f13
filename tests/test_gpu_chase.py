"""GPU: the chase of the search kernel (ps_narrow.h, nt_chase) against the same kernel with the chase switched off (PS_CHASE=0) and
against the oracle.  Below the jump table's levels a lane whose expansion was barren takes its match child's step in the same
iteration when that is barren too: the hits must not know, the counting kernel must see fewer iterations and the same
expansions, pushes, pops and Occ pairs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("k", "l", "n_mm", "n_gapo", "n_gape", "n_ins", "n_del", "score")
N_ORACLE = 300                                               # reads of every launch held against the oracle


@pytest.fixture(scope="module")
def ctx_mid(mid):
    import capi
    return capi.Ctx.build(mid["fa"])


def _tc_profile(t2c=0.12):
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = t2c, 1.0 - t2c - P[3, 0] - P[3, 2]
    return P


def _set_costs(ctx, costs):
    import orc
    if costs == "profile":
        P = _tc_profile()
        ctx.set_profile(P, 2.1e-5, 5.9e-4, -1)
        return orc.profile_opt(P, 2.1e-5, 5.9e-4, -1)
    ctx.set_stock("0.04")
    return orc.stock_opt("0.04")


LAUNCHES = {"fixed50": ("profile", dict(n_reads=4096, read_len=50, seed=11)),
            "ragged": ("profile", dict(n_reads=4096, read_len=75, min_len=14, seed=12)),      # 14-75 bp: both homes of the N mask, reads on either side of the seed
            "stock50": ("stock", dict(n_reads=4096, read_len=50, seed=13))}


@pytest.fixture(scope="module")
def launches(mid, workdir):
    """name -> (costs, fastq, reads, the oracle's hit lists of the first N_ORACLE reads), made once"""
    import orc
    import simulate as S
    out = {}
    for name, (costs, kw) in LAUNCHES.items():
        sim = S.simulate_reads(mid["genome"], profile=_tc_profile(), indel_scale=1.0, n_frac=0.002, **kw)
        fq = os.path.join(workdir, "chase_%s.fq" % name)
        S.write_fastq(fq, sim)
        opt = orc.profile_opt(_tc_profile(), 2.1e-5, 5.9e-4, -1) if costs == "profile" else orc.stock_opt("0.04")
        ref = []
        for r in range(N_ORACLE):
            n, hits = mid["orc_index"].aln_one(opt, sim["codes"][r, :sim["lens"][r]], cap=64)
            ref.append((n, [tuple(a[f] for f in FIELDS) for a in hits]))
        out[name] = (costs, fq, sim, ref)
    return out


def _search(ctx, fq, monkeypatch, env, stats=False):
    monkeypatch.setenv("PS_ORDER_MIN", "1")                  # the order indirection and the estimate are live in launches this small
    for k in ("PS_CHASE", "PS_SKIP", "PS_JUMP"):
        if k in env:
            monkeypatch.setenv(k, env[k])
        else:
            monkeypatch.delenv(k, raising=False)
    if stats:
        monkeypatch.setenv("PS_STATS_JUMP", "1")             # the counting kernel WITH the jump table, as the timed kernel runs
    ctx.set_stats(stats)
    try:
        b = ctx.batch_from_fastq(fq)
        b.search()
    finally:
        ctx.set_stats(False)
        for k in ("PS_CHASE", "PS_SKIP", "PS_JUMP", "PS_STATS_JUMP"):
            monkeypatch.delenv(k, raising=False)
    return b


def _same_hits(on, off, what):
    n_on, n_off = on.n_aln(), off.n_aln()
    assert np.array_equal(n_on, n_off), what
    for r in range(on.n):
        assert on.alns(r).tobytes() == off.alns(r).tobytes(), (what, r)


def _is_oracle(b, ref, what):
    n_aln = b.n_aln()
    for r, (n, hits) in enumerate(ref):
        got = [tuple(int(a[f]) for f in FIELDS) for a in b.alns(r)]
        assert n == n_aln[r] and got == hits, (what, r)


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_hits_do_not_know_about_the_chase(ctx_mid, launches, monkeypatch, name):
    costs, fq, sim, ref = launches[name]
    _set_costs(ctx_mid, costs)
    on, off = _search(ctx_mid, fq, monkeypatch, {}), _search(ctx_mid, fq, monkeypatch, {"PS_CHASE": "0"})
    _same_hits(on, off, name)
    _is_oracle(on, ref, (name, "chase"))
    _is_oracle(off, ref, (name, "PS_CHASE=0"))


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_fewer_iterations_same_work(ctx_mid, launches, monkeypatch, name):
    costs, fq, _, _ = launches[name]
    _set_costs(ctx_mid, costs)
    ks_on = _search(ctx_mid, fq, monkeypatch, {}, stats=True).kstats(1)
    ks_off = _search(ctx_mid, fq, monkeypatch, {"PS_CHASE": "0"}, stats=True).kstats(1)
    print(name, "iters with the chase %d, without %d;" % (ks_on["iters"], ks_off["iters"]),
          " ".join("%s %d / %d" % (k, ks_on[k], ks_off[k]) for k in ("nodes", "pushes", "pops", "occ_pairs", "occ_same_blk", "exact_steps")))
    for k in ("nodes", "pushes", "pops", "occ_pairs", "occ_same_blk", "exact_steps"):
        assert ks_on[k] == ks_off[k], k
    assert ks_on["iters"] < ks_off["iters"]


@pytest.mark.parametrize("env", [{"PS_SKIP": "0"}, {"PS_JUMP": "0"}], ids=["no_table_skip", "no_jump_table"])
def test_chase_without_the_table_beside_it(ctx_mid, launches, monkeypatch, env):
    """the chase with the table skip off, and with no jump table at all (every step below the root goes through the Occ array)"""
    costs, fq, _, ref = launches["fixed50"]
    _set_costs(ctx_mid, costs)
    on = _search(ctx_mid, fq, monkeypatch, dict(env, PS_CHASE="1"))
    off = _search(ctx_mid, fq, monkeypatch, dict(env, PS_CHASE="0"))
    _same_hits(on, off, env)
    _is_oracle(on, ref, env)
