"""CPU tier: the chase of the narrow search tiers (ps_narrow.h, nt_chase) on the host lane machine.  A lane whose expansion was
barren (it could only follow its match child) takes the child's step in the same iteration when that is barren too, below the jump
table's levels, where the LF step itself has to be taken: one block, the count of one symbol.  tests/hostsim is built twice, with
the chase (the default) and with -DPS_CHASE=0: hit lists, hit counts and status must be byte-identical between the two and equal
to the oracle's, the work counters (expansions, pushes, pops, Occ block pairs, exact steps) identical, and the iterations fewer."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import simulate as S

HERE = os.path.dirname(os.path.abspath(__file__))
ALNREC = np.dtype([("k", "<u8"), ("l", "<u8"), ("score", "<u2"), ("units", "<u2"), ("n_mm", "u1"), ("n_gapo", "u1"),
                   ("n_gape", "u1"), ("n_ins", "u1"), ("n_del", "u1"), ("pad", "u1", 7)])
FIELDS = ("k", "l", "n_mm", "n_gapo", "n_gape", "n_ins", "n_del", "score", "units")
KS = dict(occ_pairs=0, occ_same_blk=1, nodes=2, pushes=3, pops=4, lf_steps=5, iters=6, exact_steps=7)
SAME_WORK = ("nodes", "pushes", "pops", "occ_pairs", "occ_same_blk", "exact_steps")


def _build(workdir, name, extra):
    so = os.path.join(workdir, name)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas"] + extra +
                          ["-o", so, os.path.join(HERE, "hostsim", "hostsim.cpp")])
    H = C.CDLL(so)
    H.hs_index_new.restype = C.c_void_p
    H.hs_index_new.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
    H.hs_index_free.argtypes = [C.c_void_p]
    H.hs_sizeof_model.restype = C.c_size_t
    H.hs_model_stock.argtypes = [C.c_char_p, C.c_int, C.c_void_p]
    H.hs_model_profile.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    H.hs_aln.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7
    H.hs_set_est.argtypes = [C.c_void_p]
    H.hs_index_jump.argtypes = [C.c_void_p, C.c_int]
    return H


@pytest.fixture(scope="module")
def libs(workdir):
    """the lane machine with the chase (the default build) and without it"""
    return dict(chase=_build(workdir, "libhostsim_chase.so", []), plain=_build(workdir, "libhostsim_nochase.so", ["-DPS_CHASE=0"]))


def _sim_index(H, ix):
    bw, sa, pac = ix.bwt_syms(), ix.sa_samples(), ix.pac()
    h = H.hs_index_new(bw.ctypes.data, ix.seq_len, ix.primary, sa.ctypes.data, sa.size, 32, pac.ctypes.data, ix.l_pac)
    return h, H.hs_index_jump(h, -1)


@pytest.fixture(scope="module")
def genomes(libs, example, mid):
    """name -> (genome, oracle index, the index in either library); `mid` has ten table levels"""
    out, made = {}, []
    for name, g in (("example", example), ("mid", mid)):
        hd = {}
        for tag, H in libs.items():
            h, levels = _sim_index(H, g["orc_index"])
            made.append((H, h))
            hd[tag] = h
            if name == "mid":
                assert levels == 10
        out[name] = (g["genome"], g["orc_index"], hd)
    yield out
    for H, h in made:
        H.hs_index_free(h)


def _tc_profile(t2c=0.12):
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = t2c, 1.0 - t2c - P[3, 0] - P[3, 2]
    return P


def _model(H, costs, L, x=-1):
    model = (C.c_uint8 * H.hs_sizeof_model())()
    if costs == "profile":
        P = _tc_profile()
        Pc = np.ascontiguousarray(P.reshape(16))
        assert H.hs_model_profile(Pc.ctypes.data, 2.1e-5, 5.9e-4, x, L, model) == 0
        return model, orc.profile_opt(P, 2.1e-5, 5.9e-4, x)
    assert H.hs_model_stock(b"0.04", L, model) == 0
    return model, orc.stock_opt("0.04")


def _run(H, h, model, codes, est=None, n_lanes=64, pool_cap=65535, aln_cap=64, n_big=0):
    n, L = codes.shape
    if est is not None:
        est = np.ascontiguousarray(est, dtype=np.uint8)
        H.hs_set_est(est.ctypes.data)           # for the call below only
    alns = np.zeros((n, aln_cap), dtype=ALNREC)
    n_aln = np.zeros(n, dtype=np.int32)
    status = np.zeros(n, dtype=np.uint8)
    ks = np.zeros(8, dtype=np.uint64)
    cc = np.ascontiguousarray(codes)
    assert H.hs_aln(h, model, n, L, cc.ctypes.data, n_lanes, pool_cap, aln_cap, 0, n_big, None, None, None, alns.ctypes.data,
                    n_aln.ctypes.data, status.ctypes.data, ks.ctypes.data) == 0
    return alns, n_aln, status, ks


def _same(a, b, what):
    (a0, n0, s0, _), (a1, n1, s1, _) = a, b
    assert np.array_equal(n0, n1) and np.array_equal(s0, s1), what
    for r in range(n0.size):
        assert a0[r, :min(n0[r], a0.shape[1])].tobytes() == a1[r, :min(n1[r], a1.shape[1])].tobytes(), (what, r)


def _is_oracle(ix, opt, codes, res, what):
    for r in range(codes.shape[0]):
        n, ref = ix.aln_one(opt, codes[r], cap=64)
        assert res[2][r] == 0, (what, r)
        got = [tuple(int(a[f]) for f in FIELDS) for a in res[0][r, :res[1][r]]]
        assert n == res[1][r] and got == [tuple(a[f] for f in FIELDS) for a in ref], (what, r)


def _same_work(chase, plain, what, chased=False):
    for k in SAME_WORK:
        assert int(chase[3][KS[k]]) == int(plain[3][KS[k]]), (what, k)
    it1, it0 = int(chase[3][KS["iters"]]), int(plain[3][KS["iters"]])
    assert it1 <= it0, what
    if chased:
        assert it1 < it0, (what, "the case did not chase")


def _best(base):
    return np.where(base[1] > 0, base[0]["units"][:, 0], 255).astype(np.int64)


def _reads(genome, n, L, seed, n_frac=0.002):
    return S.simulate_reads(genome, n, L, seed=seed, profile=_tc_profile(), indel_scale=1.0, n_frac=n_frac)["codes"]


@pytest.mark.parametrize("L", [14, 20, 50, 75])
@pytest.mark.parametrize("costs", ["profile", "stock"])
@pytest.mark.parametrize("gname", ["example", "mid"])
def test_chase_changes_nothing_but_the_iterations(libs, genomes, gname, costs, L):
    """with the chase and without it: the same hits (and the oracle's), the same expansions, pushes, pops, Occ block pairs and
    exact steps -- without estimates of the best score, with exact ones, and with estimates eight units too low (the restart path)"""
    genome, ix, hd = genomes[gname]
    codes = _reads(genome, 160, L, seed=100 + L)
    assert (codes == 4).any()
    model, opt = _model(libs["chase"], costs, L)
    base = _run(libs["plain"], hd["plain"], model, codes)
    _is_oracle(ix, opt, codes, base, "plain")
    best = _best(base)
    for tag, est in (("none", None), ("exact", best), ("low", np.maximum(best - 8, 0))):
        plain = _run(libs["plain"], hd["plain"], model, codes, est=est)
        chase = _run(libs["chase"], hd["chase"], model, codes, est=est)
        _same(base, plain, (tag, "plain"))
        _same(base, chase, (tag, "chase"))
        _same_work(chase, plain, tag)


def test_chase_takes_effect(libs, genomes):
    """8 Mbp (ten table levels), 1,000 reads of 50 bp, profile costs, exact estimates: the iterations with the chase are at most 0.85
    of those without.  (Counted on 3,000 such reads: one chase step with every Occ pair taken leaves 0.774; the margin is for the
    children whose rows lie in two blocks, about 5 % of the pairs, and the excluded cases.)"""
    genome, ix, hd = genomes["mid"]
    codes = S.simulate_reads(genome, 1000, 50, seed=11, profile=_tc_profile(), indel_scale=1.0)["codes"]
    model, _ = _model(libs["chase"], "profile", 50)
    base = _run(libs["plain"], hd["plain"], model, codes)
    best = _best(base)
    plain = _run(libs["plain"], hd["plain"], model, codes, est=best)
    chase = _run(libs["chase"], hd["chase"], model, codes, est=best)
    _same(plain, chase, "exact estimates")
    _same_work(chase, plain, "exact estimates")
    it0, it1 = int(plain[3][KS["iters"]]), int(chase[3][KS["iters"]])
    print("iters without the chase %d, with it %d: ratio %.4f" % (it0, it1, it1 / it0))
    assert it1 <= 0.85 * it0, (it0, it1)


def _edge(libs, genomes, codes, L, what, gname="mid", costs="profile", x=-1, est="exact", oracle=True, **kw):
    """one edge: it chased (fewer iterations), the hits and the work are the same, and the plain build's hits are the oracle's"""
    genome, ix, hd = genomes[gname]
    model, opt = _model(libs["chase"], costs, L, x)
    base = _run(libs["plain"], hd["plain"], model, codes)
    if oracle:
        _is_oracle(ix, opt, codes, base, what)
    e = _best(base) if est == "exact" else None
    plain = _run(libs["plain"], hd["plain"], model, codes, est=e, **kw)
    chase = _run(libs["chase"], hd["chase"], model, codes, est=e, **kw)
    _same_work(chase, plain, what, chased=True)
    _same(plain, chase, what)
    return plain, chase


def _exact_reads(genome, n, L, seed):
    """n substrings of the forward strand, as codes, with T>C conversions and nothing else: reads with a few cheap differences"""
    return S.simulate_reads(genome, n, L, seed=seed, profile=_tc_profile(0.3), indel_scale=0.0)["codes"]


def test_edge_run_reaches_position_one(libs, genomes):
    """the base consumed last is an N, so D(0) = 1: the positions down to 1 are barren once one difference is left, and a chase
    lands on the entry at position 1 (whose child, at position 0, is the hit -- never chased)"""
    codes = _exact_reads(genomes["mid"][0], 96, 50, seed=501).copy()
    codes[:, -1] = 4
    _edge(libs, genomes, codes, 50, "N at the last base")
    codes = _exact_reads(genomes["mid"][0], 96, 50, seed=502).copy()
    codes[:, -2] = 4
    _edge(libs, genomes, codes, 50, "N at the last base but one")


@pytest.mark.parametrize("L", [20, 32])
def test_edge_read_no_longer_than_the_seed(libs, genomes, L):
    """such a read has no seed rule of its own: only the read's bounds make a step barren"""
    codes = _reads(genomes["mid"][0], 128, L, seed=510 + L)
    _edge(libs, genomes, codes, L, "read of %d bp" % L)


def test_edge_n_inside_a_run(libs, genomes):
    """one read base in fifty is an N: runs end on it, and the entry is left to the normal step"""
    codes = _reads(genomes["mid"][0], 128, 50, seed=520, n_frac=0.02)
    assert ((codes == 4).sum(axis=1) > 0).sum() > 40
    _edge(libs, genomes, codes, 50, "N in the read")


def test_edge_largest_budget(libs, genomes):
    """-X 15, the largest budget the narrow tiers pack (the chase compares bounds as integers, not as bytes: nothing to overflow)"""
    codes = _reads(genomes["example"][0], 48, 50, seed=530)
    _edge(libs, genomes, codes, 50, "-X 15", gname="example", x=15)


def test_edge_one_lane(libs, genomes):
    """a one-lane machine (the general 64-bit bucket bitmap), with the hit service as the odd lanes have it"""
    codes = _reads(genomes["mid"][0], 48, 50, seed=540)
    _edge(libs, genomes, codes, 50, "one lane", n_lanes=1)


def test_edge_move_to_a_large_slot(libs, genomes):
    """a private stack of 24 entries: reads move to a large slot in mid-run, and the expansion that asked for it is redone there"""
    codes = _reads(genomes["mid"][0], 64, 50, seed=550)
    plain, chase = _edge(libs, genomes, codes, 50, "pool_cap 24", est=None, oracle=False, pool_cap=24, n_big=64, n_lanes=16)      # a slot for every read (the lane machine never hands one back)
    assert (plain[2] == 0).all() and int(plain[3][KS["pushes"]]) > 64 * 24
    roomy = _run(libs["chase"], genomes["mid"][2]["chase"], _model(libs["chase"], "profile", 50)[0], codes)
    _same(roomy, chase, "against a stack that never fills")


def test_blk_count1_is_an_entry_of_blk_count4b(workdir):
    """the count of one symbol (ps_core.h's blk_count1 and the chase's blk_count1b) against the four-symbol count, every r in 0..192"""
    so = os.path.join(workdir, "libchase_blk_counts.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(HERE, "chase_blk_counts.cpp")])
    H = C.CDLL(so)
    H.cb_blk_counts.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(7)
    blocks = [rng.integers(0, 2 ** 32, 16, dtype=np.uint64).astype(np.uint32) for _ in range(6)]
    blocks.append(np.zeros(16, dtype=np.uint32))
    blocks.append(np.full(16, 0xFFFFFFFF, dtype=np.uint32))
    for b in blocks:
        b[:4] &= 0x7FFFFFFF                      # running counts: room for 192 more
        b = np.ascontiguousarray(b)
        for r in range(193):
            o4, o1, o1b = (np.zeros(4, dtype=np.uint32) for _ in range(3))
            H.cb_blk_counts(b.ctypes.data, r, o4.ctypes.data, o1.ctypes.data, o1b.ctypes.data)
            assert np.array_equal(o4, o1) and np.array_equal(o4, o1b), (r, o4, o1, o1b)
            assert int(o4.sum()) == int(b[:4].sum()) + r
