"""CPU tier: the table skip of the narrow search tiers (ps_narrow.h, nt_skip) on the host lane machine.  An entry inside the jump
table's levels crosses the run of barren steps in front of it -- steps that can only follow the match child -- in one iteration.
tests/hostsim is built twice, with the skip (the default) and with -DPS_TABLE_SKIP=0: hit lists, hit counts and status must be
byte-identical between the two and equal to the oracle's, the work counters that the skip has no business with (pushes, pops,
Occ block pairs) identical, and the iterations fewer."""
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
    """the lane machine with the skip (the default build) and without it"""
    return dict(skip=_build(workdir, "libhostsim_skip.so", []), plain=_build(workdir, "libhostsim_noskip.so", ["-DPS_TABLE_SKIP=0"]))


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


def _model(H, costs, L):
    model = (C.c_uint8 * H.hs_sizeof_model())()
    if costs == "profile":
        P = _tc_profile()
        Pc = np.ascontiguousarray(P.reshape(16))
        assert H.hs_model_profile(Pc.ctypes.data, 2.1e-5, 5.9e-4, -1, L, model) == 0
        return model, orc.profile_opt(P, 2.1e-5, 5.9e-4, -1)
    assert H.hs_model_stock(b"0.04", L, model) == 0
    return model, orc.stock_opt("0.04")


def _run(H, h, model, codes, est=None, n_lanes=64, pool_cap=65535, aln_cap=64):
    n, L = codes.shape
    if est is not None:
        est = np.ascontiguousarray(est, dtype=np.uint8)
        H.hs_set_est(est.ctypes.data)           # for the call below only
    alns = np.zeros((n, aln_cap), dtype=ALNREC)
    n_aln = np.zeros(n, dtype=np.int32)
    status = np.zeros(n, dtype=np.uint8)
    ks = np.zeros(8, dtype=np.uint64)
    cc = np.ascontiguousarray(codes)
    assert H.hs_aln(h, model, n, L, cc.ctypes.data, n_lanes, pool_cap, aln_cap, 0, 0, None, None, None, alns.ctypes.data,
                    n_aln.ctypes.data, status.ctypes.data, ks.ctypes.data) == 0
    return alns, n_aln, status, ks


def _same(a, b, what):
    (a0, n0, s0, _), (a1, n1, s1, _) = a, b
    assert np.array_equal(n0, n1) and np.array_equal(s0, s1), what
    for r in range(n0.size):
        assert a0[r, :min(n0[r], a0.shape[1])].tobytes() == a1[r, :min(n1[r], a1.shape[1])].tobytes(), (what, r)


def _reads(genome, n, L, seed):
    return S.simulate_reads(genome, n, L, seed=seed, profile=_tc_profile(), indel_scale=1.0, n_frac=0.002)["codes"]


@pytest.mark.parametrize("L", [14, 20, 50, 75])
@pytest.mark.parametrize("costs", ["profile", "stock"])
@pytest.mark.parametrize("gname", ["example", "mid"])
def test_skip_changes_nothing_but_the_iterations(libs, genomes, gname, costs, L):
    """with the skip and without it: the same hits (and the oracle's), the same pushes, pops and Occ block pairs -- with exact
    estimates of the best score and with estimates eight units too low (the restart path)"""
    genome, ix, hd = genomes[gname]
    codes = _reads(genome, 160, L, seed=100 + L)
    model, opt = _model(libs["skip"], costs, L)
    base = _run(libs["plain"], hd["plain"], model, codes)
    for r in range(codes.shape[0]):                      # the oracle
        n, ref = ix.aln_one(opt, codes[r], cap=64)
        assert base[2][r] == 0
        got = [tuple(int(a[f]) for f in FIELDS) for a in base[0][r, :base[1][r]]]
        assert n == base[1][r] and got == [tuple(a[f] for f in FIELDS) for a in ref], r
    best = np.where(base[1] > 0, base[0]["units"][:, 0], 255).astype(np.int64)
    for tag, est in (("none", None), ("exact", best), ("low", np.maximum(best - 8, 0))):
        plain = _run(libs["plain"], hd["plain"], model, codes, est=est)
        skip = _run(libs["skip"], hd["skip"], model, codes, est=est)
        _same(base, plain, (tag, "plain"))
        _same(base, skip, (tag, "skip"))
        for k in ("pushes", "pops", "occ_pairs", "occ_same_blk"):
            assert int(skip[3][KS[k]]) == int(plain[3][KS[k]]), (tag, k)
        assert int(skip[3][KS["iters"]]) <= int(plain[3][KS["iters"]]), tag


def test_skip_saves_a_tenth_of_the_iterations(libs, genomes):
    """8 Mbp (ten table levels), 50 bp, profile costs, exact estimates: the iterations with the skip are at most 0.90 of those
    without.  (A prototype that absorbed every barren run measured 0.833 on 3,000 such reads; above 0.90 the skip is not taking effect.)"""
    genome, ix, hd = genomes["mid"]
    codes = S.simulate_reads(genome, 1000, 50, seed=11, profile=_tc_profile(), indel_scale=1.0)["codes"]
    model, _ = _model(libs["skip"], "profile", 50)
    base = _run(libs["plain"], hd["plain"], model, codes)
    best = np.where(base[1] > 0, base[0]["units"][:, 0], 255).astype(np.int64)
    plain = _run(libs["plain"], hd["plain"], model, codes, est=best)
    skip = _run(libs["skip"], hd["skip"], model, codes, est=best)
    _same(plain, skip, "exact estimates")
    it0, it1 = int(plain[3][KS["iters"]]), int(skip[3][KS["iters"]])
    print("iters without the skip %d, with it %d: ratio %.4f" % (it0, it1, it1 / it0))
    for k in ("pushes", "pops", "occ_pairs", "occ_same_blk"):
        assert int(skip[3][KS[k]]) == int(plain[3][KS[k]]), k
    assert it1 <= 0.90 * it0, (it0, it1)
