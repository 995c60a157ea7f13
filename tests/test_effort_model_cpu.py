"""CPU: known answers for the plain restatements of tests/effort_model.py (the references test_gpu_launch_order.py holds the
width, effort and model kernels against), on a random 20 kb text: at that size no 20-mer occurs twice, on either strand."""
import os

import numpy as np
import pytest

import effort_model as E

TEXT_BP = 20000
W_PIN = 16


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    import orc
    import simulate as S
    rng = np.random.default_rng(0x20B)
    codes = rng.integers(0, 4, size=TEXT_BP).astype(np.uint8)
    fa = os.path.join(str(tmp_path_factory.mktemp("effort")), "text.fa")
    S.write_fasta(fa, [("t", S.BASES[codes])])
    oix = orc.Index.from_fasta(fa)
    return dict(codes=codes, oix=oix, fm=E.fm_of(oix))


def _profile_opt():
    import orc
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 1.0 - 0.12 - P[3, 0] - P[3, 2]
    return orc.profile_opt(P, 2.1e-5, 5.9e-4, 2)


def _stock_opt():
    import orc
    return orc.stock_opt("2")


def _copies(text, n=12, length=50, seed=5):
    """(start, strand, codes): reads copied from the text, every other one from the other strand"""
    import simulate as S
    rng = np.random.default_rng(seed)
    out = []
    for q in range(n):
        a = int(rng.integers(0, TEXT_BP - length))
        fwd = text["codes"][a:a + length]
        out.append((a, q & 1, S.COMP[fwd[::-1]] if q & 1 else fwd.copy()))
    return out


def test_prefix_counts_are_the_oracles_occ(text):
    fm = text["fm"]
    assert fm.seq_len == 2 * TEXT_BP                            # both strands
    assert E.check_prefix_counts(text["oix"], fm) > 40


def test_no_20mer_twice(text):
    """what the known answers below rest on"""
    import simulate as S
    both = np.concatenate([text["codes"], S.COMP[text["codes"][::-1]]]).astype(np.uint64)
    h = np.zeros(both.size - 19, dtype=np.uint64)
    for j in range(20):
        h = h * np.uint64(4) + both[j:j + h.size]
    ok = np.ones(h.size, dtype=bool)
    ok[TEXT_BP - 19:TEXT_BP] = False                            # windows across the seam of the two strands are no text
    assert np.unique(h[ok]).size == int(ok.sum())


@pytest.mark.parametrize("costs", ["stock", "profile"])
def test_a_copy_costs_nothing(text, costs):
    m = E.launch_model(_stock_opt() if costs == "stock" else _profile_opt(), 50)
    for _, strand, read in _copies(text):
        assert E.effort_scans(text["oix"], read, m["u_mm"], E.average_mismatch(m["u_mm"]), W_PIN) == (0, 0, 0, 0, 0), strand


@pytest.mark.parametrize("costs", ["stock", "profile"])
def test_one_substitution_costs_its_unit_cost(text, costs):
    opt = _stock_opt() if costs == "stock" else _profile_opt()
    m = E.launch_model(opt, 50)
    rng = np.random.default_rng(9)
    seen = set()
    for a, strand, read in _copies(text, n=48):
        p = int(rng.integers(20, 50 - 20))
        true, new = int(read[p]), int((read[p] + 1 + rng.integers(0, 3)) % 4)
        read[p] = new
        want = int(opt.sub_cost[true * 4 + new]) if costs == "profile" else 1     # the table is in read orientation: [true base * 4 + read base]
        seen.add(want)
        ta, ra, tb, rb, est = E.effort_scans(text["oix"], read, m["u_mm"], E.average_mismatch(m["u_mm"]), W_PIN)
        assert (ta, ra, tb, rb, est) == (want, 0, want, 0, want), (a, strand, p, true, new)
    assert costs == "stock" or len(seen) > 3                   # the cheap conversion and dear substitutions were both drawn


@pytest.mark.parametrize("costs,c_restart", [("stock", 1), ("profile", 8), ("profile", 3)])
def test_all_n_restarts_at_every_base(text, costs, c_restart):
    m = E.launch_model(_stock_opt() if costs == "stock" else _profile_opt(), 37)
    read = np.full(37, 4, dtype=np.uint8)
    assert E.effort_scans(text["oix"], read, m["u_mm"], c_restart, W_PIN) == (37 * c_restart, 37, 37 * c_restart, 37, 37 * c_restart)
    assert E.pack_est_ab(37 * 8, 37, 5, 0) == (127 | 0x80) | (5 << 8)


def test_average_mismatch_of_the_stock_model_is_one(text):
    assert E.average_mismatch(E.launch_model(_stock_opt(), 50)["u_mm"]) == 1
    assert E.average_mismatch(E.launch_model(_profile_opt(), 50)["u_mm"]) == 8      # the profile's unit IS its average mismatch


def test_bounds_are_the_oracles(text):
    """width_bounds' bid against the widths aln_one itself searched with, read and seed chain; the equal-width flag from its w"""
    opt = _stock_opt()
    rng = np.random.default_rng(3)
    for a, strand, read in _copies(text, n=10, length=50) + _copies(text, n=4, length=33) + _copies(text, n=4, length=32):
        for p in rng.integers(0, read.size, size=int(rng.integers(0, 4))):
            read[p] = (read[p] + 1) % 4
        if a % 3 == 0:
            read[int(rng.integers(0, read.size))] = 4
        _, _, w, sw = text["oix"].aln_one(opt, read, want_width=True)
        chain, seed = E.width_bounds(text["oix"], read, opt.seed_len)
        assert [b for b, _ in chain] == [b for _, b in w]
        assert [e for _, e in chain] == [i > 0 and w[i][0] == w[i - 1][0] for i in range(len(w))]
        assert chain[-1] == (chain[-2][0] + 1, False) and not chain[0][1]
        if read.size > opt.seed_len:
            assert [b for b, _ in seed] == [b for _, b in sw]
        else:
            assert seed is None
        words = E.pack_bounds(chain, 64)
        assert words.size == 16 and int(words[0]) & 0xff == chain[0][0] and int(words[(read.size) >> 2] >> (8 * (read.size & 3))) & 0x7f == chain[-1][0]


def test_no_budget_counts_the_levels_the_exact_path_lives(text):
    """with a budget of 0 units only the exact path exists: one node per level while the bound lets it live and the read has a base"""
    m = E.launch_model(_stock_opt(), 50)
    rows = 4 ** 64                                             # every string occurs: no thinning
    _, _, read = _copies(text, n=1)[0]
    D = np.zeros(51, dtype=np.int64)
    assert E.expected_nodes(read, D, 0, m, rows, 13) == 50.0   # 13 levels walked, the 37 behind them by the one survivor
    assert E.expected_nodes(read, D, 0, m, rows, 64) == 50.0
    for p in (0, 1, 7, 12):                                    # an N: the node at its level is the last
        r = read.copy()
        r[p] = 4
        assert E.expected_nodes(r, D, 0, m, rows, 13) == p + 1.0
    for dead_from in (0, 3, 12):                               # a bound no budget pays for, at the level that reads it: nothing from there on
        Dd = D.copy()
        Dd[50 - 1 - dead_from] = 1
        assert E.expected_nodes(read, Dd, 0, m, rows, 13) == float(dead_from)
    # thinning: a level's survivor is worth the chance that its string occurs at all
    assert E.expected_nodes(read[:3], np.zeros(4, dtype=np.int64), 0, m, 8, 13) == 1.0 + 1.0 + 0.5


def test_one_unit_opens_the_children_by_the_table(text):
    """stock costs, one unit, no bounds, no thinning, away from the ends' gap rule: the root has three mismatch children, four
    deletions and an insertion, each of which lives on as an exact path"""
    m = E.launch_model(_stock_opt(), 50)
    rows = 4 ** 64
    _, _, read = _copies(text, n=1)[0]
    D = np.zeros(51, dtype=np.int64)
    skip = m["indel_end_skip"]
    want, alive0, alive1 = 0.0, 1.0, 0.0
    for d in range(50):
        i = 49 - d
        want += alive0 + alive1
        gap = 5.0 if (i >= skip and 50 - i >= skip) else 0.0
        alive1 += alive0 * (3.0 + gap)
    m1 = dict(m, use_seed=False, seed_len=0)
    assert E.expected_nodes(read, D, 1, m1, rows, 64) == want
    assert E.model_depth(2 * 483300) == 13 and E.model_depth(4 ** 5) == 9 and E.model_depth(4 ** 5 - 1) == 8
    assert E.order_key(0.0, 8) == 255 and E.order_key(1.0, 8) == 247 and E.order_key(2.0 ** 40, 8) == 0


@pytest.mark.parametrize("costs,c_restart,w_pin", [("stock", 1, 16), ("profile", 8, 16), ("profile", 3, 1), ("stock", 1, 2)])
def test_all_reads_at_once_is_read_by_read(text, costs, c_restart, w_pin):
    """effort_scans_many (what the GPU tests use for thousands of reads) against the plain scan, read by read: copies with 0-5
    substitutions, some in a cluster, N, random reads, lengths 1-60"""
    m = E.launch_model(_stock_opt() if costs == "stock" else _profile_opt(), 50)
    rng = np.random.default_rng(17)
    lens = rng.integers(1, 61, size=120)
    codes = np.full((120, 60), 255, dtype=np.uint8)
    for r, (a, _, read) in enumerate(_copies(text, n=120, length=60, seed=23)):
        for p in rng.integers(0, 60, size=int(rng.integers(0, 6))):
            read[p] = (read[p] + 1 + rng.integers(0, 3)) % 4
        if r % 5 == 0:
            q = int(rng.integers(0, 56))
            read[q:q + 4] = (read[q:q + 4] + 1) % 4             # a cluster
        if r % 7 == 0:
            read[rng.integers(0, 60, size=2)] = 4
        if r % 11 == 0:
            read[:] = rng.integers(0, 4, size=60)
        codes[r, :lens[r]] = read[:lens[r]]
    many = E.effort_scans_many(text["oix"], codes, lens, m["u_mm"], c_restart, w_pin)
    restarted = 0
    for r in range(120):
        one = E.effort_scans(text["oix"], codes[r, :lens[r]], m["u_mm"], c_restart, w_pin)
        assert one == tuple(int(x[r]) for x in many), r
        restarted += one[1] > 0
    assert 10 < restarted < 110
