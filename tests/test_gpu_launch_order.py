"""GPU: what a search launch is prepared with, held by VALUE against plain restatements (tests/effort_model.py) -- the width
stage's D(i) bounds (k_width), the effort estimate (k_effort), the expected-nodes model and its class (k_effort_model<16|32|64>,
k_order_keys) and the hand-out order (the order sort).  Parity cannot see any of them: a bound that is too small prunes less and
finds the same hits, and the estimate, the model and the order decide only when a read is searched.

The launch's arrays come through the profiling seam (PS_READ_ITERS=1): ps_ctx_read_iters (bounds as the search fetched them, the
two scans' totals) and ps_ctx_launch_order (est, key, pred, order, ids), all by the bin's read index; `ids` maps that to the
input read.  Every launch here is one search launch of one bin with no read sent to a larger tier."""
import math
import os

import numpy as np
import pytest

import effort_model as E

pytestmark = pytest.mark.gpu

SCALE = 8                     # PS_ORDER_SCALE's default: classes per doubling of the expected node count
W_PIN = 16                    # PS_ORDER_WPIN's default
LOG2_ULPS = 4.0 * 2.0 ** -24  # the fast log2 (v_log_f32: 1 ulp), the rounding of tot + 1 and of the product with the scale, half an ulp each


def _tc_profile(t2c=0.12):
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = t2c, 1.0 - t2c - P[3, 0] - P[3, 2]
    return P


def _set_costs(ctx, costs):
    """the library's costs and the oracle's option struct of the same"""
    import orc
    kind, arg = costs.split("_")
    if kind == "stock":
        ctx.set_stock(arg[1:])
        return orc.stock_opt(arg[1:])
    ctx.set_profile(_tc_profile(), 2.1e-5, 5.9e-4, int(arg[1:]))
    return orc.profile_opt(_tc_profile(), 2.1e-5, 5.9e-4, int(arg[1:]))


@pytest.fixture(scope="module")
def ctx(example):
    import capi
    before = os.environ.get("PS_READ_ITERS")
    os.environ["PS_READ_ITERS"] = "1"                           # read when the context is made
    try:
        c = capi.Ctx.build(example["fa"])
    finally:
        if before is None:
            del os.environ["PS_READ_ITERS"]
        else:
            os.environ["PS_READ_ITERS"] = before
    yield c
    c.close()


@pytest.fixture(scope="module")
def gcodes(example):
    import simulate as S
    E.check_prefix_counts(example["orc_index"], E.fm_of(example["orc_index"]))
    return S.contig_codes(example["genome"][0][1])


# ---- reads -----------------------------------------------------------------------------------------------------------------
def _substrings(gc, n, length, rng):
    """n windows of the genome without an N, every other one (at random) from the other strand"""
    import simulate as S
    cs = np.concatenate([[0], np.cumsum(gc == 4)])
    start, todo = np.zeros(n, dtype=np.int64), np.arange(n)
    while todo.size:
        s = rng.integers(0, gc.size - length, size=todo.size)
        ok = cs[s + length] == cs[s]
        start[todo[ok]] = s[ok]
        todo = todo[~ok]
    reads = gc[start[:, None] + np.arange(length)[None, :]]
    rev = rng.random(n) < 0.5
    reads[rev] = S.COMP[reads[rev][:, ::-1]]
    return reads


def _substitute(reads, n_sub, rng, lo=0, hi=None):
    """n_sub[r] substitutions into read r at random positions of [lo, hi)"""
    hi = reads.shape[1] if hi is None else hi
    for j in range(int(np.max(n_sub, initial=0))):
        rows = np.nonzero(np.asarray(n_sub) > j)[0]
        p = rng.integers(lo, hi, size=rows.size)
        reads[rows, p] = (reads[rows, p] + rng.integers(1, 4, size=rows.size)) % 4
    return reads


def _mixed_pool(gc, n, length, rng, heavy=True):
    """reads by class r % 10 -- 0, 1: copies; 2..5: one to four substitutions (heavy; else one or two); 6: a 1-base insertion;
    7: a 1-base deletion (heavy; else copies); 8: one or two N; 9: a substitution and an N -- on both strands"""
    wide = _substrings(gc, n, length + 1, rng)
    reads = wide[:, :length].copy()
    cls = np.arange(n) % 10
    n_sub = np.select([cls == 2, cls == 3, cls == 4, cls == 5, cls == 9], [1, 2, 3 if heavy else 1, 4 if heavy else 2, 1], 0)
    _substitute(reads, n_sub, rng)
    if heavy:
        for r in np.nonzero(cls == 6)[0]:
            p = int(rng.integers(10, length - 10))
            reads[r] = np.concatenate([reads[r, :p], [(reads[r, p] + 1) % 4], reads[r, p:length - 1]])
        for r in np.nonzero(cls == 7)[0]:
            p = int(rng.integers(10, length - 10))
            reads[r] = np.concatenate([wide[r, :p], wide[r, p + 1:length + 1]])
    for r in np.nonzero(cls >= 8)[0]:
        reads[r, rng.integers(0, length, size=2 if (cls[r] == 8 and r % 20 >= 10) else 1)] = 4
    return reads


# ---- a launch and what it was prepared with ------------------------------------------------------------------------------------
def _launch(ctx, monkeypatch, codes=None, fq=None, env=()):
    """one search launch -> (the per-read profile [n, 20], the launch's order arrays); holds (d): order is the stable sort of key"""
    monkeypatch.setenv("PS_ORDER_MIN", "1")
    for k in ("PS_ORDER", "PS_ORDER_WPIN", "PS_ORDER_RESTART", "PS_ORDER_CAP", "PS_ORDER_SCALE", "PS_KEEP_ORDER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env).items():
        monkeypatch.setenv(k, v)
    b = ctx.batch_from_codes(codes) if fq is None else ctx.batch_from_fastq(fq)
    b.search()
    tm = b.timing()
    assert tm["n_backtrack_launches"] == 1 and tm["n_overflow_tier1"] == 0
    ri, lo = ctx.read_iters().reshape(-1, ctx.RI_WORDS), ctx.launch_order()
    n = b.n
    b.free()
    assert ri.shape[0] == n and all(lo[k].size == n for k in ("est", "key", "pred", "order", "ids"))
    assert np.array_equal(np.sort(lo["ids"]), np.arange(n))
    assert np.array_equal(lo["order"], np.argsort(lo["key"], kind="stable"))
    return ri, lo


def _rows(n, clamps=()):
    """the reads of a launch that are looked at: all of a small one; of a large one every read at or past a kernel's block clamp
    (the second trip of its grid-stride loop), the 64 before it, and every 257th"""
    if n <= 2000:
        return np.arange(n)
    pick = set(range(0, n, 257))
    for c in clamps:
        if c < n:
            pick.update(range(c - 64, min(n, c + 37)))
    return np.array(sorted(pick))


CLAMPS = (8192, 16384, 32768, 262144, 524288)      # k_effort_model<64 | 32 | 16>, k_effort, k_width: reads per trip at the block clamp of 2,048


def _check_bounds(oix, opt, ri, lo, codes, lens, rows):
    """(a) words 4..19: the packed bytes of chain steps 0..len (the first 64), bit 7 the equal-width flag; word 2: D(read) | D(seed) << 8"""
    launch_seed = opt.seed_len if int(lens.max()) > opt.seed_len else 0
    for r in rows:
        g = lo["ids"][r]
        n = int(lens[g])
        chain, seed = E.width_bounds(oix, codes[g, :n], launch_seed)
        assert np.array_equal(ri[r, 4:20], E.pack_bounds(chain, 64)), (r, g, n)
        want = min(chain[n - 1][0], 127) | ((min(seed[launch_seed - 1][0], 127) if seed else 0) << 8)
        assert int(ri[r, 2]) & 0xffff == want, (r, g, n)


def _check_estimate(oix, opt, ri, lo, codes, lens, rows, c_restart=None, w_pin=W_PIN):
    """(b) the two scans' totals and restart flags (word 2, << 16 and << 24) and the estimate; returns the reference's estimate"""
    m = E.launch_model(opt, int(lens.max()))
    g = lo["ids"][rows]
    ta, ra, tb, rb, est = E.effort_scans_many(oix, codes[g], lens[g], m["u_mm"], E.average_mismatch(m["u_mm"]) if c_restart is None else c_restart, w_pin)
    assert max(int(ta.max()), int(tb.max())) < 127             # on the reference: the 7-bit fields hold every total
    want = (ta | ((ra > 0) << 7)) | ((tb | ((rb > 0) << 7)) << 8)
    bad = np.nonzero(((ri[rows, 2] >> 16) != want) | (lo["est"][rows] != est))[0]
    assert bad.size == 0, [(int(rows[q]), int(g[q]), hex(int(ri[rows[q], 2]) >> 16), hex(int(want[q])), int(lo["est"][rows[q]]), int(est[q])) for q in bad[:8]]
    return est


def _check_model(oix, opt, lo, codes, lens, rows, est):
    """(c) pred against the float64 recurrence, key against the class of the float64 value.

    The tolerance.  Every term of the recurrence is non-negative, so float32 sums lose no more than their roundings: a value that
    went through k roundings is within (1 + 2^-24)^k of exact, relative.  A level puts a state's value through at most 8 -- the
    product with phi, the match child's move, three mismatch children, the two gap openings (4 * x is exact) and the sum into tot
    -- and the reduction over the group's lanes through log2(64) = 6 more, fewer than a ninth level's.  So 8 * depth + 8 roundings
    bound the error by (8 * depth + 8) * 2^-24; the test allows twice that, (8 * depth + 8) * 2^-23, which also pays for the order
    of the sums (the kernel gathers, the reference scatters).
    The class is floor(log2(tot + 1) * scale): it may be the neighbour's only where that product lies within the same relative
    distance, plus the fast log2's own error, of an integer -- and such reads may be at most 1 % of a launch, counted on the
    reference"""
    ragged = bool((lens != lens[0]).any())
    m = E.launch_model(opt, int(lens.max()))
    rows_ix, depth = int(oix.seq_len), E.model_depth(int(oix.seq_len))
    n_near = 0
    for q, r in enumerate(rows):
        g = lo["ids"][r]
        n = int(lens[g])
        chain, _ = E.width_bounds(oix, codes[g, :n])
        own = E.launch_model(opt, n)["max_units"] if ragged else m["max_units"]
        tot = E.expected_nodes(codes[g, :n], [min(b, 127) for b, _ in chain], min(min(int(est[q]), 255) + m["u_tight"], own), m, rows_ix, depth)
        eps = (8 * min(n, depth) + 8) * 2.0 ** -23
        assert abs(float(lo["pred"][r]) - tot) <= eps * tot, (r, g, n, float(lo["pred"][r]), tot)
        x = math.log2(tot + 1.0) * SCALE
        near = abs(x - round(x)) < x * (eps + LOG2_ULPS)         # (tot = 0 is 0 on the device too: a sum of non-negative terms)
        n_near += near
        key, want = int(lo["key"][r]), E.order_key(tot, SCALE)
        assert key == want or (near and abs(key - want) == 1), (r, g, n, key, want, tot)
    assert n_near <= len(rows) // 100, n_near


def _check_all(oix, opt, ri, lo, codes, lens, rows):
    _check_bounds(oix, opt, ri, lo, codes, lens, rows)
    _check_model(oix, opt, lo, codes, lens, rows, _check_estimate(oix, opt, ri, lo, codes, lens, rows))


def _fixed(codes):
    return np.full(codes.shape[0], codes.shape[1], dtype=np.int64)


# ---- (a) width bounds ------------------------------------------------------------------------------------------------------
def _width_reads(gc, n, length, rng):
    """substrings with zero to two substitutions; of every eight reads one has an N as its first base, one as its last and one
    at a seam of the packing (the 16-base word, the 32-base mask word) -- one N per read, which a budget of one difference pays for"""
    reads = _substitute(_substrings(gc, n, length, rng), rng.integers(0, 3, size=n), rng)
    seams = [p for p in (15, 16, 31, 32) if p < length] or [length // 2]
    for r in range(n):
        if r % 8 == 5:
            reads[r, 0] = 4
        elif r % 8 == 6:
            reads[r, length - 1] = 4
        elif r % 8 == 7:
            reads[r, seams[(r >> 3) % len(seams)]] = 4
    return reads


@pytest.mark.parametrize("length", [1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 100, 250])
def test_width_bounds_are_the_oracles(ctx, example, gcodes, monkeypatch, length):
    """the seams of the 4-byte packing, the 16-base word and the 32-base mask word; 33: the first length with a seed chain; 100 and
    250: word 2 and the first 64 steps.  257 reads: a second workgroup with one read"""
    opt = _set_costs(ctx, "stock_n1")
    codes = _width_reads(gcodes, 257, length, np.random.default_rng(1000 + length))
    ri, lo = _launch(ctx, monkeypatch, codes)
    _check_bounds(example["orc_index"], opt, ri, lo, codes, _fixed(codes), np.arange(257))


@pytest.mark.parametrize("n", [1, 255, 256])
def test_width_bounds_at_the_workgroup_seam(ctx, example, gcodes, monkeypatch, n):
    opt = _set_costs(ctx, "stock_n1")
    codes = _width_reads(gcodes, n, 33, np.random.default_rng(2000 + n))
    ri, lo = _launch(ctx, monkeypatch, codes)
    _check_all(example["orc_index"], opt, ri, lo, codes, _fixed(codes), np.arange(n))


@pytest.fixture(scope="module")
def ragged(example, workdir):
    """18-44 bases under profile costs: one bin with reads on both sides of the 32-base seed (written as FASTQ: a batch made from
    codes holds one length)"""
    import simulate as S
    sim = S.simulate_reads(example["genome"], 700, read_len=44, min_len=18, seed=31, profile=_tc_profile(), indel_scale=3.0)
    rng = np.random.default_rng(32)
    for r in range(0, 700, 9):
        sim["codes"][r, int(rng.integers(0, sim["lens"][r]))] = 4
    fq = os.path.join(workdir, "launch_order_ragged.fq")
    S.write_fastq(fq, sim)
    return fq, sim["codes"], sim["lens"].astype(np.int64)


def test_ragged_launch(ctx, example, ragged, monkeypatch):
    """every read's own length, seed rule and budget (units_by_len): bounds, estimate, model and order of one ragged launch; the
    reads no longer than the seed have no seed bound"""
    fq, codes, lens = ragged
    assert lens.min() == 18 and lens.max() == 44 and (lens <= 32).sum() > 100 and (lens > 32).sum() > 100
    opt = _set_costs(ctx, "profile_x-1")
    assert len({E.launch_model(opt, int(n))["max_units"] for n in lens}) > 1          # budgets differ inside the launch
    ri, lo = _launch(ctx, monkeypatch, fq=fq)
    short = lens[lo["ids"]] <= 32
    assert not ((ri[short, 2] >> 8) & 0xff).any() and ((ri[~short, 2] >> 8) & 0xff).any()
    _check_all(example["orc_index"], opt, ri, lo, codes, lens, np.arange(lens.size))


# ---- (b) the estimate ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool50(gcodes):
    return _mixed_pool(gcodes, 600, 50, np.random.default_rng(41))


@pytest.mark.parametrize("costs,env", [("stock_n2", {}), ("profile_x2", {}), ("profile_x2", {"PS_ORDER_WPIN": "1"}), ("stock_n2", {"PS_ORDER_WPIN": "1"}),
                                       ("profile_x2", {"PS_ORDER_RESTART": "3"})],
                         ids=["stock", "profile", "profile_wpin1", "stock_wpin1", "profile_restart3"])
def test_estimate_is_the_two_scans(ctx, example, pool50, monkeypatch, costs, env):
    """600 reads of 50 bp: copies, one to four substitutions, an insertion, a deletion, N, both strands.  PS_ORDER_WPIN=1: an
    interval of two rows is no pinned locus any more, so scans start over where the default takes a substitution"""
    opt = _set_costs(ctx, costs)
    ri, lo = _launch(ctx, monkeypatch, pool50, env=env)
    est = _check_estimate(example["orc_index"], opt, ri, lo, pool50, _fixed(pool50), np.arange(600),
                          c_restart=int(env["PS_ORDER_RESTART"]) if "PS_ORDER_RESTART" in env else None, w_pin=int(env.get("PS_ORDER_WPIN", W_PIN)))
    assert len(set(est.tolist())) > 2
    if not env:
        _check_model(example["orc_index"], opt, lo, pool50, _fixed(pool50), np.arange(600), est)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_estimate_at_the_half_wave_seam(ctx, example, pool50, monkeypatch, n):
    """lanes 0..31 of a wave run scan A of 32 reads, lanes 32..63 scan B of the same reads: launches that end on either side of it"""
    opt = _set_costs(ctx, "profile_x2")
    codes = pool50[100:100 + n]
    ri, lo = _launch(ctx, monkeypatch, codes)
    _check_estimate(example["orc_index"], opt, ri, lo, codes, _fixed(codes), np.arange(n))


def test_estimate_on_repeats(multi, monkeypatch):
    """a tandem repeat of twelve copies and a duplication across contigs: intervals wider than w_pin (PS_ORDER_WPIN=4) where a
    scan meets a difference, so it starts over there instead of taking a substitution"""
    import capi
    import simulate as S
    monkeypatch.setenv("PS_READ_ITERS", "1")
    c = capi.Ctx.build(multi["fa"])
    try:
        chr_b, chr_c = S.contig_codes(multi["genome"][1][1]), S.contig_codes(multi["genome"][2][1])
        rng = np.random.default_rng(51)
        reads = np.stack([chr_b[a:a + 40] for a in rng.integers(2990, 3000 + 37 * 12 - 36, size=160)] + [chr_c[a:a + 40] for a in rng.integers(4000, 4560, size=96)])
        rev = rng.random(256) < 0.5
        reads[rev] = S.COMP[reads[rev][:, ::-1]]
        _substitute(reads, rng.integers(0, 3, size=256), rng)
        E.check_prefix_counts(multi["orc_index"], E.fm_of(multi["orc_index"]))
        for wpin in (16, 4):
            opt = _set_costs(c, "profile_x2")
            ri, lo = _launch(c, monkeypatch, reads, env={"PS_ORDER_WPIN": str(wpin)})
            _check_estimate(multi["orc_index"], opt, ri, lo, reads, _fixed(reads), np.arange(256), w_pin=wpin)
            _check_bounds(multi["orc_index"], opt, ri, lo, reads, _fixed(reads), np.arange(256))
    finally:
        c.close()


# ---- (c) the model ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_light(gcodes):
    """no read without a hit inside a budget of seven average mismatches: zero to two substitutions, N"""
    return _mixed_pool(gcodes, 300, 50, np.random.default_rng(61), heavy=False)


def test_model_with_a_lane_per_unit_of_a_large_budget(ctx, example, pool_light, monkeypatch):
    """-X 7: 57 budget units, a read per wave (k_effort_model<64>)"""
    opt = _set_costs(ctx, "profile_x7")
    assert E.launch_model(opt, 50)["max_units"] == 56
    ri, lo = _launch(ctx, monkeypatch, pool_light)
    _check_all(example["orc_index"], opt, ri, lo, pool_light, _fixed(pool_light), np.arange(300))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("costs", ["stock_n2", "profile_x2", "profile_x7"])
def test_model_groups_that_leave_early(ctx, example, pool_light, monkeypatch, costs, n):
    """G = 16, 32 and 64 lanes per read, 4, 2 and 1 reads per wave: launches of 64 / G - 1 and + 1 reads, so that a wave's last
    groups have no read"""
    opt = _set_costs(ctx, costs)
    codes = pool_light[20:20 + n]
    ri, lo = _launch(ctx, monkeypatch, codes)
    _check_all(example["orc_index"], opt, ri, lo, codes, _fixed(codes), np.arange(n))


def test_model_with_indels_away_from_the_ends(ctx, example, gcodes, monkeypatch):
    """reads with an insertion or a deletion between their tenth and their tenth-last base (and what the estimate makes of them)"""
    opt = _set_costs(ctx, "profile_x2")
    pool = _mixed_pool(gcodes, 400, 50, np.random.default_rng(71))
    codes = pool[(np.arange(400) % 10 == 6) | (np.arange(400) % 10 == 7)]
    ri, lo = _launch(ctx, monkeypatch, codes)
    assert E.launch_model(opt, 50)["max_gapo"] > 0
    _check_all(example["orc_index"], opt, ri, lo, codes, _fixed(codes), np.arange(codes.shape[0]))


def test_order_by_the_estimate_alone(ctx, example, pool50, monkeypatch):
    """PS_ORDER=2 (k_order_keys): key = cap - min(est, cap)"""
    opt = _set_costs(ctx, "profile_x2")
    ri, lo = _launch(ctx, monkeypatch, pool50, env={"PS_ORDER": "2", "PS_ORDER_CAP": "100"})
    est = _check_estimate(example["orc_index"], opt, ri, lo, pool50, _fixed(pool50), np.arange(600))
    assert np.array_equal(lo["key"], 100 - np.minimum(est, 100)) and not lo["pred"].any()
    ri, lo = _launch(ctx, monkeypatch, pool50, env={"PS_ORDER": "2", "PS_ORDER_CAP": "9"})       # a cap the estimates pass
    assert (est > 9).any() and np.array_equal(lo["key"], 9 - np.minimum(est, 9))


# ---- (e) second trips of the grid-stride loops --------------------------------------------------------------------------------
@pytest.mark.parametrize("costs,n,length", [("profile_x7", 8192 + 37, 50), ("stock_n2", 32768 + 37, 50), ("stock_n1", 262144 + 37, 33), ("stock_n1", 524288 + 37, 33)],
                         ids=["model64", "model16", "effort", "width"])
def test_second_trip(ctx, example, gcodes, monkeypatch, costs, n, length):
    """launches past the block clamp of k_effort_model<64>, k_effort_model<16>, k_effort and k_width (33 bp: the seed chain is
    live): random substrings with zero to two substitutions"""
    opt = _set_costs(ctx, costs)
    rng = np.random.default_rng(n)
    codes = _substitute(_substrings(gcodes, n, length, rng), rng.integers(0, 3, size=n), rng)
    ri, lo = _launch(ctx, monkeypatch, codes)
    rows = _rows(n, CLAMPS)
    assert rows.size < 2700 and (rows >= max(c for c in CLAMPS if c < n)).sum() == 37
    _check_all(example["orc_index"], opt, ri, lo, codes, _fixed(codes), rows)


# ---- (f) the order is worth something -------------------------------------------------------------------------------------------
# measured on the first run of this test: the share of all true iterations in the first tenth of the queue
SHARE_LIBRARY, SHARE_INPUT, SHARE_SORTED = 0.2751, 0.0985, 0.3186


def test_order_puts_the_work_first(ctx, example, monkeypatch):
    """8,192 reads of 50 bp under -X -1 with indels and 0.2 % N.  The library's order must beat input order by at least half the gap
    measured between them -- a constant or an inverted key does not -- and cannot beat the sort by the true counts; the other
    half of the gap is the leading-base order inside a class and run-to-run noise of a search that races for its large stack slots"""
    import simulate as S
    _set_costs(ctx, "profile_x-1")
    sim = S.simulate_reads(example["genome"], 8192, 50, seed=81, profile=_tc_profile(), indel_scale=5.0, n_frac=0.002)
    ri, lo = _launch(ctx, monkeypatch, sim["codes"])
    it = ri[:, 0].astype(np.float64)
    tenth = 8192 // 10
    share = lambda rows: float(it[rows[:tenth]].sum() / it.sum())
    lib, inp, best = share(lo["order"]), share(np.argsort(lo["ids"], kind="stable")), share(np.argsort(-it, kind="stable"))
    print("share of the iterations in the first tenth of the queue: library %.4f, input order %.4f, sorted by true iterations %.4f" % (lib, inp, best))
    assert lib <= best
    assert lib >= inp + 0.5 * (SHARE_LIBRARY - SHARE_INPUT)
