"""Plain restatements of what a search launch is prepared with: the width stage's D(i) bounds, the effort estimate's two greedy
scans and the expected-nodes model (NumPy, float64, the oracle's C for the index).  Nothing here is taken from the .hip files
but the rules they state:

  * width_bounds   -- upstream's bwt_cal_width, through the oracle (oracle/ps_oracle.c: orc_cal_width);
  * effort_scans   -- items 1 and 3 of the head of csrc/ps_effort.hip;
  * expected_nodes -- item 2 there, with the search's own tests as csrc/ps_narrow.h applies them (nt_head: the pop's test;
    nt_tail: which children an expansion has and what they cost; nt_m_seed: the seed's budget).

Read codes are 0..3 = A C G T, anything above = N, in read orientation throughout."""
import math

import numpy as np

CLUSTER_SPAN = 4        # "three substitutions within a few bases of each other": each at most this far from the one before
CLUSTER_SIZE = 3


# ---- the cost model of a launch (csrc/ps_model.h: make_model, in the oracle's option struct) -----------------------------------
def launch_model(opt, length):
    """what the search of reads of one length works with, in budget units: dict(max_units, c_min, inv_c_min, u_tight, u_mm [5][4]
    (read code s of the reverse-complemented read against text symbol t), u_gapo_ins, u_gapo_del, max_gapo, indel_end_skip,
    use_seed, seed_len, seed_units)"""
    import orc
    L = orc.lib()
    u_mm = np.zeros((5, 4), dtype=np.int64)
    if opt.profile:
        diffs = opt.x_avg_mm if opt.x_avg_mm >= 0 else L.orc_cal_maxdiff(int(length), 0.02, 0.04)
        for s in range(5):
            for t in range(4):
                u_mm[s, t] = opt.n_cost if s == 4 else (0 if s == t else opt.sub_cost[(3 - t) * 4 + (3 - s)])
        gaps = [opt.gapo_ins_cost, opt.gapo_del_cost, opt.gape_cost]
        c_min = max(1, min([int(c) for c in u_mm.reshape(-1) if c > 0] + gaps))
        m = dict(max_units=diffs * opt.unit, c_min=c_min, u_tight=opt.unit, u_gapo_ins=opt.gapo_ins_cost, u_gapo_del=opt.gapo_del_cost,
                 max_gapo=opt.max_gapo)
    else:
        diffs = L.orc_cal_maxdiff(int(length), 0.02, opt.fnr) if opt.fnr > 0.0 else opt.max_diff
        for s in range(5):
            for t in range(4):
                u_mm[s, t] = int(s != t)
        m = dict(max_units=diffs, c_min=1, u_tight=1, u_gapo_ins=1, u_gapo_del=1, max_gapo=min(opt.max_gapo, diffs))
    m.update(u_mm=u_mm, inv_c_min=(65536 + m["c_min"] - 1) // m["c_min"], indel_end_skip=opt.indel_end_skip,
             use_seed=length > opt.seed_len, seed_len=opt.seed_len if length > opt.seed_len else 0,
             seed_units=opt.max_seed_diff * m["u_tight"], profile=bool(opt.profile))
    return m


def average_mismatch(u_mm):
    """what a restart is charged where PS_ORDER_RESTART does not say: the mean of the twelve substitution costs, rounded, at least 1"""
    return max(1, (int(sum(u_mm[s, t] for s in range(4) for t in range(4) if s != t)) + 6) // 12)


# ---- the index as prefix counts --------------------------------------------------------------------------------------------
class Fm:
    """Occ from prefix counts of the BWT string: occ(row)[c] = symbols c in rows 0..row of the BW matrix of T$ (the '$' row, row
    `primary`, holds none and is not stored)"""

    def __init__(self, oix):
        syms = oix.bwt_syms()
        self.seq_len, self.primary, self.L2 = int(oix.seq_len), int(oix.primary), [int(v) for v in oix.L2]
        self.P = np.zeros((self.seq_len + 1, 4), dtype=np.int64)
        for c in range(4):
            np.cumsum(syms == c, out=self.P[1:, c])

    def occ(self, row):
        if row < 0:
            return self.P[0]
        return self.P[min(self.seq_len, row + 1 - (1 if row >= self.primary else 0))]


_FM = {}


def fm_of(oix):
    if id(oix) not in _FM:
        _FM[id(oix)] = (oix, Fm(oix))        # the index is kept with its counts: an id is only unique while its object lives
    return _FM[id(oix)][1]


def check_prefix_counts(oix, fm):
    """the prefix counts against the oracle's own Occ: at the edges of its 128-symbol blocks and of the device's 192-symbol ones,
    around the '$' row and at both ends; and L2 against the totals"""
    n, p = fm.seq_len, fm.primary
    rows = {-1, 0, 1, n - 2, n - 1, n}
    for blk in (64, 128, 192):
        for e in list(range(blk, min(n, 6 * blk) + 1, blk)) + [n // blk * blk, (p // blk) * blk, (p // blk + 1) * blk]:
            rows.update((e - 2, e - 1, e, e + 1))
    rows.update(range(p - 3, p + 4))
    for row in sorted(r for r in rows if -1 <= r <= n):
        got = fm.occ(row)
        for c in range(4):
            assert int(got[c]) == oix.occ(row, c), (row, c)
    tot = fm.occ(n)
    for c in range(4):
        assert fm.L2[c] == int(tot[:c].sum()), c
    return len(rows)


# ---- D(i) bounds ---------------------------------------------------------------------------------------------------------
def width_bounds(oix, read, seed_len=0):
    """-> (read chain, seed chain): per chain step i = 0..len a pair (bid, w == the step before's w), both from the oracle's
    bwt_cal_width over the read reversed; the seed chain is the same over the first seed_len bases (None: the read is no
    longer than the seed, or seed_len is 0).  Step len closes the chain: bid one more, w = 0"""
    read = np.minimum(np.asarray(read, dtype=np.uint8), 4)

    def chain(codes):
        w = oix.cal_width(codes[::-1])
        return [(bid, i > 0 and wi == w[i - 1][0]) for i, (wi, bid) in enumerate(w)]
    return chain(read), (chain(read[:seed_len]) if 0 < seed_len < read.size else None)


def pack_bounds(chain, n_bytes=None):
    """the chain as the launch packs it: a byte per step, min(bid, 127) | equal-width flag << 7, four steps per little-endian word"""
    b = np.array([min(bid, 127) | (0x80 if eq else 0) for bid, eq in chain], dtype=np.uint8)
    n_bytes = (b.size + 3) // 4 * 4 if n_bytes is None else n_bytes
    out = np.zeros(n_bytes, dtype=np.uint8)
    out[:min(n_bytes, b.size)] = b[:n_bytes]
    return out.view("<u4")


# ---- the estimate: two greedy scans ----------------------------------------------------------------------------------------
def _scan(fm, syms, cost_rows, positions, c_restart, w_pin):
    """one scan: syms[i] the symbol the pattern grows by at step i (4: N), cost_rows[i][t] what text symbol t costs there instead,
    positions[i] the read position of that base -> (total, restarts)"""
    k, l, total, n_rs, cl_n, cl_last = 0, fm.seq_len, 0, 0, 0, 0
    for sym, cost, pos in zip(syms, cost_rows, positions):
        ck, cl = fm.occ(k - 1), fm.occ(l)
        if sym < 4 and ck[sym] < cl[sym]:                       # the exact extension goes on
            k, l = fm.L2[sym] + int(ck[sym]) + 1, fm.L2[sym] + int(cl[sym])
            continue
        best = -1
        if l - k + 1 <= w_pin:                                  # the locus is pinned down: the cheapest substitution that continues it
            for t in range(4):
                if t != sym and ck[t] < cl[t] and (best < 0 or cost[t] < cost[best]):
                    best = t
        if best < 0:                                            # a new piece, an average mismatch
            k, l, cl_n, n_rs, total = 0, fm.seq_len, 0, n_rs + 1, total + c_restart
            continue
        cl_n = cl_n + 1 if cl_n > 0 and abs(pos - cl_last) <= CLUSTER_SPAN else 1
        cl_last = pos
        total += int(cost[best])
        if cl_n >= CLUSTER_SIZE:                                # they stay charged, the scan goes on with a new piece
            k, l, cl_n, n_rs = 0, fm.seq_len, 0, n_rs + 1
            continue
        k, l = fm.L2[best] + int(ck[best]) + 1, fm.L2[best] + int(cl[best])
    return total, n_rs


def effort_scans(oix, read, costs, c_restart, w_pin):
    """costs: the model's u_mm [5][4].  -> (total A, restarts A, total B, restarts B, estimate).  Scan A grows the read itself
    leftwards from its last base; scan B grows the reverse complement, i.e. takes the read from its first base (the index holds
    both strands).  Base b of the read against text symbol t costs u_mm[3 - b][t] on the reverse-complemented read -- scan B --
    and u_mm[3 - b][3 - t] on the read itself, the other strand -- scan A.
    The estimate: a scan that never started over has priced a real alignment, so its total stands (the cheaper one if neither did);
    where both started over, the larger total counts"""
    fm = fm_of(oix)
    read = np.minimum(np.asarray(read, dtype=np.int64), 4)
    costs = np.asarray(costs, dtype=np.int64)
    n = read.size
    code = np.where(read > 3, 4, 3 - read)
    pos_a = np.arange(n - 1, -1, -1)
    ta, ra = _scan(fm, read[pos_a], [costs[code[j]][::-1] for j in pos_a], pos_a, c_restart, w_pin)
    pos_b = np.arange(n)
    tb, rb = _scan(fm, code[pos_b], [costs[code[j]] for j in pos_b], pos_b, c_restart, w_pin)
    if ra == 0 and rb == 0:
        est = min(ta, tb)
    elif ra == 0 or rb == 0:
        est = ta if ra == 0 else tb
    else:
        est = max(ta, tb)
    return ta, ra, tb, rb, est


def _scan_many(fm, syms, cost4, pos, valid, c_restart, w_pin):
    """_scan over many reads at once, a step of all of them per pass: syms, pos, valid [R, S], cost4 [R, S, 4]; valid: the read
    has a step i (reads of several lengths).  -> (totals, restarts)"""
    R, S = syms.shape
    ar, n, L2 = np.arange(R), fm.seq_len, np.asarray(fm.L2[:4], dtype=np.int64)
    k, l = np.zeros(R, dtype=np.int64), np.full(R, n, dtype=np.int64)
    total, n_rs, cl_n, cl_last = (np.zeros(R, dtype=np.int64) for _ in range(4))
    at = lambda row: np.where(row < 0, 0, np.minimum(n, row + 1 - (row >= fm.primary)))
    for i in range(S):
        v, sym = valid[:, i], syms[:, i]
        ck, cl = fm.P[at(k - 1)], fm.P[at(l)]
        there = ck < cl
        sym3 = np.minimum(sym, 3)
        ext = v & (sym < 4) & there[ar, sym3]
        cand = there & (np.arange(4)[None, :] != sym[:, None]) & ((l - k + 1) <= w_pin)[:, None]
        best = np.argmin(np.where(cand, cost4[:, i, :], 1 << 30), axis=1)        # the first of the cheapest
        sub, rst = v & ~ext & cand.any(axis=1), v & ~ext & ~cand.any(axis=1)
        near = (cl_n > 0) & (np.abs(pos[:, i] - cl_last) <= CLUSTER_SPAN)
        cl_n = np.where(sub, np.where(near, cl_n + 1, 1), cl_n)
        cl_last = np.where(sub, pos[:, i], cl_last)
        total = total + np.where(sub, cost4[ar, i, best], 0) + np.where(rst, c_restart, 0)
        over = rst | (sub & (cl_n >= CLUSTER_SIZE))
        n_rs, cl_n = n_rs + over, np.where(over, 0, cl_n)
        t = np.where(ext, sym3, best)
        move = ext | (sub & ~over)
        k = np.where(move, L2[t] + ck[ar, t] + 1, np.where(over, 0, k))
        l = np.where(move, L2[t] + cl[ar, t], np.where(over, n, l))
    return total, n_rs


def effort_scans_many(oix, codes, lens, costs, c_restart, w_pin):
    """effort_scans for the reads codes[r, :lens[r]], all at once -> five arrays (test_effort_model_cpu.py holds it against the
    plain one read by read)"""
    fm = fm_of(oix)
    lens = np.asarray(lens, dtype=np.int64)
    R, S = lens.size, int(lens.max())
    costs = np.asarray(costs, dtype=np.int64)
    step = np.arange(S)[None, :]
    valid = step < lens[:, None]
    out = []
    for pos in (np.where(valid, lens[:, None] - 1 - step, 0), np.where(valid, step, 0)):
        read = np.minimum(np.asarray(codes, dtype=np.int64)[np.arange(R)[:, None], pos], 4)
        code = np.where(read > 3, 4, 3 - read)
        scan_a = len(out) == 0
        out.append(_scan_many(fm, read if scan_a else code, costs[code][:, :, ::-1] if scan_a else costs[code], pos, valid, c_restart, w_pin))
    (ta, ra), (tb, rb) = out
    est = np.where((ra == 0) & (rb == 0), np.minimum(ta, tb), np.where(ra == 0, ta, np.where(rb == 0, tb, np.maximum(ta, tb))))
    return ta, ra, tb, rb, est


def pack_est_ab(ta, ra, tb, rb):
    """the two totals as the per-read profile holds them: min(total, 127) | started over << 7, scan A low byte, scan B high"""
    return (min(ta, 127) | (0x80 if ra else 0)) | ((min(tb, 127) | (0x80 if rb else 0)) << 8)


# ---- the model: the search's rules on expected counts ----------------------------------------------------------------------
def model_depth(rows):
    """levels the model walks: three past the first level whose 4^level strings outnumber the rows of the index"""
    lv = 0
    while lv < 31 and (rows >> (2 * lv)) > 0:
        lv += 1
    return lv + 3


def expected_nodes(read, D, budget, m, rows, depth):
    """W[u] = expected live partial alignments with u units spent after d bases; a level's states are expanded into the next level's
    (scatter), pruned by the tests of csrc/ps_narrow.h; returns the expected number of nodes the search expands, `tot`.
    read: the codes; D[i]: the bound of chain step i (width_bounds, 7 bits); budget: the units the search ends with; m: launch_model
    of the LAUNCH (its seed rule and gap limit) -- the budget is the read's own; rows: of the index; depth: levels walked, what is
    alive after them walks the rest of the read.
    What the model leaves out (ps_effort.hip, item 2): gap extensions and the gap states, the seed's own bounds (only its budget)
    and the equal-width rule that spares the mismatch children.  Every child of a level, a gap opening too, is a state of the next
    level and exists with the chance that a string of that many symbols occurs at all, min(1, rows / 4^(d+1))"""
    read = np.minimum(np.asarray(read, dtype=np.int64), 4)
    n, B = read.size, int(budget)
    depth = min(n, depth)
    inv, u_mm = m["inv_c_min"], m["u_mm"]
    afford = lambda units: (units * inv) >> 16 if units >= 0 else -1          # differences that many units still pay for (units / c_min)
    W = np.zeros(B + 1, dtype=np.float64)
    W[0] = 1.0
    tot = 0.0
    for d in range(depth):
        i = n - 1 - d                                          # the search's position: read base d against seq[i]
        s = 4 if read[d] > 3 else 3 - int(read[d])
        phi = min(1.0, rows / 4.0 ** (d + 1))
        in_seed = m["use_seed"] and n > m["seed_len"] and i > 0 and i - (n - m["seed_len"]) > 0
        gap_here = m["max_gapo"] > 0 and i >= m["indel_end_skip"] and n - i >= m["indel_end_skip"]
        Wn = np.zeros(B + 1, dtype=np.float64)
        for u in range(B + 1):
            if W[u] == 0.0:
                continue
            left = afford(B - u)
            if left < int(D[i]):                               # nt_head: the pop's own test
                continue
            tot += W[u]
            wc = W[u] * phi
            if s < 4:
                Wn[u] += wc                                    # the match child
            allow = left - 1 >= int(D[i - 1]) if i > 0 else True             # nt_tail: a child with a difference must still afford D(i-1)
            if in_seed:                                        # ... and inside the seed one of the differences its budget pays for (nt_m_seed)
                s_left = m["seed_units"] - u
                allow = allow and (afford(s_left) if s_left > 0 else 0) >= 1
            if not allow:
                continue
            for t in range(4):
                if t != s and u + u_mm[s, t] <= B:
                    Wn[u + u_mm[s, t]] += wc
            if gap_here:
                if u + m["u_gapo_del"] <= B:
                    Wn[u + m["u_gapo_del"]] += 4.0 * wc        # a deletion of either text symbol
                if u + m["u_gapo_ins"] <= B:
                    Wn[u + m["u_gapo_ins"]] += wc
        W = Wn
    return tot + float(W.sum()) * (n - depth)


def order_key(tot, scale):
    """the class the hand-out order sorts by: ascending = heaviest first"""
    return 255 - min(255, int(math.floor(math.log2(tot + 1.0) * scale)))
