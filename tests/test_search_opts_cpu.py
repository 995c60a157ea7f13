"""CPU tier of the search options (include/parasuite_hip.h: ps_search_opts).

* The product's conversion ps_search_opts -> Options -> Model (csrc/ps_search_opts.h, ps_model.h), run by tests/search_opts_check.cpp -- a plain
  executable built here with the host compiler, AddressSanitizer and UBSan -- hands its Model bytes to the unchanged lane machine of
  tests/hostsim; the hit lists must equal the oracle's under the same options, which this file states in the oracle's own fields.
  A read the narrow stack reports as overflowing goes to the wide stack, as the product's tiers do.
* ps_search_opts_check through ctypes (the library loads without a GPU): every limit from both sides.
* The merge of a context's two option parts in either order of calls, and the `bwa` shim's command lines and .sai stub
  (csrc/bwa_args.h), in the same executable."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import orc
import simulate as S
from test_capi_cpu import ROOT
from test_hostsim import ALNREC, _run, hs, sim_index   # noqa: F401  (fixtures)

CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
FIELDS = ("max_gap_opens", "max_gap_extensions", "indel_end_skip", "max_del_occ", "seed_len", "max_seed_diff", "max_entries",
          "s_mm", "s_gapo", "s_gape", "max_top2", "max_alt_hits")
DEFAULTS = dict(zip(FIELDS, (1, -1, 5, 10, 32, 2, 2000000, 3, 11, 4, 30, 3)))
FLAG = dict(o="max_gap_opens", e="max_gap_extensions", i="indel_end_skip", d="max_del_occ", l="seed_len", k="max_seed_diff",
            m="max_entries", M="s_mm", O="s_gapo", E="s_gape", R="max_top2", n="max_alt_hits")
FULL = 4 + 4 * len(FIELDS)
PROFILE = S.EXAMPLE_PROFILE.copy()
PROFILE[3, 1], PROFILE[3, 3] = 0.12, 0.87


def opts(**flags):
    """o=2, l=20 ... -> all twelve fields"""
    d = dict(DEFAULTS)
    for f, v in flags.items():
        d[FLAG[f]] = v
    return d


def orc_fields(d):
    """the same options in the oracle's fields (orc_opt_t): the rule of `bwa aln -e`, stated here a second time"""
    e = d["max_gap_extensions"]
    return dict(max_gapo=d["max_gap_opens"], max_gape=e if e >= 1 else 6, mode_gape=0 if e >= 1 else 1,
                indel_end_skip=d["indel_end_skip"], max_del_occ=d["max_del_occ"], max_entries=d["max_entries"],
                seed_len=d["seed_len"], max_seed_diff=d["max_seed_diff"], max_top2=d["max_top2"],
                s_mm=d["s_mm"], s_gapo=d["s_gapo"], s_gape=d["s_gape"], n_occ=d["max_alt_hits"])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sopts") / "search_opts_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g",
                           "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(ROOT, "tests", "search_opts_check.cpp"), "-o", out])
    return out


def _lines(exe, args, stdin=""):
    return subprocess.run([exe] + list(args), input=stdin, check=True, timeout=120, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def case_line(d, length, cost="0.04", profile=False, struct_size=FULL):
    s = "%s %d %s %d %s" % ("profile" if profile else "stock", length, cost, struct_size, " ".join(str(d[f]) for f in FIELDS))
    if profile:
        s += " " + " ".join(repr(float(v)) for v in PROFILE.reshape(16)) + " %r %r" % (S.INS_RATE, S.DEL_RATE)
    return s


def product_model(exe, d, length, **kw):
    """(wide, Model bytes) of the product's conversion + make_model"""
    line, = _lines(exe, ["models"], case_line(d, length, **kw) + "\n")
    assert line.startswith("ok "), line
    _, wide, hexbytes = line.split()
    return int(wide), bytes.fromhex(hexbytes)


def compare_with_oracle(hs, h, ix, opt, model_bytes, wide, codes, want=None):
    """hit lists of the lane machine under the product's Model == the oracle's under opt; returns the lane machine's lists"""
    assert len(model_bytes) == hs.hs_sizeof_model()
    model = (C.c_uint8 * len(model_bytes)).from_buffer_copy(model_bytes)
    codes = np.ascontiguousarray(codes)
    alns, n_aln, status, _ = _run(hs, h, model, codes, pool_cap=16384, aln_cap=64, wide=wide)
    todo = np.nonzero(status != 0)[0]
    if todo.size:                                            # the product's next tiers (a deeper stack, a longer hit list); the wide stack keeps upstream's exact -m count
        assert set(status[todo].tolist()) <= {1, 2, 4}
        a2, n2, s2, _ = _run(hs, h, model, codes[todo], n_lanes=4, pool_cap=200000, aln_cap=256, wide=1)
        assert not s2.any()
    out = []
    keys = ("k", "l", "n_mm", "n_gapo", "n_gape", "n_ins", "n_del", "score", "units")
    for r in range(codes.shape[0]):
        n, ref = ix.aln_one(opt, codes[r], cap=256)
        if status[r] == 0:
            rows, cnt = alns[r], int(n_aln[r])
        else:
            q = int(np.nonzero(todo == r)[0][0])
            rows, cnt = a2[q], int(n2[q])
        got = [tuple(int(a[f]) for f in keys) for a in rows[:cnt]]
        assert n == cnt and got == [tuple(a[f] for f in keys) for a in ref], r
        out.append(got)
    if want is not None:
        want(out, int(todo.size))
    return out


STOCK_CASES = (
    [dict(o=v) for v in (0, 2, 3)] +
    [dict(e=v) for v in (-1, 0, 2, 3, 7)] +                  # below 1: the k-difference mode; from 1 on: extensions that are no differences
    [dict(o=2, e=3)] +
    [dict(i=v) for v in (0, 1, 12)] +
    [dict(d=v) for v in (0, 1, 200)] +
    [dict(l=l, k=k) for l, k in ((10, 0), (10, 3), (20, 1), (25, 0), (25, 3), (49, 1), (50, 1), (1000, 0), (1000, 3), (20, 0))] +
    [dict(R=v) for v in (0, 1, 5, 254, 1000)] +
    [dict(M=1, O=1, E=1), dict(M=5, O=6, E=1), dict(M=0, O=11, E=4), dict(M=3, O=0, E=0), dict(M=2, O=20, E=9)] +
    [dict(m=50), dict(m=500)]
)


@pytest.fixture(scope="module")
def sim_reads(example):
    return {L: S.simulate_reads(example["genome"], 200, L, seed=41 + L, indel_scale=60, n_frac=0.002)["codes"] for L in (50, 36)}


@pytest.mark.parametrize("flags", STOCK_CASES, ids=lambda f: "-".join("%s%s" % kv for kv in f.items()))
def test_model_conversion_matches_oracle_stock(exe, hs, sim_index, example, sim_reads, flags):
    d = opts(**flags)
    for L in (50, 36):
        wide, mb = product_model(exe, d, L)
        compare_with_oracle(hs, sim_index, example["orc_index"], orc.stock_opt("0.04", **orc_fields(d)), mb, wide, sim_reads[L])


def test_model_conversion_matches_oracle_profile(exe, hs, sim_index, example, sim_reads):
    d = opts(o=2, l=20, k=1)
    for L in (50, 36):
        wide, mb = product_model(exe, d, L, cost="-1", profile=True)
        compare_with_oracle(hs, sim_index, example["orc_index"], orc.profile_opt(PROFILE, S.INS_RATE, S.DEL_RATE, -1, **orc_fields(d)),
                            mb, wide, sim_reads[L])


def indel_reads(example, n, lo, hi, seed):
    """50-bp reads with one deletion or insertion of lo..hi bases in the middle (the simulator makes single-base indels only)"""
    fwd = example["orc_index"].forward_codes()
    rng = np.random.default_rng(seed)
    out = np.empty((n, 50), dtype=np.uint8)
    for r in range(n):
        while True:
            p = int(rng.integers(20000, 200000))
            if (fwd[p:p + 80] < 4).all():
                break
        k, at = int(rng.integers(lo, hi + 1)), int(rng.integers(18, 32))
        if r & 1:
            read = np.concatenate([fwd[p:p + at], fwd[p + at + k:p + 50 + k]])                     # deletion from the reference
        else:
            read = np.concatenate([fwd[p:p + at], rng.integers(0, 4, k).astype(np.uint8), fwd[p + at:p + 50 - k]])
        out[r] = read if rng.random() < 0.5 else (3 - read[::-1])
    return out


@pytest.mark.parametrize("flags,longest", [(dict(e=8), 8), (dict(e=12), 8), (dict(o=3, e=9), 8), (dict(e=5), 5)], ids=["e8", "e12", "o3-e9", "e5"])
def test_long_gaps_match_oracle(exe, hs, sim_index, example, flags, longest):
    """-e above 7 takes the wide stack (launch_is_wide); reads with 5-9-base indels are found with the gap the option allows"""
    d = opts(**flags)
    wide, mb = product_model(exe, d, 50)
    assert wide == (1 if d["max_gap_opens"] + d["max_gap_extensions"] > 7 else 0)
    reads = indel_reads(example, 120, 5, 9, seed=7)

    def want(lists, n_escalated):
        gape = [a[4] for hits in lists for a in hits]
        assert max(gape) == longest and sum(1 for hits in lists if hits) >= 20

    compare_with_oracle(hs, sim_index, example["orc_index"], orc.stock_opt("0.04", **orc_fields(d)), mb, wide, reads, want)


def test_r_300_takes_the_wide_stack(exe, hs, sim_index, example, sim_reads):
    d = opts(R=300)
    wide, mb = product_model(exe, d, 50)
    assert wide == 1
    assert product_model(exe, opts(R=254), 50)[0] == 0
    compare_with_oracle(hs, sim_index, example["orc_index"], orc.stock_opt("0.04", **orc_fields(d)), mb, wide, sim_reads[50])


def test_small_m_escalates_to_the_wide_stack(exe, hs, sim_index, example, sim_reads):
    """-m 50: the narrow tier hands the reads that reach the limit on (ps_narrow.h), the wide tier ends them at upstream's exact count"""
    d = opts(m=50)
    wide, mb = product_model(exe, d, 50)
    seen = []
    compare_with_oracle(hs, sim_index, example["orc_index"], orc.stock_opt("0.04", **orc_fields(d)), mb, wide, sim_reads[50],
                        lambda lists, n_escalated: seen.append(n_escalated))
    assert wide == 0 and seen[0] > 0


# ---- the draw of the GPU fuzz (tests/test_gpu_search_opts.py), on the lane machine first ------------------------------------------
def n_buckets(d, md):
    """make_model's count of score buckets under stock costs (ps_model.h), restated: the draw stays inside PS_MAX_BUCKETS = 128"""
    o = orc_fields(d)
    top = 0
    for bb in range(min(o["max_gapo"], md) + 1):
        for cc in range((o["max_gape"] if bb else 0) + 1):
            used = bb + (cc if o["mode_gape"] else 0)
            if used <= md:
                top = max(top, (md - used) * o["s_mm"] + bb * o["s_gapo"] + cc * o["s_gape"])
    return top + 1


def draw_options(rng):
    """all twelve fields inside their accepted ranges, the ends of every range among them.  -n stays at 0.04 (3 differences at 50 bp);
    the score table is drawn again until it fits PS_MAX_BUCKETS.  (The oracle maps 4,096 reads under -o 7 -e 15 in 0.15 s here.)"""
    while True:
        d = dict(DEFAULTS)
        d["max_gap_opens"] = int(rng.choice([0, 1, 1, 2, 3, 4, 7]))
        d["max_gap_extensions"] = int(rng.choice([-1, -1, 0, 1, 2, 4, 7, 8, 12, 15]))
        d["indel_end_skip"] = int(rng.choice([0, 1, 5, 5, 12, 30, 255]))
        d["max_del_occ"] = int(rng.choice([0, 1, 10, 10, 100, 255]))
        d["seed_len"] = int(rng.choice([1, 10, 20, 25, 32, 32, 49, 50, 1000]))
        d["max_seed_diff"] = int(rng.choice([0, 1, 2, 2, 3, 4095]))
        d["max_entries"] = int(rng.choice([1, 50, 500, 5000, 2000000, 2000000, 2000000]))
        d["s_mm"], d["s_gapo"], d["s_gape"] = int(rng.integers(0, 41)), int(rng.integers(0, 61)), int(rng.integers(0, 16))
        if rng.random() < 0.4:
            d["s_mm"], d["s_gapo"], d["s_gape"] = 3, 11, 4
        d["max_top2"] = int(rng.choice([0, 1, 4, 30, 30, 254, 255, 400]))
        d["max_alt_hits"] = int(rng.choice([0, 1, 3, 3, 10, 20]))
        if n_buckets(d, 3) <= 128:
            return d


@pytest.mark.parametrize("case", range(40))
def test_fuzz_draw_on_the_lane_machine(exe, hs, sim_index, example, sim_reads, case):
    """every case of the GPU fuzz's draw, 100 simulated and 40 long-gap reads each, before a device sees it"""
    d = draw_options(np.random.default_rng(77000 + case))
    wide, mb = product_model(exe, d, 50)
    reads = np.concatenate([sim_reads[50][:100], indel_reads(example, 40, 2, 9, seed=case)])
    compare_with_oracle(hs, sim_index, example["orc_index"], orc.stock_opt("0.04", **orc_fields(d)), mb, wide, reads)


# ---- the range check, through the library ---------------------------------------------------------------------------------------
LIMITS = [  # field, flag in the message, last accepted below, first refused below, last accepted above, first refused above (None: none)
    ("max_gap_opens", "aln -o", 0, -1, 7, 8),
    ("max_gap_extensions", "aln -e", -1000, None, 15, 16),
    ("indel_end_skip", "aln -i", 0, -1, 100000, None),
    ("max_del_occ", "aln -d", 0, -1, 255, 256),
    ("seed_len", "aln -l", 1, 0, 1000000, None),
    ("max_seed_diff", "aln -k", 0, -1, 4095, 4096),
    ("max_entries", "aln -m", 1, 0, 2000000, 2000001),
    ("s_mm", "aln -M", 0, -1, 255, 256),
    ("s_gapo", "aln -O", 0, -1, 255, 256),
    ("s_gape", "aln -E", 0, -1, 255, 256),
    ("max_top2", "aln -R", 0, -1, 1000000, None),
    ("max_alt_hits", "samse -n", 0, -1, 1000000, None),
]


@pytest.mark.parametrize("field,flag,ok_lo,bad_lo,ok_hi,bad_hi", LIMITS, ids=[l[0] for l in LIMITS])
def test_range_check_each_limit_from_both_sides(field, flag, ok_lo, bad_lo, ok_hi, bad_hi):
    import capi
    for v in (ok_lo, ok_hi):
        capi.SearchOpts(**{field: v}).check()
    for v, limit in ((bad_lo, ok_lo), (bad_hi, ok_hi)):
        if v is None:
            continue
        with pytest.raises(capi.PsError) as ei:
            capi.SearchOpts(**{field: v}).check()
        msg = str(ei.value)
        assert field in msg and flag in msg and str(v) in msg and str(limit) in msg, msg


def test_range_check_profile_mode_and_struct_size():
    import capi
    capi.SearchOpts(max_seed_diff=511).check(profile_mode=True)
    with pytest.raises(capi.PsError, match=r"max_seed_diff \(aln -k\) is 512, accepted: 0 to 511"):
        capi.SearchOpts(max_seed_diff=512).check(profile_mode=True)
    L = capi.lib()
    assert L.ps_search_opts_check(None, 0) == 0                       # NULL: the defaults
    o = capi.SearchOpts()
    assert o.struct_size == C.sizeof(capi.SearchOpts) == FULL
    assert [getattr(o, f) for f in FIELDS] == [DEFAULTS[f] for f in FIELDS]
    # a caller built against a shorter struct: the fields behind its size are not read
    o = capi.SearchOpts(max_gap_opens=2, max_del_occ=999)
    o.struct_size = 12                                              # struct_size, max_gap_opens, max_gap_extensions
    assert L.ps_search_opts_check(C.byref(o), 0) == 0
    o.struct_size = 20
    assert L.ps_search_opts_check(C.byref(o), 0) == 1 and b"max_del_occ" in L.ps_last_error()
    for bad in (0, 3, 10, FULL + 4):
        o.struct_size = bad
        assert L.ps_search_opts_check(C.byref(o), 0) == 1 and b"struct_size" in L.ps_last_error(), bad
    with pytest.raises(TypeError):
        capi.SearchOpts(max_gapo=1)


def test_shorter_struct_keeps_defaults_in_the_model(exe):
    d = opts(o=2, e=99, d=999)                                        # only struct_size + max_gap_opens lie inside 8 bytes
    assert product_model(exe, d, 50, struct_size=8) == product_model(exe, opts(o=2), 50)
    line, = _lines(exe, ["models"], case_line(d, 50) + "\n")
    assert line.startswith("error ps_search_opts: max_gap_extensions (aln -e) is 99, accepted: at most 15")


def test_score_table_past_the_buckets_is_refused_by_the_model(exe):
    """-M/-O/-E are bytes each; what they add up to under -n is make_model's check, with its own message"""
    line, = _lines(exe, ["models"], case_line(opts(M=40, O=60, E=30), 50) + "\n")
    assert line.startswith("error score range exceeds PS_MAX_BUCKETS") and "at most 128" in line


# ---- the two parts of a context's options ---------------------------------------------------------------------------------------
def test_search_part_survives_the_cost_part_in_either_order(exe):
    d = opts(o=2, e=5, i=7, d=20, l=24, k=1, m=1000, M=4, O=9, E=2, R=12, n=10)
    search = "2 5 0 7 20 1000 24 1 12 4 9 2 10"                        # max_gapo max_gape mode_gape -i -d -m -l -k -R -M -O -E n_occ
    a, b = _lines(exe, ["order"], case_line(d, 50, cost="3") + "\n")
    assert a == b == "3 -1 0 -1 | " + search
    a, b = _lines(exe, ["order"], case_line(d, 50, cost="2", profile=True) + "\n")
    assert a == b and a.endswith("| " + search) and a.split()[2:4] == ["1", "2"]
    # a -k that only stock costs can carry is refused under a profile, whichever part comes second
    a, b = _lines(exe, ["order"], case_line(opts(k=600), 50, cost="2", profile=True) + "\n")
    assert a.startswith("error") and b.startswith("error") and "max_seed_diff" in a and "511" in a and "max_seed_diff" in b and "511" in b


# ---- the shim's command lines ---------------------------------------------------------------------------------------------------
def test_shim_aln_parses_every_option(exe):
    out = _lines(exe, ["aln", "-t", "6", "-n", "0.02", "-o", "2", "-e", "5", "-i", "7", "-d", "20", "-l", "24", "-k", "1", "-m", "1000",
                       "-M", "4", "-O", "9", "-E", "2", "-R", "12", "-q", "0", "ref.fa", "reads.fq", "-f", "out.sai"])
    assert out == ["ok", "PSSAI2", "aln", "6", "0.02", "", "", "ref.fa", "reads.fq", "2 5 7 20 24 1 1000 4 9 2 12"]
    back, = _lines(exe, ["sai"], "\n".join(out[1:]) + "\n")
    assert back == "ok sub=aln threads=6 mm=0.02 ep= ip= ref=ref.fa fq=reads.fq search=2 5 7 20 24 1 1000 4 9 2 12 3"
    out = _lines(exe, ["parasuite", "-t", "2", "-X", "-1", "-p", "a.ep", "-g", "a.ip", "-l", "20", "ref.fa", "reads.fq", "-f", "out.sai"])
    assert out == ["ok", "PSSAI2", "parasuite", "2", "-1", "a.ep", "a.ip", "ref.fa", "reads.fq", "1 -1 5 10 20 2 2000000 3 11 4 30"]
    assert _lines(exe, ["aln", "ref.fa", "reads.fq", "-f", "o.sai"])[4] == "0.04"          # aln's default -n


def test_shim_reads_the_old_stub_with_defaults(exe):
    back, = _lines(exe, ["sai"], "PSSAI1\naln\n4\n2\n\n\nref.fa\nreads.fq\n")
    assert back == "ok sub=aln threads=4 mm=2 ep= ip= ref=ref.fa fq=reads.fq search=" + " ".join(str(DEFAULTS[f]) for f in FIELDS)
    assert _lines(exe, ["sai"], "BWASAI\n")[0].startswith("error [bwa samse] in.sai was not written by this bwa")
    assert _lines(exe, ["sai"], "PSSAI2\naln\n4\n2\n\n\nref.fa\nreads.fq\n1 2 x\n")[0].startswith("error [bwa samse] in.sai: the line of search options is damaged")


def test_shim_samse(exe):
    assert _lines(exe, ["samse", "-n", "10", "ref.fa", "a.sai", "r.fq", "-f", "o.sam"]) == ["ok out=o.sam n=10 have_n=1 pos=ref.fa|a.sai|r.fq"]
    assert _lines(exe, ["samse", "ref.fa", "a.sai", "r.fq", "-f", "o.sam"]) == ["ok out=o.sam n=3 have_n=0 pos=ref.fa|a.sai|r.fq"]
    assert _lines(exe, ["samse", "-r", "@RG\tID:x", "ref.fa", "a.sai", "r.fq", "-f", "o.sam"])[0].startswith("error [bwa samse] option -r is not supported")
    assert _lines(exe, ["samse", "-n", "ten", "ref.fa", "a.sai", "r.fq", "-f", "o.sam"])[0].startswith("error [bwa samse] option -n needs an integer")
    assert _lines(exe, ["samse", "ref.fa", "a.sai", "-f", "o.sam"])[0].startswith("error [bwa samse] need <ref> <in.sai> <reads> -f <out.sam>")


@pytest.mark.parametrize("args,named", [(["-q", "15"], "-q 15"), (["-N"], "-N"), (["-B", "6"], "-B"), (["-b"], "-b"), (["-0"], "-0"),
                                        (["-1"], "-1"), (["-2"], "-2"), (["-c"], "-c"), (["-I"], "-I"), (["-L"], "-L"), (["-Y"], "-Y"),
                                        (["-Z"], "unknown option -Z")], ids=lambda a: "".join(a) if isinstance(a, list) else None)
def test_shim_refuses_what_the_library_cannot_honour(exe, args, named):
    for cmd, extra in (("aln", []), ("parasuite", ["-p", "a.ep"])):
        out = _lines(exe, [cmd] + extra + args + ["ref.fa", "reads.fq", "-f", "o.sai"])
        assert len(out) == 1 and out[0].startswith("error [bwa %s] " % cmd) and named in out[0], out
    assert _lines(exe, ["aln", "-o", "two", "ref.fa", "reads.fq", "-f", "o.sai"])[0].startswith("error [bwa aln] option -o needs an integer")
    assert _lines(exe, ["aln", "ref.fa", "reads.fq", "-f", "o.sai", "-o"])[0].startswith("error [bwa aln] option -o needs a value")
