"""CPU tier: the oracle on the edge texts of tests/index_edges.py.

Its index (a host suffix sort of its own) against a plain sort of the suffixes -- seq_len, primary, L2, every BWT symbol, every
SA sample -- with a negative control of the comparison; then the edge reads of every text through both cost models: no error,
junction reads unmapped where the text has no repeat, and enough gapped CIGARs, XA:Z: tags and unmapped reads overall that the
inputs exercise what they are meant to.  The GPU tier (test_gpu_index_edges.py) holds the library against both references."""
import os

import numpy as np
import pytest

import index_edges as IE
from conftest import sam_records

MODES = ("stock", "profile")
_CACHE = {}


def _opt(mode):
    import orc
    if mode == "stock":
        return orc.stock_opt("0.04")
    return orc.profile_opt(IE.profile_matrix(), IE.INS_RATE, IE.DEL_RATE, IE.X_ARG)


def _built(name, workdir):
    """the text's FASTA, the oracle's index of it, the plain reference and the edge reads (made once)"""
    if name not in _CACHE:
        import orc
        text = IE.TEXT_BY_NAME[name]
        d = os.path.join(workdir, "edges_cpu")
        os.makedirs(d, exist_ok=True)
        fa = os.path.join(d, name + ".fa")
        text.write_fasta(fa)
        oix = orc.Index.from_fasta(fa)
        fwd = np.asarray(oix.forward_codes(), dtype=np.uint8) if text.has_n else IE.codes_of(text.ascii)
        IE.assert_pac_matches_fasta(IE.unpack_pac(oix.pac(), text.l_pac), text)
        fq = os.path.join(d, name + ".fq")
        with open(fq, "w") as f:
            f.write(IE.edge_reads(IE.string_of(fwd), seed=1000 + IE.NAMES.index(name)))
        _CACHE[name] = dict(text=text, fa=fa, oix=oix, plain=IE.plain_index(fwd), fq=fq, dir=d, sam={})
    return _CACHE[name]


def _mapped(name, mode, workdir):
    c = _built(name, workdir)
    if mode not in c["sam"]:
        out = os.path.join(c["dir"], "%s.%s.sam" % (name, mode))
        r = c["oix"].map_fastq(_opt(mode), c["fq"], out, n_threads=4)
        rec = sam_records(out)
        names = [l[1:].rstrip("\n") for l in open(c["fq"]).read().split("\n")[0::4] if l]
        assert r["n"] == len(names) == len(rec)
        assert [l.split("\t")[0] for l in rec] == names
        c["sam"][mode] = rec
    return c["sam"][mode]


@pytest.mark.parametrize("name", IE.NAMES)
def test_oracle_index_equals_plain_sort(name, workdir):
    c = _built(name, workdir)
    oix, plain = c["oix"], c["plain"]
    assert oix.l_pac == plain.l_pac == c["text"].l_pac
    IE.assert_index_equals_plain(plain, oix.seq_len, oix.primary, oix.L2, oix.bwt_syms(), oix.sa_samples())


def test_texts_sit_on_the_edges_they_are_meant_for(workdir):
    """the list itself: lengths on the layout's boundaries, primary at both extremes, long ties"""
    seq_lens = {2 * t.l_pac for t in IE.TEXTS}
    assert {26, 28, 30, 32, 192, 4032, 4094, 4096, 4098, 8192} <= seq_lens
    p = {n: _built(n, workdir)["plain"] for n in ("A300", "C96", "T300", "G97", "ACGT1024", "x_x", "x_rcx", "rand13")}
    assert p["A300"].primary == 1 and p["C96"].primary == 1
    assert p["T300"].primary == p["T300"].seq_len and p["G97"].primary == p["G97"].seq_len
    assert p["ACGT1024"].longest_repeat() == 8188 and p["ACGT1024"].min_sa_rounds() == 10
    assert p["x_x"].longest_repeat() >= 1500 and p["x_rcx"].longest_repeat() >= 3000
    assert p["rand13"].min_sa_rounds() == 1                   # shorter than the key: round 0 alone
    for sym, name in (("A", "A300"), ("C", "C96")):            # two symbols absent from T: two empty chunks
        L2 = p[name].L2
        assert sum(1 for c in range(4) if L2[c + 1] == L2[c]) == 2


def test_comparison_sees_a_damaged_index(workdir):
    """negative control: two neighbouring rows of the suffix array swapped, one BWT symbol changed"""
    plain = _built("rand2048", workdir)["plain"]
    ok = IE.PlainIndex(plain.fwd, plain.sa)
    IE.assert_index_equals_plain(plain, ok.seq_len, ok.primary, ok.L2, ok.bwt, ok.sa_samples())
    T = plain.T
    r = next(r for r in range(64, plain.seq_len, 32) if plain.sa[r] > 0 and plain.sa[r + 1] > 0
             and T[plain.sa[r] - 1] == T[plain.sa[r + 1] - 1])
    sa = plain.sa.copy()
    sa[r], sa[r + 1] = sa[r + 1], sa[r]                      # a sampled row, the same symbol in front of both: only the sample shows it
    bad = IE.PlainIndex(plain.fwd, sa)
    with pytest.raises(AssertionError, match="SA samples"):
        IE.assert_index_equals_plain(plain, bad.seq_len, bad.primary, bad.L2, bad.bwt, bad.sa_samples())
    r = next(r for r in range(70, plain.seq_len) if r % 32 not in (0, 31) and plain.sa[r] > 0 and plain.sa[r + 1] > 0
             and T[plain.sa[r] - 1] != T[plain.sa[r + 1] - 1])
    sa = plain.sa.copy()
    sa[r], sa[r + 1] = sa[r + 1], sa[r]                      # between samples: only the BWT shows it
    bad = IE.PlainIndex(plain.fwd, sa)
    with pytest.raises(AssertionError, match="BWT differs"):
        IE.assert_index_equals_plain(plain, bad.seq_len, bad.primary, bad.L2, bad.bwt, bad.sa_samples())
    bwt = plain.bwt.copy()
    bwt[1000] = (bwt[1000] + 1) & 3
    with pytest.raises(AssertionError, match="BWT differs"):
        IE.assert_index_equals_plain(plain, plain.seq_len, plain.primary, plain.L2, bwt, plain.sa_samples())
    with pytest.raises(AssertionError, match="primary"):
        IE.assert_index_equals_plain(plain, plain.seq_len, plain.primary + 1, plain.L2, plain.bwt, plain.sa_samples())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", IE.NAMES)
def test_oracle_maps_the_edge_reads(name, mode, workdir):
    rec = _mapped(name, mode, workdir)
    text = IE.TEXT_BY_NAME[name]
    exact = [l for l in rec if l.startswith(IE.JUNCTION_EXACT)]
    assert len(exact) >= 2
    assert any(l.startswith(IE.JUNCTION_SUB) for l in rec) == (text.l_pac >= 36)
    if text.kind == "random" and text.l_pac >= 48:           # no repeat: a junction read has nowhere else to go
        flags = [int(l.split("\t")[1]) for l in exact]
        assert flags == [4] * len(exact), [l.split("\t")[:4] for l in exact if int(l.split("\t")[1]) != 4]


def test_inputs_exercise_gaps_alternatives_and_unmapped_reads(workdir):
    tot = np.zeros(4, dtype=np.int64)
    per = {}
    for name in IE.NAMES:
        for mode in MODES:
            per[name, mode] = IE.sam_counts(_mapped(name, mode, workdir))
            tot += per[name, mode]
    mapped, unmapped, gapped, xa = tot.tolist()
    assert mapped > 2000 and unmapped > 100 and gapped > 50, tot
    for name in ("x_x", "x_rcx"):                               # every window has a second copy
        assert per[name, "stock"][3] >= 100, per[name, "stock"]
    assert xa > 400, tot
