"""The inputs of tests/profile_seams.py have the properties their names claim, shown with the plain restatement
tests/java_errorprofile.py alone; tests/test_gpu_profile_seams.py then holds ps_error_profile_full to the restatement's
bytes on the same inputs.  224 = records per staged chunk of k_qual_sd, 64 = read positions per block (the constants are
read from the source in tests/test_cluster_seams_cpu.py::test_kernel_constants)."""
import pytest

import java_errorprofile as J
import profile_seams as P


def _qualities(recs, max_len):
    return J.infer(P.sam_text(recs), P.REF, max_len, True)[0][".qualities"].split(b"\n")[:-1]


@pytest.mark.parametrize("max_len", P.B1_MAX)
@pytest.mark.parametrize("n", P.B1_N)
def test_b1_file_order_shows_in_the_qualities(n, max_len):
    recs = P.b1_records(n, max_len)
    assert len(recs) == n and max(len(r[5]) for r in recs) <= max_len
    fwd = _qualities(recs, max_len)
    assert len(fwd) == max_len
    if n == 1:
        assert recs[0][1] != 4 and fwd[0] != b"NaN\tNaN"
        return
    assert min(n % 224, 224 - n % 224) <= 1                                   # one below, on, or one above a chunk boundary
    assert max(len(r[5]) for r in recs) == max_len and any(len(r[5]) in (63, 64, 65) for r in recs)
    assert sum(1 for r in recs if r[1] == 4) == n // 40 and sum(1 for r in recs if r[6] == "*") == n // 50
    assert {r[1] for r in recs} == {0, 4, 16}
    # a kernel that adds a chunk, or the records within one, in another order cannot pass: reversed, at least a third of the lines differ
    rev = _qualities(recs[::-1], max_len)
    differ = sum(1 for a, b in zip(fwd, rev) if a != b)
    assert [a.split(b"\t")[0] for a in fwd] == [b.split(b"\t")[0] for b in rev]          # the means are exact
    assert 3 * differ >= max_len, (differ, max_len)


def test_b1_first_chunk_books_nothing():
    n, max_len, lead = P.B1_LEAD
    recs = P.b1_records(n, max_len, lead)
    assert lead == 224 and all(r[1] == 4 for r in recs[:lead]) and recs[lead][1] != 4
    files, st = J.infer(P.sam_text(recs), P.REF, max_len, True)
    assert st["n_unmapped"] >= lead and st["n_counted"] >= 70
    rev = _qualities(recs[::-1], max_len)
    assert 3 * sum(1 for a, b in zip(files[".qualities"].split(b"\n")[:-1], rev) if a != b) >= max_len


def test_b2_counts_add_up():
    """the 524,289 records are 524 copies of a block and a prefix: their counts are sums, shown here for 3 copies"""
    assert P.B2_N == 2048 * 256 + 1 == 524289 and divmod(P.B2_N, P.B2_BLOCK) == (524, 289)
    block = P.b2_block()
    cigs = {(r[4], r[1]) for r in block}
    assert {("4M", 0), ("4M", 16), ("2M1I1M", 0), ("2M1I1M", 16), ("2M1D2M", 0), ("2M1D2M", 16), ("*", 4)} <= cigs
    whole = P.sam_text(block[:289] + block * 3)
    total = P.add_counts(J.counts(P.sam_text(block), P.REF, P.B2_MAX, False), 3, J.counts(P.sam_text(block[:289]), P.REF, P.B2_MAX, False))
    exp, est = J.infer(whole, P.REF, P.B2_MAX, False)
    assert J.render(total, P.B2_MAX, False) == exp and total["st"] == est
    assert sum(total["ins"]) > 0 and sum(total["dele"]) > 0 and est["n_without_qual"] > 0 and est["n_unmapped"] > 0
    files, st = P.b2_expected()
    assert st["n_records"] == P.B2_N and files[".qualities"] == b"" and b"NaN" not in files[".errorprofile"]
    assert files[".indelprofile"] != b"0.0\t0.0"


def test_b3_mapper_entries_share_the_plain_limit(tmp_path):
    """ps_map_profiled and the route count with ps_error_profile's kernel: 2,276 is out of range before anything is opened"""
    import capi
    names = [str(tmp_path / n) for n in ("g.fa", "r.fq", "out.sam", "prof", "route")]
    with pytest.raises(capi.PsError, match=r"maximum read length out of range \(1\.\.2275\)"):
        capi.ps_map_profiled(1, "2", None, None, names[0], names[1], names[2], 10, 2276, names[3])
    with pytest.raises(capi.PsError, match=r"maximum read length out of range \(1\.\.2275\)"):
        capi.ps_map_route(names[1], names[0], names[4], refine=True, max_read_len=2276)
    assert list(tmp_path.iterdir()) == []


def test_b3_limits_follow_from_the_lds():
    """160 KiB of LDS per workgroup, 4-byte words: 18 per read position for the two files of ps_error_profile, 18 and 1.5 KiB
    for the .qualityPerMismatch sums without -q, 20 and 1.5 KiB with -q"""
    lds, qpm = 160 * 1024, 8 * 16 * 12
    assert P.B3_LIMITS == {0: lds // (18 * 4), 1: (lds - qpm) // (18 * 4), 2: (lds - qpm) // (20 * 4)} == {0: 2275, 1: 2254, 2: 2028}
    for q, m in P.B3_LIMITS.items():
        recs = P.b3_records(m)
        assert max(len(r[5]) for r in recs) == m and all(r[3] - 1 + len(r[5]) <= 2300 for r in recs)
        files, st = J.infer(P.sam_text(recs), P.REF, m, q == 2)
        assert st["n_counted"] == 6 and st["n_without_qual"] == 1
        assert len(files[".indels"].split(b"\n")) == m + 1
        if q == 2:
            assert files[".qualities"].split(b"\n")[m - 1] != b"NaN\tNaN"     # the last position is booked
        with pytest.raises(ValueError):
            J.infer(P.sam_text(recs), P.REF, m - 1, False)
