"""ps_error_profile_full and ps_error_profile on the seams of their own layout: the inputs of tests/profile_seams.py (what
each one reaches is shown in tests/test_profile_seams_cpu.py), all six files and the stats byte for byte equal to the
plain-Python restatement tests/java_errorprofile.py."""
import os

import pytest

import java_errorprofile as J
import profile_seams as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def seams(workdir):
    import capi
    d = os.path.join(workdir, "ep_seams")
    os.makedirs(d, exist_ok=True)
    fa = os.path.join(d, "r.fa")
    open(fa, "w").write(P.FA)
    capi.ps_index(fa)
    assert J.read_fasta(fa) == P.REF
    return d, fa


def _read(prefix):
    return {k: open(prefix + k, "rb").read() for k in J.FILES}


def _full(seams, name, recs, max_len, infer_q):
    import capi
    d, fa = seams
    text = P.sam_text(recs)
    sam = os.path.join(d, name + ".sam")
    open(sam, "w").write(text)
    exp, est = J.infer(text, P.REF, max_len, infer_q)
    st = capi.ps_error_profile_full(sam, fa, max_len, os.path.join(d, name), infer_q)
    got = _read(os.path.join(d, name))
    for k in J.FILES:
        assert got[k] == exp[k], (name, k, got[k][:1500], exp[k][:1500])
    assert st == est
    return st


# ---- B1

@pytest.mark.parametrize("max_len", P.B1_MAX)
@pytest.mark.parametrize("n", P.B1_N)
def test_b1_chunk_and_block_seams(seams, n, max_len):
    _full(seams, "b1_%d_%d" % (n, max_len), P.b1_records(n, max_len), max_len, True)


def test_b1_first_chunk_books_nothing(seams):
    n, max_len, lead = P.B1_LEAD
    st = _full(seams, "b1_lead", P.b1_records(n, max_len, lead), max_len, True)
    assert st["n_unmapped"] >= lead


# ---- B2

def test_b2_second_grid_pass(seams):
    """524,289 records: lane 0 of block 0 takes a second record.  Expected from the counts of the block and the prefix."""
    import capi
    d, fa = seams
    sam = os.path.join(d, "b2.sam")
    open(sam, "w").write(P.b2_text())
    exp, est = P.b2_expected()
    st = capi.ps_error_profile_full(sam, fa, P.B2_MAX, os.path.join(d, "b2"), False)
    got = _read(os.path.join(d, "b2"))
    for k in J.FILES:
        assert got[k] == exp[k], (k, got[k][:1500], exp[k][:1500])
    assert st == est and st["n_records"] == 2048 * 256 + 1


# ---- B3

@pytest.mark.parametrize("infer_q", [True, False], ids=["q", "noq"])
def test_b3_full_limits(seams, infer_q):
    """the largest max_read_len the header states asks for the whole 160 KiB of LDS; one more is refused by the range check"""
    import capi
    d, fa = seams
    m = P.B3_LIMITS[2 if infer_q else 1]
    _full(seams, "b3_%d" % m, P.b3_records(m), m, infer_q)
    sam = os.path.join(d, "b3_%d.sam" % m)
    with pytest.raises(capi.PsError, match=r"maximum read length out of range.*1\.\.%d\)" % m):
        capi.ps_error_profile_full(sam, fa, m + 1, os.path.join(d, "b3_over_%d" % m), infer_q)
    assert not [f for f in os.listdir(d) if f.startswith("b3_over_%d" % m)]


def test_b3_plain_limit(seams):
    """ps_error_profile: 2,275 is the largest length its kernel's LDS holds, and 2,276 fails as out of range, not on LDS bytes"""
    import capi
    d, fa = seams
    m = P.B3_LIMITS[0]
    text = P.sam_text(P.b3_records(m))
    sam = os.path.join(d, "b3_plain.sam")
    open(sam, "w").write(text)
    exp, _ = J.infer(text, P.REF, m, False)
    capi.ps_error_profile(sam, fa, m, os.path.join(d, "b3_plain"))
    for k in (".errorprofile", ".indelprofile"):
        assert open(os.path.join(d, "b3_plain" + k), "rb").read() == exp[k], k
    for over in (m + 1, 4096, 4097, 0):
        with pytest.raises(capi.PsError, match=r"maximum read length out of range \(1\.\.2275\)"):
            capi.ps_error_profile(sam, fa, over, os.path.join(d, "b3_plain_over"))
    assert not [f for f in os.listdir(d) if f.startswith("b3_plain_over")]
