"""ps_extract_read_names without a GPU: ExtractNotMappedReads.extractReads (ExtractNotMappedReads.java:33-88), the `extractAligned`
mode -- "@" + QNAME per record of a SAM or BAM file, in file order, whatever the flags; written through a temporary name."""
import os

import pytest

HEADER = "@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:c1\tLN:100\n@SQ\tSN:c2\tLN:50\n"
RECORDS = [("mapped", 0, "c1", 5, 37), ("rev/1", 16, "c2", 7, 20), ("unmapped", 4, "*", 0, 0), ("mapped", 256, "c2", 1, 0),
           ("bridging", 4, "c1", 95, 0), ("dup", 1024, "c1", 9, 3)]
NAMES = "".join("@%s\n" % r[0] for r in RECORDS)


def _sam(path, records=RECORDS):
    with open(path, "w") as f:
        f.write(HEADER)
        for name, flag, ref, pos, mapq in records:
            f.write("%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\tACGTA\tIIIII\n" % (name, flag, ref, pos, mapq, "*" if ref == "*" else "5M"))
    return str(path)


def test_names_of_sam_and_bam(tmp_path):
    import capi
    sam = _sam(tmp_path / "a.sam")
    st = capi.ps_extract_read_names(sam, str(tmp_path / "sam.names"))
    assert open(tmp_path / "sam.names").read() == NAMES
    assert st == dict(n_records=len(RECORDS), out_bytes=len(NAMES))
    bam = str(tmp_path / "a.bam")
    capi.ps_sam_to_bam(sam, bam, threads=2)
    assert capi.ps_extract_read_names(bam, str(tmp_path / "bam.names")) == st
    assert open(tmp_path / "bam.names").read() == NAMES
    assert sorted(os.listdir(tmp_path)) == ["a.bam", "a.sam", "bam.names", "sam.names"]     # no temporary is left


def test_header_only(tmp_path):
    import capi
    sam = _sam(tmp_path / "empty.sam", [])
    out = tmp_path / "empty.names"
    out.write_text("from an earlier run\n")
    assert capi.ps_extract_read_names(sam, str(out)) == dict(n_records=0, out_bytes=0)
    assert out.read_bytes() == b""


def test_refusals_leave_nothing(tmp_path):
    import capi
    sam = _sam(tmp_path / "a.sam")
    before = open(sam).read()
    with pytest.raises(capi.PsError, match="ps_extract_read_names: .*may not be the input file"):
        capi.ps_extract_read_names(sam, sam)
    os.symlink(sam, tmp_path / "link.sam")
    with pytest.raises(capi.PsError, match="may not be the input file"):
        capi.ps_extract_read_names(sam, str(tmp_path / "link.sam"))
    assert open(sam).read() == before
    with pytest.raises(capi.PsError, match="cannot open"):
        capi.ps_extract_read_names(str(tmp_path / "missing.bam"), str(tmp_path / "out.names"))
    bad = tmp_path / "bad.sam"
    bad.write_text(HEADER + "r1\t0\tc1\tnot-a-number\n")
    with pytest.raises(capi.PsError):
        capi.ps_extract_read_names(str(bad), str(tmp_path / "out.names"))
    assert sorted(os.listdir(tmp_path)) == ["a.sam", "bad.sam", "link.sam"]
    with pytest.raises(capi.PsError, match="required"):
        capi.ps_extract_read_names(sam, "")


def test_mirror(tmp_path):
    import __graft_entry__ as ge
    mod = ge.load_package()
    sam = _sam(tmp_path / "a.sam")
    st = mod.mapping.ExtractNotMappedReads().extractReads(sam, str(tmp_path / "n"))
    assert st["n_records"] == len(RECORDS) and open(tmp_path / "n").read() == NAMES
    with pytest.raises(mod.mapping.ExternalCallErrorException):
        mod.mapping.ExtractNotMappedReads().extractReads(str(tmp_path / "none.sam"), str(tmp_path / "n2"))
    assert not os.path.exists(tmp_path / "n2")
