"""CPU tier of the one way the modes publish their output files (csrc/ps_outfiles.h).

* OutFiles and the three file helpers beside it are driven by tests/outfiles_check.cpp in a directory of its own -- a plain
  executable built here with the host compiler, AddressSanitizer and UBSan; it checks itself and prints one `ok` line per part.
* Through the library, which loads without a GPU: the host-only modes (the BAM tools, ps_extract_weak_reads) publish whole files,
  leave no temporary, refuse an output that is their input and leave a file from before a failed call as it was."""
import os
import subprocess

import pytest

from test_capi_cpu import ROOT

CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
SAM = ("@SQ\tSN:chr1\tLN:1000\n"
       "r1\t0\tchr1\t10\t30\t4M\t*\t0\t0\tACGT\tIIII\n"
       "r2\t16\tchr1\t5\t3\t4M\t*\t0\t0\tACGA\tIHGF\n")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("outfiles") / "outfiles_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g",
                           "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "outfiles_check.cpp"), "-o", out])
    return out


def test_the_header_needs_no_hip():
    text = open(os.path.join(CSRC, "ps_outfiles.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and not any("hip/" in i for i in includes), includes
    assert [i for i in includes if i.startswith('"')] == ['"ps_error.h"']


@pytest.mark.parametrize("part", ["success", "no_keep", "rename_fails", "preexisting", "unopenable", "paths", "refuse_inputs", "text_file"])
def test_part(exe, tmp_path, part):
    """success: written and published in order, the finals hold the bytes, no temporary is left.  no_keep: the destructor leaves the
    directory as it was, after zero publishes and after some.  rename_fails: a final that is a directory (step by step, and all
    together) and a temporary that is gone in the middle: earlier finals and all temporaries are gone, the directory stands.
    preexisting: a final from before the call that was never replaced is untouched.  unopenable: the error names the path.
    paths: every final and temporary, the explicit-temporary form too.  refuse_inputs: the same path, a hard link, a symlink, an
    input equal to a temporary name -- and the refusal removes none of them.  text_file: write_text_file removes nothing."""
    r = subprocess.run([exe, part, str(tmp_path)], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == ["ok " + part], r.stdout


# ---- through the library --------------------------------------------------------------------------------------------------------
def _listing(d):
    return sorted((p, open(os.path.join(d, p), "rb").read()) for p in os.listdir(d))


def test_host_modes_publish_whole_files_and_leave_no_temporary(tmp_path):
    import capi
    d = str(tmp_path)
    sam, bam, srt, view, kept, weak = (os.path.join(d, n) for n in ("m.sam", "m.bam", "s.bam", "v.bam", "k.bam", "w.fq"))
    open(sam, "w").write(SAM)
    capi.ps_sam_to_bam(sam, bam)
    capi.ps_sam_to_bam(sam, srt, sort_by_coordinate=True, write_index=True)
    capi.ps_bam_view(bam, view, 10)
    capi.ps_bam_sort(bam, os.path.join(d, "n.bam"), by_name=True)
    os.remove(srt + ".bai")
    capi.ps_bam_index(srt)
    capi.ps_extract_weak_reads(bam, kept, weak, 10)
    assert sorted(os.listdir(d)) == ["k.bam", "m.bam", "m.sam", "n.bam", "s.bam", "s.bam.bai", "v.bam", "w.fq"]
    assert open(weak).read() == "@r2\nTCGT\n+\nFGHI\n"
    first = _listing(d)
    capi.ps_sam_to_bam(sam, srt, sort_by_coordinate=True, write_index=True)      # over the files of the first round: the same bytes
    capi.ps_bam_index(srt)
    capi.ps_extract_weak_reads(bam, kept, weak, 10)
    assert _listing(d) == first


def test_host_modes_refuse_an_output_that_is_their_input(tmp_path):
    import capi
    d = str(tmp_path)
    sam, bam = os.path.join(d, "m.sam"), os.path.join(d, "m.bam")
    open(sam, "w").write(SAM)
    capi.ps_sam_to_bam(sam, bam, sort_by_coordinate=True)
    os.link(sam, os.path.join(d, "o.bam.bam-tmp"))                                # the temporary name of o.bam IS the SAM
    os.link(bam, os.path.join(d, "x.bam.bai.bam-tmp"))
    os.symlink("m.bam", os.path.join(d, "x.bam"))
    before = _listing(d)
    for call, who in ((lambda: capi.ps_sam_to_bam(sam, sam), "ps_sam_to_bam"), (lambda: capi.ps_sam_to_bam(sam, os.path.join(d, "o.bam")), "ps_sam_to_bam"),
                      (lambda: capi.ps_bam_view(bam, bam, 0), "ps_bam_view"), (lambda: capi.ps_bam_sort(bam, os.path.join(d, "x.bam")), "ps_bam_sort"),
                      (lambda: capi.ps_bam_index(os.path.join(d, "x.bam")), "ps_bam_index"),
                      (lambda: capi.ps_extract_weak_reads(bam, os.path.join(d, "k.bam"), bam, 10), "ps_extract_weak_reads")):
        with pytest.raises(capi.PsError, match=who + ": the output .* the input"):
            call()
        assert _listing(d) == before


def test_a_failed_host_call_leaves_files_from_before_it(tmp_path):
    import capi
    d = str(tmp_path)
    sam, kept, weak, out = (os.path.join(d, n) for n in ("m.sam", "k.bam", "w.fq", "o.bam"))
    open(sam, "w").write(SAM.replace("IHGF", "*"))                                # the weak record has no QUAL
    for p in (kept, weak, out):
        open(p, "w").write("from before " + p)
    os.mkdir(out + ".bai")                                                        # the index cannot be published
    before = _listing_with_dirs(d)
    with pytest.raises(capi.PsError, match="r2 has MAPQ below 10 and no QUAL"):
        capi.ps_extract_weak_reads(sam, kept, weak, 10)
    with pytest.raises(capi.PsError, match="cannot rename"):
        capi.ps_sam_to_bam(sam, out, sort_by_coordinate=True, write_index=True)
    with pytest.raises(capi.PsError, match="cannot open"):
        capi.ps_bam_sort(os.path.join(d, "absent.bam"), out)
    assert _listing_with_dirs(d) == before


def _listing_with_dirs(d):
    return sorted((p, None if os.path.isdir(os.path.join(d, p)) else open(os.path.join(d, p), "rb").read()) for p in os.listdir(d))
