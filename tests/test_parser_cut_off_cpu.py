"""A FASTQ input cut off behind the '+' line of its last record fails the call (csrc/ps_reads.cpp: refuse_cut_off_fastq) instead
of getting qualities made up for that record; every other end of an input is parsed as it was.  Host only, through ps_parse_check,
for the whole-file parse and the streamed one."""
import pytest

import capi

WHOLE = "@a\nACGT\n+\nIIII\n"


@pytest.mark.parametrize("tail", ["@b x\nACGTA\n+\n", "@b x\nACGTA\n+", "@b x\nACGTA\r\n+\r\n\n", "@b x\nACGTA\n+b x\n"],
                         ids=["newline", "no_newline", "crlf_and_blank", "named_plus"])
@pytest.mark.parametrize("window", [0, 4096])
def test_cut_off_after_the_plus_line_is_refused(tmp_path, tail, window):
    p = str(tmp_path / "cut.fq")
    open(p, "w", newline="").write(WHOLE * 3 + tail)
    with pytest.raises(capi.PsError, match=r"cut\.fq: the last FASTQ record \(b\) is cut off after its '\+' line: it has no quality line"):
        capi.ps_parse_check(p, 2, window)


@pytest.mark.parametrize("text,reads,bases", [
    (WHOLE * 3, 3, 12),
    (WHOLE * 3 + "@b\nA\n+\n+\n", 4, 13),                   # a one-base read whose quality is '+'
    (WHOLE * 3 + "@b\nACGTA\n+b\n+IIII", 4, 17),            # a quality line that starts with '+', no newline at the end
    (WHOLE * 3 + "@b\nACGTA\n", 4, 17),                     # ends before any '+' line: as before
    (">a\nACGT\n>b\nACGTA\n", 2, 9),                        # FASTA is not looked at
], ids=["whole", "plus_quality", "plus_first_quality", "no_plus_line", "fasta"])
@pytest.mark.parametrize("window", [0, 4096])
def test_other_ends_parse_as_before(tmp_path, text, reads, bases, window):
    p = str(tmp_path / "ok.fq")
    open(p, "w").write(text)
    assert capi.ps_parse_check(p, 2, window)[:2] == (reads, bases)
