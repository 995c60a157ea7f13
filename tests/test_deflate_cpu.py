"""The BGZF block encoder (csrc/ps_deflate.h) without a device.  tests/deflate_check.cpp is the host build of the header -- the lanes
of a block run one after the other -- built with AddressSanitizer and UBSan as a plain executable; what it writes is held to
Python's zlib: every member's payload is one raw DEFLATE stream that inflates to its block, CRC32, ISIZE and BSIZE are right and no
member is larger than its stored form.  And the switch as far as it goes without a device."""
import gzip
import os

import pytest

import bgzf_inputs as B

INPUTS = B.edge_inputs()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return B.build_check(tmp_path_factory.mktemp("deflate"), sanitize=True)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_members_inflate_and_the_chooser_holds(exe, tmp_path, name):
    """the three conditions per input; and by exact counting the default is never larger than fixed-only, stored-only or
    dynamic-only, block by block"""
    data = INPUTS[name]
    raw, blocks = B.host_members(exe, data, tmp_path)
    ms = B.check_members(raw, data)
    assert [B.btype(m) for m in ms] == [b[0] for b in blocks] and [len(m) - 26 for m in ms] == [b[1] for b in blocks]
    for mode, want_type in (("stored", 0), ("fixed", 1), ("dynamic", 2)):
        raw_m, blocks_m = B.host_members(exe, data, tmp_path, mode)
        ms_m = B.check_members(raw_m, data)
        for k, (m, mm) in enumerate(zip(ms, ms_m)):
            assert len(m) <= len(mm), (mode, k)
            assert B.btype(mm) in (want_type, 0), (mode, k)                 # stored stays the fallback of a block that would grow
            assert len(mm) <= len(data[k * B.BLK:(k + 1) * B.BLK]) + 5 + 26


def test_what_the_edges_are_for(exe, tmp_path):
    """the inputs do what they are in the list for"""
    run = lambda name: B.host_members(exe, INPUTS[name], tmp_path)[1]
    assert run("n0") == []
    n = B.BLK
    assert run("random_block")[0][:2] == (0, n + 5)                             # stored, n + 5 bytes (the member: n + 5 + 26)
    assert run("all256")[0][:2] == (0, 261) and run("all256")[0][3] == 0        # no match at all: no distance symbol was counted
    assert [b[0] for b in run("nib%d" % (n + 1))] == [2, 1]                     # a second block of one byte
    assert len(run("three_blocks_17")) == 4
    assert run("dist32768")[0][1] < n * 3 // 4                                  # the copy at exactly 32768 is used
    assert run("dist32769")[0][0] == 0                                          # the one at 32769 is not
    for name in ("rep257", "rep258", "rep259", "rep260"):
        assert run(name)[0][1] < 40, name
    assert run("rep%d" % n)[0][1] < 400                                         # matches of 258, chained
    for p in (2, 3, 4):
        assert run("period%d" % p)[0][1] < 200, p
    assert run("fib_shuffled")[0][0] == 2 and run("fib_runs")[0][0] == 2
    cl = run("runs_cl_depth8")[0]
    assert cl[0] == 2 and cl[4] > 7                                             # the code-length alphabet's plain tree is deeper than its limit
    two = run("two_values_64")[0]
    assert two[0] == 2 and two[3] == 0                                          # dynamic, and no distance symbol was counted


def test_host_path_through_the_library():
    """ps_bgzf_compress with device -1 is the library's own zlib path on the same cuts; it needs no device"""
    import capi
    data = INPUTS["nib%d" % (B.BLK + 1)]
    raw, st = capi.ps_bgzf_compress(data, -1)
    B.check_members(raw, data)
    assert (st["n_blocks"], st["in_bytes"], st["out_bytes"], st["kernel_ms"]) == (2, len(data), len(raw), 0.0) and len(raw) == B.zlib1_size(data)


def _lengths(exe, maxbits, freqs):
    import subprocess
    out = subprocess.check_output([exe, "lengths", str(maxbits)] + [str(f) for f in freqs], text=True).splitlines()
    return [int(x) for x in out[0].split()], int(out[1])


@pytest.mark.parametrize("maxbits, freqs", [(15, B.FIB), (7, B.FIB[:19]), (7, B.FIB[:12] + [0, 7]), (15, [5, 0, 0, 9]), (15, list(range(1, 287))),
                                             (15, [1] * 285 + [60000]), (7, [1] * 19), (15, [1, 1]), (15, [0, 3, 0]), (15, [0, 0, 0])])
def test_code_lengths_are_limited_and_complete(exe, maxbits, freqs):
    """the tree builder itself on chosen histograms.  The 7-bit limit is reached inside a real block (runs_cl_depth8).  The
    15-bit limit is not: on the Fibonacci bytes the frequent values are taken by matches and the literal tree that is left is
    13 to 15 deep (the third figure deflate_check prints), and among 18,800 seeded inputs of other kinds (runs of random
    values, snippets of 1 to 12 bytes from pools of 100 to 1000 bytes, unit strings with Fibonacci and geometric counts) the
    deepest literal/length tree was 15: one block holds at most 65,280 tokens, a tree 16 deep needs Fibonacci-like counts over
    17 symbols with every lighter symbol in place, and whatever the matcher leaves as literals flattens the bottom of it.
    Fibonacci counts over 22 symbols need 21 bits and over 19 symbols 18:
    every length is within the limit, the Kraft sum is exactly one (a complete code, which zlib's inflate insists on), a
    symbol never has a longer code than a rarer one, unused symbols get none; fewer than two used symbols get two one-bit
    codes"""
    lens, depth = _lengths(exe, maxbits, freqs)
    used = [k for k, f in enumerate(freqs) if f]
    if len(used) < 2:
        want = sorted(used + [1 if used == [0] else 0]) if used else [0, 1]
        assert [k for k, l in enumerate(lens) if l] == want and sum(lens) == 2
        return
    assert all(1 <= lens[k] <= maxbits for k in used) and all(lens[k] == 0 for k in range(len(freqs)) if k not in used)
    assert sum(2 ** (maxbits - lens[k]) for k in used) == 2 ** maxbits
    for a in used:
        for b in used:
            assert not (freqs[a] < freqs[b] and lens[a] < lens[b]), (a, b)
    if freqs == B.FIB:
        assert depth == 21 and max(lens) == 15
    if freqs == B.FIB[:19]:
        assert depth == 18 and max(lens) == 7


def test_exported_and_in_the_binding():
    import capi
    lib = capi.lib()
    for name in ("ps_bgzf_device", "ps_bgzf_compress"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and name in capi.EXPORTS
    assert capi.STRUCTS["ps_bgzf_stats"] is capi.BgzfStats and capi.BgzfStats.struct_size.offset == 0


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_without_a_device_the_switch_fails_and_zlib_goes_on(tmp_path):
    import capi
    from test_rec_table_cpu import RECORDS, sam_text
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_bgzf_device(0)
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.ps_bgzf_compress(b"abc", 0)
    capi.ps_bgzf_device(-1)
    sam, bam = str(tmp_path / "a.sam"), str(tmp_path / "a.bam")
    with open(sam, "w") as f:
        f.write(sam_text(RECORDS))
    assert capi.ps_sam_to_bam(sam, bam, threads=2)["n_out"] == len(RECORDS)
    raw = open(bam, "rb").read()
    assert gzip.decompress(raw)[:4] == b"BAM\x01" and raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    assert os.path.getsize(bam) == len(raw)
