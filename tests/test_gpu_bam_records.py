"""The mapper's BAM records built on the device (csrc/ps_bamrec.hip: ps_bam_records_device, PS_BAM_RECORDS_GPU, ps_batch_bam_records).
The host route (ps_records.hip: bam_record) is the oracle throughout: the device route's bytes are its bytes, record for record; the
sorted files and their .bai are the same files, the unsorted ones inflate to the same stream."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 21
LUT = np.frombuffer(b"ACGTN", dtype=np.uint8)


def _profile():
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    return P


def _write_fastq(path, sim, n, names=None):
    with open(path, "wb") as f:
        for i in range(n):
            L = int(sim["lens"][i])
            name = names[i] if names else b"r%d" % i
            f.write(b"@" + name + b"\n" + LUT[np.minimum(sim["codes"][i, :L], 4)].tobytes() + b"\n+\n" + sim["quals"][i, :L].tobytes() + b"\n")


def _records(data):
    """the records of a byte stream: dicts of flag, n_cigar ops, the bases and the raw tag bytes"""
    out, at = [], 0
    while at < len(data):
        bs, ref, pos, l_name, mapq, _, n_cig, flag, l_seq = struct.unpack_from("<iiiBBHHHi", data, at)
        p = at + 36 + l_name
        cig = struct.unpack_from("<%dI" % n_cig, data, p)
        p += 4 * n_cig
        nib = data[p:p + (l_seq + 1) // 2]
        tags = data[p + (l_seq + 1) // 2 + l_seq:at + 4 + bs]
        out.append(dict(flag=flag, ref=ref, pos=pos, mapq=mapq, ops="".join("MIDNS"[c & 15] for c in cig), l_seq=l_seq, tags=bytes(tags),
                        has_n=any(((nib[i >> 1] >> (0 if i & 1 else 4)) & 15) == 15 for i in range(l_seq))))
        at += 4 + bs
    assert at == len(data)
    return out


def _block_sizes(data):
    out, at = [], 0
    while at < len(data):
        out.append(struct.unpack_from("<i", data, at)[0])
        at += 4 + out[-1]
    return out


def _both(batch, q, threads=8):
    """(device bytes, origin, device stats, host bytes, host stats) of a located batch"""
    dev, origin, st = batch.bam_records(q, True, threads)
    host, _, st_h = batch.bam_records(q, False, threads)
    return dev, origin, st, host, st_h


@pytest.fixture(scope="module")
def ex(example, workdir):
    """the example genome's context (the profile options of smoke()) and 2,000 simulated 50 bp reads"""
    import capi
    import simulate as S
    d = os.path.join(workdir, "bamrec")
    os.makedirs(d)
    ctx = capi.Ctx.build(example["fa"], device=0)
    ctx.set_profile(_profile(), 2.1e-5, 5.9e-4, -1)
    sim = S.simulate_reads(example["genome"], 2000, 50, seed=SEED, indel_scale=30, n_frac=0.002)
    return dict(ctx=ctx, sim=sim, dir=d)


def _located(ctx, path):
    b = ctx.batch_from_fastq(path)
    b.run(8)
    return b


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2000])
def test_staged_batches(ex, n):
    """batches around the 64 reads of one wave of the fill kernel: the device route's bytes are the host route's at every filter"""
    fq = os.path.join(ex["dir"], "n%d.fq" % n)
    _write_fastq(fq, ex["sim"], n)
    b = _located(ex["ctx"], fq)
    assert b.n == n
    for q in (0, 10, 255):
        dev, origin, st, host, st_h = _both(b, q)
        assert dev == host, (n, q, len(dev), len(host), next((i for i in range(min(len(dev), len(host))) if dev[i] != host[i]), None))
        assert st["n_records"] == st_h["n_records"] == len(origin) and st["bytes"] == len(dev) and st["n_reads"] == n
        assert st["n_device"] + st["n_host"] == st["n_records"]
        if q == 255:
            assert dev == b"" and st["n_records"] == 0
        if q == 0:
            assert st["n_records"] == n
    if n == 2000:
        dev, origin, st, _, _ = _both(b, 0)
        recs = _records(dev)
        assert len(recs) == 2000 == len(origin) and st["n_device"] > 0 and st["n_host"] > 0 and set(origin.tolist()) == {0, 1}
        built = [r for r, o in zip(recs, origin) if o == 0]
        cats = dict(forward=lambda r: not r["flag"] & 20, reverse=lambda r: r["flag"] & 16 and not r["flag"] & 4, unmapped=lambda r: r["flag"] & 4 and r["ref"] < 0,
                    gapped=lambda r: "I" in r["ops"] or "D" in r["ops"], with_n=lambda r: r["has_n"] and not r["flag"] & 4)
        count = {k: sum(1 for r in built if f(r)) for k, f in cats.items()}
        print("device-built records by category:", count, "host-built:", st["n_host"])
        assert all(count.values()), count
        assert all(b"XAZ" not in r["tags"] for r in built)                      # alternative hits are the host's
    b.free()


def test_capacity(ex):
    """one byte short is refused with both numbers and dst untouched; the exact capacity is taken"""
    import capi
    fq = os.path.join(ex["dir"], "n65.fq")
    _write_fastq(fq, ex["sim"], 65)
    b = _located(ex["ctx"], fq)
    want, _, _ = b.bam_records(0, False)
    n = len(want)
    for on_device in (1, 0):
        dst = C.create_string_buffer(b"\xee" * n, n)
        assert capi.lib().ps_batch_bam_records(b.h, 0, on_device, 4, None, 0, None, None) == n
        assert capi.lib().ps_batch_bam_records(b.h, 0, on_device, 4, dst, n - 1, None, None) == -1
        err = capi.lib().ps_last_error()
        assert str(n).encode() in err and str(n - 1).encode() in err and dst.raw == b"\xee" * n
        assert capi.lib().ps_batch_bam_records(b.h, 0, on_device, 4, dst, n, None, None) == n and dst.raw == want
    b.free()


def test_multi_contig_edges(multi, workdir):
    """three contigs, FASTA reads (QUAL 0xff), reads across the end of chrA (flag 4, position kept) and reads that reach into the
    hole of chrA at 9000-9400"""
    import capi
    import simulate as S
    from test_gpu_map_to_bam import _multi_fasta_reads
    reads = os.path.join(workdir, "bamrec_multi.fa")
    assert _multi_fasta_reads(multi, reads) == 60
    a = S.contig_codes(multi["genome"][0][1])
    with open(reads, "ab") as f:
        for k, (x0, x1) in enumerate([(8958, 9001), (8955, 9002), (9399, 9445), (9398, 9440), (8960, 9000), (9400, 9440)]):
            f.write(b">hole%d\n" % k + LUT[np.minimum(a[x0:x1], 4)].tobytes() + b"\n")
    ctx = capi.Ctx.build(multi["fa"], device=0)
    ctx.set_profile(_profile(), 2.1e-5, 5.9e-4, -1)
    b = _located(ctx, reads)
    for q in (0, 10):
        dev, origin, st, host, _ = _both(b, q)
        assert dev == host, q
        recs = _records(dev)
        built = [r for r, o in zip(recs, origin) if o == 0]
        assert any(r["flag"] & 4 and r["ref"] >= 0 and r["pos"] >= 0 for r in built)               # bridging, device-built
        assert len({r["ref"] for r in built}) == (4 if q == 0 else 3)
        print("multi q%d: %d records, %d device-built, %d of them with XN" % (q, len(recs), len(built), sum(b"XNC" in r["tags"] for r in built)))
        assert any(b"XNC" in r["tags"] for r in built)                                             # a span with hole bases
    b.free()
    ctx.close()


def test_two_byte_x0_on_a_periodic_text(workdir):
    """(AC)^1024 of tests/index_edges.py: a read of 25 units has one best interval of about a thousand rows, and X0 takes the
    two-byte type in a record the device builds"""
    import capi
    import index_edges as E
    d = os.path.join(workdir, "bamrec_ac")
    os.makedirs(d)
    fa, fq = os.path.join(d, "ac.fa"), os.path.join(d, "ac.fq")
    E.TEXT_BY_NAME["AC1024"].write_fasta(fa)
    with open(fq, "w") as f:
        for i, read in enumerate(["AC" * 25, "CA" * 20, "AC" * 12 + "A", "GT" * 25, "ACGTTGCATTGACCATGACCATGGTACCATTGA"]):
            f.write("@p%d\n%s\n+\n%s\n" % (i, read, "I" * len(read)))
    ctx = capi.Ctx.build(fa, device=0)
    ctx.set_stock("2")
    b = _located(ctx, fq)
    dev, origin, st, host, _ = _both(b, 0)
    assert dev == host
    recs = _records(dev)
    wide = [r for r, o in zip(recs, origin) if o == 0 and b"X0S" in r["tags"]]
    print("periodic text: origins", origin.tolist(), "records with a two-byte X0:", len(wide))
    assert wide and all(struct.unpack_from("<H", r["tags"], r["tags"].index(b"X0S") + 3)[0] >= 256 for r in wide)
    b.free()
    ctx.close()


def _tandem_genome(rng, n_sites=160, gap=300):
    """random text with a tandem repeat every 300 bases: a unit of 1 to 6 bases (1: a homopolymer), 8 to 20 copies; -> (ASCII, [(start, unit length, copies)])"""
    parts, sites, at = [], [], 0
    for _ in range(n_sites):
        flank = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, gap))
        u = int(rng.integers(1, 7))
        unit = "".join("ACGT"[int(c)] for c in rng.integers(0, 4, u))
        copies = int(rng.integers(8, 21))
        parts += [flank, unit * copies]
        sites.append((at + gap, u, copies))
        at += gap + u * copies
    parts.append("".join("ACGT"[int(c)] for c in rng.integers(0, 4, gap)))
    return "".join(parts), sites


@pytest.mark.parametrize("forced", [False, True])
def test_hits_that_the_locate_stage_patched_on_the_host(workdir, monkeypatch, forced):
    """batch_locate cleans a gapped hit's CIGAR on the host and patches the host copy of the hit alone: a leading deletion is dropped
    and moves the position forward, an empty CIGAR makes the read unmapped.  The device route has to build from the patched values.
    Reads that start in or just before a homopolymer or a tandem repeat and have lost or gained a unit of it (some a second unit
    further on), either strand, searched with gaps allowed up to the read's ends and two gap opens: the alignment of such a read is
    not unique, and where the banded alignment puts its deletion is its own choice.  Bytes equal to the host route's.
    Measured: none of the 835 device-built gapped hits of these reads had its position patched (the banded alignment runs on exactly
    the window the search found, and an alignment that starts with a deletion there means an exact hit further on, which the search
    prefers).  So `forced` makes the clean-up do its two patches (PS_LOCATE_PATCH_TEST: position moved with the first base clipped;
    CIGAR emptied) on the gapped hits themselves, and the records of both kinds must still be the host route's."""
    import capi
    rng = np.random.default_rng(0x7A4D)
    text, sites = _tandem_genome(rng)
    d = os.path.join(workdir, "bamrec_tandem%d" % forced)
    os.makedirs(d)
    if forced:
        monkeypatch.setenv("PS_LOCATE_PATCH_TEST", "1")
    fa, fq = os.path.join(d, "t.fa"), os.path.join(d, "t.fq")
    with open(fa, "w") as f:
        f.write(">tandem\n" + "\n".join(text[i:i + 60] for i in range(0, len(text), 60)) + "\n")
    comp = str.maketrans("ACGT", "TGCA")
    n = 0
    with open(fq, "w") as f:
        for start, u, copies in sites:
            for lead in (0, 1, 2, 3, 5, 7, 9, 12):                              # bases of the read in front of the repeat (0: it starts with it)
                for k in range(4):
                    x0 = start - lead + (int(rng.integers(0, u * 3)) if lead == 0 else 0)
                    window = text[x0:x0 + 70]
                    cut = max(0, start - x0) + u * int(rng.integers(0, 3))         # where a unit goes or comes: at the repeat's start or a few units in
                    read = window[:cut] + window[cut + u:] if k & 1 else window[:cut] + window[cut:cut + u] + window[cut:]
                    if k & 2:                                                      # a second change of one unit, further on
                        c2 = cut + u * int(rng.integers(2, 5))
                        read = read[:c2] + read[c2 + u:]
                    read = read[:50]
                    if (n >> 2) & 1:
                        read = read.translate(comp)[::-1]
                    f.write("@t%d\n%s\n+\n%s\n" % (n, read, "I" * len(read)))
                    n += 1
    ctx = capi.Ctx.build(fa, device=0)
    ctx.set_stock("4")
    ctx.set_search(max_gap_opens=2, indel_end_skip=0)
    b = _located(ctx, fq)
    hits = b.hits()
    for q in (0, 10):
        dev, origin, st, host, _ = _both(b, q)
        bad = next((i for i in range(min(len(dev), len(host))) if dev[i] != host[i]), None)
        assert dev == host, (q, len(dev), len(host), bad)
    dev, origin, st, _, _ = _both(b, 0)
    on_ref = np.array([sum(int(c) >> 4 for c in h["cigar"][:h["n_cigar"]] if (int(c) & 15) in (0, 2)) for h in hits])
    lens = np.array([r["l_seq"] for r in _records(dev)])
    gapped = (hits["n_cigar"] > 0) & (origin == 0)
    shortened = gapped & (on_ref < lens + hits["ref_shift"])                       # a deletion at one end of the alignment was dropped
    emptied = (origin == 0) & (hits["type"] == 0) & (hits["n_gapo"] > 0)
    print("tandem reads: %d, device-built %d, of them gapped %d, with a deletion dropped at an end %d, with an emptied CIGAR %d"
          % (n, int((origin == 0).sum()), int(gapped.sum()), int(shortened.sum()), int(emptied.sum())))
    assert gapped.sum() > 100
    if forced:
        clipped = gapped & np.array([h["n_cigar"] > 0 and (int(h["cigar"][0]) & 15) == 3 and int(h["cigar"][0]) >> 4 == 1 for h in hits])
        print("forced: position moved on %d device-built hits, CIGAR emptied on %d" % (int(clipped.sum()), int(emptied.sum())))
        assert clipped.sum() > 100 and emptied.sum() > 20
    b.free()
    ctx.close()


def test_a_group_larger_than_the_staging(ex, example):
    """The fill kernel stages one wave's 64 records in 24,576 bytes of LDS (BAMREC_STAGE in csrc/ps_bamrec.hip).  Here every name has
    254 characters and every read 200 to 250 bases (PS_MAX_LEN is 250, so the longest read the library takes): a record is at least 36 + 255 + 4 + 100 + 200 = 595 bytes before its tags, 64 of
    them at least 38,080 bytes, so every full group overflows the staging and is built in sub-groups of lanes that fit."""
    import capi
    import simulate as S
    sim = S.simulate_reads(example["genome"], 150, 250, seed=5, indel_scale=30, n_frac=0.002, min_len=200)
    names = [(b"long%04d_" % i).ljust(254, b"x") for i in range(150)]
    fq = os.path.join(ex["dir"], "long.fq")
    _write_fastq(fq, sim, 150, names)
    ctx = capi.Ctx.build(example["fa"], device=0)
    ctx.set_stock("0.04")
    b = _located(ctx, fq)
    dev, origin, st, host, _ = _both(b, 0)
    assert dev == host and st["n_records"] == 150 and st["n_device"] >= 100
    sizes = [4 + r_bs for r_bs in _block_sizes(dev)]
    assert min(len(n) for n in names) == 254 and len(sizes) == 150 and min(sizes) >= 595
    assert all(sum(sizes[g:g + 64]) > 24576 for g in (0, 64))                     # both full groups of 64 exceed the staging
    b.free()
    ctx.close()


@pytest.fixture(scope="module")
def mid_input(mid, workdir):
    import capi
    import simulate as S
    d = os.path.join(workdir, "bamrec_mid")
    os.makedirs(d)
    sim = S.simulate_reads(mid["genome"], n_reads=30000, read_len=50, seed=91, indel_scale=30, n_frac=0.002, min_len=28)
    fq = os.path.join(d, "r.fq")
    S.write_fastq(fq, sim)
    ep, ip = os.path.join(d, "p.errorprofile"), os.path.join(d, "p.indelprofile")
    with open(ep, "w") as f:
        for row in _profile():
            f.write("".join(repr(float(v)) + "\t" for v in row) + "\n")
    open(ip, "w").write("2.1E-5\t5.9E-4")
    if not os.path.exists(mid["fa"] + ".bwt"):
        capi.ps_index(mid["fa"])
    return dict(dir=d, fq=fq, ep=ep, ip=ip, fa=mid["fa"])


def _map_both(m, monkeypatch, tag, **kw):
    """ps_map_to_bam with the switch off, then on: (off path, on path, off stats, on stats, the counters of the on run)"""
    import capi
    monkeypatch.setenv("PS_CHUNK_MB", "1")
    off, on = os.path.join(m["dir"], tag + ".off.bam"), os.path.join(m["dir"], tag + ".on.bam")
    capi.ps_bam_records_device(0)
    st_off = capi.ps_map_to_bam(8, "-1", m["ep"], m["ip"], m["fa"], m["fq"], off, **kw)
    assert capi.ps_bam_records_info()["n_reads"] == 0                              # the host route counts nothing
    capi.ps_bam_records_device(1)
    try:
        st_on = capi.ps_map_to_bam(8, "-1", m["ep"], m["ip"], m["fa"], m["fq"], on, **kw)
        info = capi.ps_bam_records_info()
    finally:
        capi.ps_bam_records_device(0)
    return off, on, st_off, st_on, info


@pytest.mark.parametrize("bgzf_on_device", [False, True])
def test_map_to_bam_unsorted(mid_input, monkeypatch, bgzf_on_device):
    """30,000 reads in several pieces, MAPQ >= 10 and all records: the same inflated stream and the same counts, with host zlib and
    with the device compressor as well"""
    import capi
    capi.ps_bgzf_device(0 if bgzf_on_device else -1)
    try:
        for q in (0, 10):
            off, on, st_off, st_on, info = _map_both(mid_input, monkeypatch, "u%d_%d" % (q, bgzf_on_device), min_mapq=q)
            assert gzip.decompress(open(off, "rb").read()) == gzip.decompress(open(on, "rb").read()), q
            assert (st_off["n_in"], st_off["n_out"]) == (st_on["n_in"], st_on["n_out"]) and st_on["n_in"] == 30000
            assert info["n_device"] > 0 and info["n_device"] + info["n_host"] == info["n_records"] == st_on["n_out"] and info["n_reads"] == 30000
    finally:
        capi.ps_bgzf_device(-1)


def test_map_to_bam_sorted_and_indexed(mid_input, monkeypatch):
    """the same records through the same writer at the same level: the .bam and the .bai are the same files"""
    monkeypatch.setenv("PS_BAM_LEVEL", "6")
    off, on, st_off, st_on, info = _map_both(mid_input, monkeypatch, "sorted", min_mapq=1, sort_by_coordinate=True, write_index=True)
    assert open(off, "rb").read() == open(on, "rb").read() and open(off + ".bai", "rb").read() == open(on + ".bai", "rb").read()
    assert st_off == st_on and info["n_device"] > 0 and info["n_device"] + info["n_host"] == st_on["n_out"]


_CHILD = """
import os, sys
sys.path.insert(0, sys.argv[1])
import capi
capi.ps_map_route(sys.argv[2], sys.argv[3], sys.argv[4], transcripts_fa=sys.argv[5], threads=4)
info = capi.ps_bam_records_info()
print("INFO", info["n_reads"], info["n_device"], info["n_host"], info["n_records"])
"""


def test_map_route_under_the_environment_switch(workdir):
    """the route test's input with transcripts (a sorted + indexed pass whose records are kept, a name-sorted pass): every BAM of a call
    made in a fresh process with PS_BAM_RECORDS_GPU=1 inflates to the bytes of the same call without it; the child's counters show
    that its passes took the device route; with the switch set back to 0 this process writes the host route's files again"""
    import capi
    import map_route as M
    d = os.path.join(workdir, "bamrec_route")
    os.makedirs(d)
    data = M.make_data(d)
    capi.ps_index(data["genome_fa"])
    capi.ps_index(data["transcripts_fa"])
    for where in ("host", "dev", "back"):
        os.makedirs(os.path.join(d, where))
    capi.ps_bam_records_device(0)
    capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "host", "o"), transcripts_fa=data["transcripts_fa"], threads=4)
    e = dict(os.environ, PS_BAM_RECORDS_GPU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "para-suite_amd"), data["route_fastq"], data["genome_fa"], os.path.join(d, "dev", "o"),
                        data["transcripts_fa"]], env=e, timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    n_reads, n_device, n_host, n_records = (int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("INFO")][0].split()[1:])
    assert n_reads > data["n_route_reads"] and n_device > 0 and n_device + n_host == n_records
    capi.ps_bam_records_device(1)
    capi.ps_bam_records_device(0)
    capi.ps_map_route(data["route_fastq"], data["genome_fa"], os.path.join(d, "back", "o"), transcripts_fa=data["transcripts_fa"], threads=4)
    assert capi.ps_bam_records_info()["n_reads"] == 0
    files = sorted(os.listdir(os.path.join(d, "host")))
    bams = [f for f in files if f.endswith(".bam")]
    assert len(bams) >= 3 and files == sorted(os.listdir(os.path.join(d, "dev"))) == sorted(os.listdir(os.path.join(d, "back")))
    for f in files:
        h, v, k = (open(os.path.join(d, w, f), "rb").read() for w in ("host", "dev", "back"))
        assert h == k, f
        if f.endswith(".bam"):
            assert gzip.decompress(h) == gzip.decompress(v), f
        else:
            assert h == v, f
