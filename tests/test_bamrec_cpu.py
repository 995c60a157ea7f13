"""The BAM record of a located read as csrc/ps_bamrec.h states it for host and device, without a device.  tests/bamrec_check.cpp
is the header under the host compiler alone, built with AddressSanitizer and UBSan as a plain executable; every input array is a
heap block of its exact size and the destination stands between guard bytes.  What it writes is held to a record built here from
first principles (struct.pack, an MD / NM walk of its own over the case's reference string), and -- as a second opinion -- the
records are put into a BAM file that tests/test_bam.py's independent reader decodes field by field."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
RNG = np.random.default_rng(0xBA3)
REF = "".join("ACGT"[c] for c in RNG.integers(0, 4, 1200))
L_PAC = len(REF)
CONTIGS = [(0, 700), (700, 500)]
HOLES = [(100, 1), (300, 11)]
MAX_TOP2 = 30
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _read(pos, cigar, strand, bad=(), n_at=(), length=None):
    """codes in read orientation of a read that aligns at pos with this CIGAR: reference bases (past the text: A), inserted and
    clipped bases drawn, the oriented positions in `bad` changed to another base, those in n_at to N"""
    ops = cigar or [(length, "M")]
    o, x = [], pos
    for l, op in ops:
        if op == "M":
            o += ["ACGT".index(REF[x + z]) if x + z < L_PAC else 0 for z in range(l)]
            x += l
        elif op == "D":
            x += l
        else:
            o += [int(v) for v in RNG.integers(0, 4, l)]
    for y in bad:
        o[y] = (o[y] + 1) % 4
    for y in n_at:
        o[y] = 4
    return [c if c > 3 else 3 - c for c in reversed(o)] if strand else o


def _case(name, pos, strand=0, cigar=None, length=50, typ=1, mapq=37, qual=True, c1=1, c2=0, n_mm=0, n_gapo=0, n_gape=0, **kw):
    seq = _read(pos if typ else 0, cigar, strand if typ else 0, length=length, **kw)
    q = bytes(int(v) for v in RNG.integers(33, 74, len(seq))) if qual else None
    return dict(name=name if isinstance(name, bytes) else name.encode(), seq=seq, qual=q, type=typ, pos=pos if typ else 0, strand=strand, mapq=mapq,
                n_mm=n_mm, n_gapo=n_gapo, n_gape=n_gape, c1=c1, c2=c2, cigar=cigar or [])


GAPPED = [(5, "S"), (20, "M"), (2, "I"), (10, "M"), (3, "D"), (13, "M")]
CASES = []
for L in (1, 2, 49, 50, 255, 256):
    for strand in (0, 1):
        CASES.append(_case("len%d_%d" % (L, strand), 400 + L, strand, length=L, bad=(L // 2,), n_mm=1))
CASES += [
    _case("n_in_read", 420, 0, n_at=(0, 17, 49)), _case("n_in_read_rev", 421, 1, n_at=(0, 17, 49)),
    _case("no_qual", 430, 0, qual=False), _case("no_qual_rev", 431, 1, qual=False, length=33),
    _case("x", 440), _case(b"n" * 254, 441, 1),
    _case("unmapped", 0, typ=0, mapq=25), _case("unmapped_odd", 0, typ=0, length=37, qual=False, n_at=(3,)),
    _case("emptied_rev", 0, strand=1, typ=0, length=11),
    _case("bridging", 680, 0), _case("bridging_rev", 660, 1, length=41),
    _case("hole1", 90, 0), _case("hole11", 295, 1), _case("hole_partly", 305, 0, length=30),
    _case("c1_255", 450, c1=255, c2=7, mapq=0), _case("c1_256", 451, c1=256, mapq=0), _case("c1_65535", 452, 1, c1=65535, mapq=0),
    _case("c1_65536", 453, c1=65536, c2=70000, mapq=0),
    _case("top2_at", 460, c1=MAX_TOP2, c2=300, mapq=0), _case("top2_above", 461, c1=MAX_TOP2 + 1, c2=300, mapq=0),
    _case("gapped", 500, 0, GAPPED, n_gapo=2, n_gape=3, bad=(9,), n_mm=1), _case("gapped_rev", 510, 1, GAPPED, n_gapo=2, n_gape=3, mapq=25),
    # the read bases on both sides of the deletion mismatch: MD runs of length 0 before ^ and after the deleted bases
    _case("del_mismatch", 520, 0, [(20, "M"), (2, "D"), (30, "M")], n_gapo=1, n_gape=1, bad=(19, 20), n_mm=2),
    _case("del_first_base", 530, 1, [(1, "M"), (1, "D"), (49, "M")], n_gapo=1, bad=(0, 1, 49), n_mm=3),
    _case("ins_only", 540, 0, [(25, "M"), (4, "I"), (21, "M")], n_gapo=1, n_gape=3),
    _case("stops_at_l_pac", L_PAC - 20, 0), _case("stops_at_l_pac_rev", L_PAC - 1, 1, length=2),
    _case("del_over_l_pac", L_PAC - 12, 0, [(10, "M"), (5, "D"), (10, "M")], length=20, n_gapo=1, n_gape=4),
]


# ------------------------------------------------------------------ the record from first principles
def _reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _tag_int(tag, v):
    for ty, fmt, lo, hi in (("c", "<b", -128, -1), ("s", "<h", -32768, -1), ("i", "<i", -2 ** 31, -1), ("C", "<B", 0, 255), ("S", "<H", 0, 65535), ("I", "<I", 0, 2 ** 32 - 1)):
        if lo <= v <= hi:
            return tag.encode() + ty.encode() + struct.pack(fmt, v)
    raise AssertionError(v)


def expected(c):
    """(record bytes, (ref, pos, end, flag, mapq), the fields as test_bam.read_bam names them)"""
    seq, L, name = c["seq"], len(c["seq"]), c["name"]
    mapped = c["type"] != 0
    rc = c["strand"] != 0                 # the host route orients by the strand alone: 0 for an unmapped read, kept for a hit whose CIGAR came back empty
    oriented = [s if s > 3 else 3 - s for s in reversed(seq)] if rc else list(seq)
    tags, tag_text, words, cig_text = b"", [], [], "*"
    ref, pos, flag, mapq, span = -1, -1, 4, 0, 0
    if mapped:
        ops = c["cigar"] or [(L, "M")]
        span = sum(l for l, op in ops if op in "MD")
        ref = max(k for k, (off, _) in enumerate(CONTIGS) if off <= c["pos"])
        pos = c["pos"] - CONTIGS[ref][0]
        flag = (4 if pos + span > CONTIGS[ref][1] else 0) | (16 if c["strand"] else 0)
        mapq = c["mapq"]
        nn = sum(max(0, min(c["pos"] + span, off + hl) - max(c["pos"], off)) for off, hl in HOLES)
        words = [l << 4 | "MID_S".index(op) for l, op in ops]
        cig_text = "".join("%d%s" % (l, op) for l, op in ops)
        md, nm, u, x, y = "", 0, 0, c["pos"], 0
        for l, op in ops:
            if op == "M":
                for z in range(l):
                    if x + z >= L_PAC:
                        break
                    if oriented[y + z] > 3 or "ACGT"[oriented[y + z]] != REF[x + z]:
                        md += "%d%s" % (u, REF[x + z]); nm += 1; u = 0
                    else:
                        u += 1
                x += l; y += l
            elif op == "D":
                md += "%d^%s" % (u, REF[x:min(x + l, L_PAC)]); u = 0; x += l; nm += l
            else:
                y += l
                nm += l if op == "I" else 0
        md += "%d" % u
        ints = [("NM", nm)] + ([("XN", nn)] if nn else []) + [("X0", c["c1"])] + ([("X1", c["c2"])] if c["c1"] <= MAX_TOP2 else []) + \
               [("XM", c["n_mm"]), ("XO", c["n_gapo"]), ("XG", c["n_gapo"] + c["n_gape"])]
        xt = "N" if nn > 10 else "NURM"[c["type"]]
        tags = b"XTA" + xt.encode() + b"".join(_tag_int(t, v) for t, v in ints) + b"MDZ" + md.encode() + b"\0"
        tag_text = ["XT:A:" + xt] + ["%s:i:%d" % tv for tv in ints] + ["MD:Z:" + md]
    end = pos + max(span, 1)
    nib = [(15 if s > 3 else 1 << s) for s in oriented] + [0]
    body = name + b"\0" + b"".join(struct.pack("<I", w) for w in words) + bytes(nib[i] << 4 | nib[i + 1] for i in range(0, L, 2))
    q = c["qual"]
    body += b"\xff" * L if q is None else bytes(v - 33 for v in (reversed(q) if rc else q))
    fixed = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, mapq, _reg2bin(pos, end), len(words), flag, L, -1, -1, 0)
    rec = fixed + body + tags
    fields = dict(name=name.decode(), flag=flag, ref=ref, pos=pos, mapq=mapq, bin=_reg2bin(pos, end), nref=-1, npos=-1, tlen=0, cigar=cig_text,
                  seq="".join("ACGTN"[s] for s in oriented), qual="*" if q is None else bytes(reversed(q) if rc else q).decode(), tags=tag_text)
    return struct.pack("<i", len(rec)) + rec, (ref, pos, end, flag, mapq), fields


# ------------------------------------------------------------------ the check program
def build_check(where, sanitize):
    exe = os.path.join(str(where), "bamrec_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g"] if sanitize else ["-O2"]
    subprocess.check_call([os.environ.get("CXX", "c++")] + flags + ["-std=c++17", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "bamrec_check.cpp"), "-o", exe])
    return exe


def run_check(exe, cases, where):
    src, dst = os.path.join(str(where), "cases.txt"), os.path.join(str(where), "out.txt")
    with open(src, "w") as f:
        f.write("ref %s\n" % REF)
        f.write("contigs %d %s\n" % (len(CONTIGS), " ".join("%d %d" % c for c in CONTIGS)))
        f.write("holes %d %s\n" % (len(HOLES), " ".join("%d %d" % h for h in HOLES)))
        f.write("max_top2 %d\n" % MAX_TOP2)
        for c in cases:
            words = [l << 4 | "MIDS".index(op) for l, op in c["cigar"]]          # the library's own words: soft clip is 3
            f.write("rec %s %s %s %d %d %d %d %d %d %d %d %d %d %s\n" % (c["name"].hex(), "".join(str(s) for s in c["seq"]), c["qual"].hex() if c["qual"] is not None else "-",
                                                                       c["type"], c["pos"], c["strand"], c["mapq"], c["n_mm"], c["n_gapo"], c["n_gape"], c["c1"], c["c2"],
                                                                       len(words), " ".join(str(w) for w in words)))
    r = subprocess.run([exe, src, dst], timeout=120, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    for line in open(dst):
        n, ref, pos, end, flag, mapq, *hx = line.split()
        out.append((int(n), (int(ref), int(pos), int(end), int(flag), int(mapq)), bytes.fromhex(hx[0] if hx else "")))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """the sanitizer build, run once over every case as a program of its own"""
    where = tmp_path_factory.mktemp("bamrec")
    got = run_check(build_check(where, sanitize=True), CASES, where)
    assert len(got) == len(CASES)
    return got


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"].decode()[:24] for c in CASES])
def test_size_bytes_and_key(results, k):
    n, key, data = results[k]
    want, want_key, _ = expected(CASES[k])
    assert n == len(data) == len(want), (n, len(data), len(want))
    assert data == want, next((i, data[max(0, i - 8):i + 8].hex(), want[max(0, i - 8):i + 8].hex()) for i in range(len(want)) if data[i] != want[i])
    assert key == want_key


def _bgzf(data):
    out = b""
    for at in list(range(0, len(data), 0xff00)) + [None]:
        chunk = b"" if at is None else data[at:at + 0xff00]
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = z.compress(chunk) + z.flush()
        out += b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk))
    return out


def test_second_opinion_through_the_bam_reader(results, tmp_path):
    """the records of the check program in a BAM file of this test's making, decoded by tests/test_bam.py's reader"""
    from test_bam import read_bam
    head = b"BAM\x01" + struct.pack("<i", 0) + struct.pack("<i", len(CONTIGS))
    for k, (_, ln) in enumerate(CONTIGS):
        nm = b"c%d\0" % k
        head += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
    path = str(tmp_path / "recs.bam")
    with open(path, "wb") as f:
        f.write(_bgzf(head + b"".join(r[2] for r in results)))
    _, refs, recs, _ = read_bam(path)
    assert refs == [("c0", 700), ("c1", 500)] and len(recs) == len(CASES)
    for c, r in zip(CASES, recs):
        del r["u0"], r["u1"]
        assert r == expected(c)[2], c["name"]


def test_what_the_cases_are_for(results):
    """every case does what it is in the list for, in the bytes the check program wrote"""
    assert all(r[2] == expected(c)[0] for c, r in zip(CASES, results))
    f = {c["name"]: expected(c)[2] for c in CASES}
    tag = lambda name, t: [x for x in f[name]["tags"] if x.startswith(t)]
    assert f[b"unmapped"]["flag"] == 4 and f[b"unmapped"]["mapq"] == 0 and f[b"unmapped"]["tags"] == [] and f[b"unmapped"]["cigar"] == "*"
    assert f[b"bridging"]["flag"] == 4 and f[b"bridging"]["pos"] == 680 and f[b"bridging_rev"]["flag"] == 20 and f[b"bridging"]["tags"]
    assert tag(b"hole1", "XN") == ["XN:i:1"] and tag(b"hole1", "XT") == ["XT:A:U"]
    assert tag(b"hole11", "XN") == ["XN:i:11"] and tag(b"hole11", "XT") == ["XT:A:N"] and tag(b"hole_partly", "XN") == ["XN:i:6"]
    assert tag(b"top2_at", "X1") == ["X1:i:300"] and tag(b"top2_above", "X1") == []
    assert "0^" in tag(b"del_mismatch", "MD")[0] and tag(b"del_mismatch", "NM") == ["NM:i:4"]
    md = tag(b"del_mismatch", "MD")[0]
    assert md[md.index("^") + 3] == "0"                                         # ^ two deleted bases, then a run of 0 before the next mismatch
    assert tag(b"gapped", "NM") == ["NM:i:6"] and f[b"gapped"]["cigar"] == "5S20M2I10M3D13M"
    assert tag(b"stops_at_l_pac", "MD") == ["MD:Z:20"] and tag(b"stops_at_l_pac_rev", "MD") == ["MD:Z:1"]
    assert tag(b"del_over_l_pac", "MD")[0] == "MD:Z:10^" + REF[-2:] + "0"
    assert tag(b"n_in_read", "NM") == ["NM:i:3"] and f[b"n_in_read"]["seq"][0] == "N" and f[b"n_in_read_rev"]["seq"][-1] == "N"
    assert len(f[b"n" * 254]["name"]) == 254 and f[b"no_qual"]["qual"] == "*"


def test_plain_build_agrees(results, tmp_path):
    """the header at -O2 without a sanitizer writes the same"""
    assert run_check(build_check(tmp_path, sanitize=False), CASES, tmp_path) == results


def test_exported_and_in_the_binding():
    import ctypes as C
    import capi
    lib = capi.lib()
    for name in ("ps_bam_records_device", "ps_bam_records_info", "ps_batch_bam_records"):
        assert hasattr(lib, name) and name in capi.SIGNATURES and name in capi.EXPORTS
    assert capi.STRUCTS["ps_bam_records_stats"] is capi.BamRecordsStats and C.sizeof(capi.BamRecordsStats) == 72
    capi.ps_bam_records_device(1)                     # the switch and its counters need no device; building records does
    assert capi.ps_bam_records_info() == dict(n_reads=0, n_records=0, n_device=0, n_host=0, bytes=0, ms_upload=0.0, ms_kernels=0.0, ms_host_records=0.0, ms_download=0.0)
    capi.ps_bam_records_device(0)
