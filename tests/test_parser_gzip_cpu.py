"""CPU tier: gzip and BGZF compressed FASTQ / FASTA through the read parser (csrc/ps_inflate.h behind csrc/ps_reads.cpp; host code,
no GPU call).  The same reads however the text is compressed, cut into members or streamed; the hand-over between the inflater
and the parser wrapping many times; every kind of damage an error that names the file, with no thread left behind; and the byte
source alone under AddressSanitizer and UBSan (tests/inflate_check.cpp, a plain executable), damaged inputs included."""
import os
import subprocess

import numpy as np
import pytest

import capi
import gz_forms as G
from test_capi_cpu import ROOT
from test_parser_cpu import _records, _write

KINDS = {"plain": {}, "wrapped": dict(wrap=40), "crlf": dict(crlf=True), "fasta": dict(fasta=True), "nofinal": dict(final_newline=False)}


@pytest.fixture(scope="module")
def recs():
    return _records(30000, np.random.default_rng(5))           # ~6 MB, as tests/test_parser_cpu.py


@pytest.fixture(scope="module")
def texts(recs, tmp_path_factory):
    """kind -> (path of the plain file, its bytes, ps_parse_check of it); made when first asked for"""
    d, made = tmp_path_factory.mktemp("gzkinds"), {}
    def get(kind):
        if kind not in made:
            p = str(d / ("r." + kind))
            _write(p, recs, **KINDS[kind])
            ref = capi.ps_parse_check(p, 1, 0)
            assert ref[0] == len(recs) and ref[1] == sum(len(r[1]) for r in recs)
            made[kind] = (p, open(p, "rb").read(), ref)
        return made[kind]
    return get


@pytest.mark.parametrize("form", sorted(G.FORMS))
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_same_reads_however_compressed(texts, tmp_path, kind, form):
    plain, text, ref = texts(kind)
    data = G.FORMS[form](text)
    assert data[:2] == b"\x1f\x8b" and (form != "gz0" or len(data) > len(text))
    p = str(tmp_path / ("r.%s.%s.gz" % (kind, form)))
    open(p, "wb").write(data)
    assert capi.ps_parse_check(p, 1, 0)[:3] == ref[:3]
    assert capi.ps_parse_check(p, 8, 0)[:3] == ref[:3]
    for window in (4096, 100_000, 1_000_000):
        for threads in (1, 8):
            got = capi.ps_parse_check(p, threads, window)
            assert got[:3] == ref[:3], (kind, form, window, threads)
            if window < 1_000_000:
                assert got[3] > 4                              # really streamed in pieces


def test_plain_input_is_parsed_as_before(texts):
    """the piece counts of a plain file follow from its size, which a compressed input does not state"""
    plain, text, ref = texts("plain")
    assert capi.ps_parse_check(plain, 8, 0) == ref
    a = capi.ps_parse_check(plain, 3, 1_000_000)
    assert a[:3] == ref[:3] and a[3] == -(-len(text) // 1_000_000) - (len(text) % 1_000_000 <= 125_000)


def test_the_hand_over_wraps(texts, recs, tmp_path, monkeypatch):
    """1 MB windows: a 10 MB input passes through the two-window hand-over five times over (the same reads twice); a 20 MB input of identical records
    compresses above 500:1, so one read of compressed bytes inflates into many windows"""
    monkeypatch.setenv("PS_UNIT_MB", "1")
    plain, text, _ = texts("plain")
    big = text + text
    assert 10_000_000 < len(big)
    p = str(tmp_path / "ten.fq")
    open(p, "wb").write(big)
    ref = capi.ps_parse_check(p, 4, 0)
    for name, data in (("gz", G.gz(big, 1)), ("bgzf", G.bgzf(big, 1))):
        open(p + "." + name, "wb").write(data)
        assert capi.ps_parse_check(p + "." + name, 4, 0)[:3] == ref[:3]
        assert capi.ps_parse_check(p + "." + name, 4, 3 << 20)[:3] == ref[:3]
    # deflate spends a length and a distance code per 258 bytes, and the distance's extra bits decide the ratio: 6 bits for a
    # 200-byte record (258:1), one for a record of up to 8 bytes (688:1) -- hence FASTA records of 7 bytes
    same = b">r\nACG\n"
    same = same * (20_000_000 // len(same) + 1)
    q = str(tmp_path / "same.fq")
    open(q, "wb").write(same)
    z = G.gz(same, 6)
    assert len(same) > 20_000_000 and len(same) > 500 * len(z)
    open(q + ".gz", "wb").write(z)
    ref = capi.ps_parse_check(q, 4, 0)
    assert ref[0] == len(same) // 7 and capi.ps_parse_check(q + ".gz", 4, 0)[:3] == ref[:3]
    assert capi.ps_parse_check(q + ".gz", 4, 2 << 20)[:3] == ref[:3]


def test_inputs_from_a_fifo(texts, tmp_path):
    """the kind is told from the first two bytes, which a FIFO cannot give back: plain text loses none, compressed text is inflated"""
    import threading
    plain, text, _ = texts("plain")
    text = text[:text.index(b"\n@read3000") + 1]
    p = str(tmp_path / "small.fq")
    open(p, "wb").write(text)
    ref = capi.ps_parse_check(p, 1, 0)
    for name, data in (("plain", text), ("gz", G.gz(text)), ("bgzf", G.bgzf(text)), ("bgzf_gz", G.bgzf_then_gz(text))):
        for chunk in (0, 100_000):
            fifo = str(tmp_path / ("fifo_%s_%d" % (name, chunk)))
            os.mkfifo(fifo)
            def feed():
                with open(fifo, "wb") as f:
                    f.write(data)
            t = threading.Thread(target=feed)
            t.start()
            got = capi.ps_parse_check(fifo, 4, chunk)
            t.join()
            assert got[:3] == ref[:3], (name, chunk)


def _n_threads():
    return int([l for l in open("/proc/self/status") if l.startswith("Threads:")][0].split()[1])


def _damaged(text):
    """name -> bytes; every one of them must be refused"""
    z, b = G.gz(text), G.bgzf(text)
    body = 10                                                  # Python's gzip writes the ten fixed header bytes only
    flip = bytearray(z); flip[len(z) // 2] ^= 0x10
    crc = bytearray(z); crc[-8] ^= 0xff
    isize = bytearray(z); isize[-4] ^= 0x01
    cm7 = bytearray(z); cm7[2] = 7
    reserved = bytearray(z); reserved[3] |= 0x20
    second = len(G.bgzf_block(text[:0xff00]))                  # where the second BGZF block starts
    small = bytearray(b); small[16:18] = (20).to_bytes(2, "little")
    return {
        "cut_after_2": z[:2], "cut_in_header": z[:body - 3], "cut_in_data": z[:len(z) // 2], "cut_3_before_end": z[:-3],
        "crc32": bytes(crc), "isize": bytes(isize), "bit_flip": bytes(flip), "hello_appended": z + b"hello", "cm7": bytes(cm7),
        "reserved_flag": bytes(reserved),
        "bgzf_bsize_past_end": b[:second + 1000], "bgzf_bsize_too_small": bytes(small), "bgzf_hello_appended": b + b"hello",
        "bgzf_cut_in_end_marker": b[:-9],
    }


def test_damage_is_an_error_that_names_the_file(texts, tmp_path):
    plain, text, _ = texts("plain")
    text = text[:text.index(b"\n@read3000") + 1]               # ~600 KB: ten BGZF blocks
    p = str(tmp_path / "small.fq")
    open(p, "wb").write(text)
    ref = capi.ps_parse_check(p, 1, 0)
    good = str(tmp_path / "good.fq.gz")
    open(good, "wb").write(G.gz(text))
    assert capi.ps_parse_check(good, 2, 0)[:3] == ref[:3]
    bad = {}
    for name, data in _damaged(text).items():
        bad[name] = str(tmp_path / ("bad_%s.fq.gz" % name))
        open(bad[name], "wb").write(data)
    for name, path in bad.items():
        for chunk in (0, 100_000):
            with pytest.raises(capi.PsError) as ei:
                capi.ps_parse_check(path, 4, chunk)
            print(name, chunk, "->", str(ei.value))
            assert path in str(ei.value), name
            if not name.startswith("cut_after") and name != "cm7":
                assert "compressed byte" in str(ei.value)
        assert capi.ps_parse_check(good, 2, 0)[:3] == ref[:3] and capi.ps_parse_check(good, 2, 100_000)[:3] == ref[:3]
    capi.ps_parse_check(good, 4, 100_000)
    before = _n_threads()
    names = sorted(bad)
    for k in range(50):
        with pytest.raises(capi.PsError):
            capi.ps_parse_check(bad[names[k % len(names)]], 4, 100_000 if k & 1 else 0)
    assert _n_threads() == before
    assert capi.ps_parse_check(good, 2, 0)[:3] == ref[:3]


# ---------------------------------------------------------------- the byte source alone, under the sanitizers
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("inflate") / "inflate_check")
    csrc = os.path.join(ROOT, "para-suite_amd", "csrc")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g", "-Wall",
                           "-Werror", "-pthread", "-I", csrc, os.path.join(ROOT, "tests", "inflate_check.cpp"), os.path.join(csrc, "ps_inflate.cpp"),
                           "-lz", "-o", out])
    return out


def _fnv(data):
    """FNV-1a over the bytes, as tests/inflate_check.cpp computes it"""
    a = np.frombuffer(data, dtype=np.uint8)
    h = 1469598103934665603
    for c in a.tolist():
        h = ((h ^ c) * 1099511628211) & 0xffffffffffffffff
    return h


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode in (0, 3) and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.returncode, r.stdout.splitlines()


def test_the_source_under_the_sanitizers(exe, texts, tmp_path):
    plain, text, _ = texts("plain")
    text = text[:text.index(b"\n@read3000") + 1]               # ~600 KB: ten BGZF blocks, three of the driver's 256 KB windows
    want = "%d %d" % (len(text), _fnv(text))
    p = str(tmp_path / "t.fq")
    open(p, "wb").write(text)
    assert _run(exe, "read", p) == (0, [want])
    for form, data in G.forms(text).items():
        open(p + "." + form, "wb").write(data)
        assert _run(exe, "read", p + "." + form) == (0, [want]), form
    for name, data in _damaged(text).items():
        open(p + "." + name, "wb").write(data)
        rc, out = _run(exe, "read", p + "." + name)
        assert rc == 3 and len(out) == 1 and out[0].startswith("error: ") and p + "." + name in out[0], (name, out)
    assert _run(exe, "read", str(tmp_path / "missing.gz"))[0] == 3
    # damaged copies of a ~30 KB input: a changed byte that does not matter (MTIME, XFL, OS) gives the text, every other an error
    small = text[:text.index(b"\n@read151 ") + 1]
    assert 25_000 < len(small) < 40_000
    want = "%d %d" % (len(small), _fnv(small))
    for name, data, seed in (("gz", G.gz(small), 11), ("bgzf", G.bgzf(small, block=5000), 12)):
        q = str(tmp_path / ("sweep." + name))
        open(q, "wb").write(data)
        rc, out = _run(exe, "sweep", q, seed, 300)
        assert rc == 0 and len(out) == 300 and set(out) <= {"error", want}, [l for l in out if l not in ("error", want)][:3]
        print(name, "sweep:", out.count("error"), "errors,", out.count(want), "read as the text")
        assert out.count("error") > 250
