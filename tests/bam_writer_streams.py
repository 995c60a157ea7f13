"""What tests/bamsink_check.cpp writes, reduced to what must not move when the writer's code does: per BAM the SHA-256 of the
inflated stream, the ISIZE of every block and the number of records, read with test_bam.py's independent reader; per other file the
SHA-256 of its bytes.  Compressed bytes and .bai bytes depend on the zlib at hand and are left out.  Shared by
test_bam_writer_stable_cpu.py and tests/golden/make_bam_writer_golden.py."""
import hashlib
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden", "bam_writer_streams.json")


def build_and_run(workdir):
    """the check program, with AddressSanitizer and UBSan, run into workdir/out; -> (that directory, its stdout lines)"""
    exe, out = os.path.join(workdir, "bamsink_check"), os.path.join(workdir, "out")
    os.makedirs(out)
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                           "-I", CSRC, os.path.join(HERE, "bamsink_check.cpp"), os.path.join(CSRC, "ps_bam.cpp"), "-o", exe, "-lz", "-lpthread"])
    r = subprocess.run([exe, out], timeout=300, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return out, r.stdout.splitlines()


def digest(out):
    import test_bam as T
    d = {}
    for name in sorted(os.listdir(out)):
        path = os.path.join(out, name)
        if name.endswith(".bai"):
            continue
        if not name.endswith(".bam"):
            d[name] = {"sha256": hashlib.sha256(open(path, "rb").read()).hexdigest()}
            continue
        blocks = T.bgzf_blocks(path)
        d[name] = {"sha256": hashlib.sha256(b"".join(p for _, _, p in blocks)).hexdigest(), "isize": [len(p) for _, _, p in blocks],
                   "n_records": len(T.read_bam(path)[2])}
    return d
