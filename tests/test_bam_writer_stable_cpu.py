"""The bytes of every BAM writer, held still on the CPU.  tests/bamsink_check.cpp drives BamSink (unsorted through both add()
overloads, sorted by coordinate with index and by name, each once with the records kept, empty, a header of two blocks) and
sam_to_bam, bam_view, bam_sort, bam_index and extract_weak_reads through ps_bam.h's public interface, built with AddressSanitizer and
UBSan as a plain executable.  Every file it writes is read with test_bam.py's independent reader and compared with
tests/golden/bam_writer_streams.json: the inflated stream, the cut into blocks, the number of records.  The index files get
test_bam.py's region queries in spirit: every chunk must point at record starts of its reference."""
import json
import os

import pytest

import bam_writer_streams as W
import test_bam as T


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    out, lines = W.build_and_run(str(tmp_path_factory.mktemp("bamsink")))
    assert lines[-1] == "all ok", lines
    return out


@pytest.fixture(scope="module")
def golden():
    return json.load(open(W.GOLDEN))


def test_the_program_wrote_the_files_of_the_golden_list(written, golden):
    assert sorted(n for n in os.listdir(written) if not n.endswith(".bai")) == sorted(golden)
    assert sorted(n for n in os.listdir(written) if n.endswith(".bai")) == [
        "bighead_coord.bam.bai", "coord.bam.bai", "coord_keep.bam.bai", "empty_coord.bam.bai", "indexed.bam.bai", "s2b_sorted.bam.bai"]


def test_every_stream_every_cut_and_every_count_is_the_golden_one(written, golden):
    got = W.digest(written)
    for name in sorted(golden):
        assert got[name] == golden[name], name


def test_the_cases_the_records_were_made_for(golden):
    """three or more body blocks in the large files, a header of two blocks, a block that ends where the first buffer ends"""
    for name in ("unsorted_span.bam", "coord.bam", "name.bam", "coord_keep.bam", "name_keep.bam"):
        assert golden[name]["isize"][1:4] == [0xff00] * 3 and golden[name]["isize"][-1] == 0 and golden[name]["n_records"] == 3000, name
    assert golden["bighead.bam"]["isize"][0] == golden["bighead_coord.bam"]["isize"][0] == 0xff00 and golden["bighead.bam"]["isize"][1] > 0
    assert golden["unsorted_vec.bam"]["isize"][1:4] == [0xff00, 600 * 120 - 0xff00, 0xff00]      # a block never spans two buffers: no empty one either
    assert golden["empty.bam"]["n_records"] == golden["empty_coord.bam"]["n_records"] == 0 and len(golden["empty.bam"]["isize"]) == 2
    assert golden["coord.bam"] == golden["coord_keep.bam"] and golden["name.bam"] == golden["name_keep.bam"]
    assert golden["s2b_sorted.bam"] == golden["sort_coord.bam"] == golden["indexed.bam"]


@pytest.mark.parametrize("name", ["coord.bam", "coord_keep.bam", "s2b_sorted.bam", "indexed.bam", "bighead_coord.bam", "empty_coord.bam"])
def test_index_chunks_point_at_record_starts(written, name):
    path = os.path.join(written, name)
    _, refs, recs, starts = T.read_bam(path)
    idx, n_no_coor = T.read_bai(path + ".bai")
    assert len(idx) == len(refs) and n_no_coor == sum(r["ref"] < 0 for r in recs)
    begins = {r["u0"]: r for r in recs}
    ends = {r["u1"] for r in recs}
    for tid, (bins, lin) in enumerate(idx):
        mine = [r for r in recs if r["ref"] == tid]
        covered = set()
        for b, chunks in bins.items():
            if b == 37450:
                assert chunks[1] == (sum(not r["flag"] & 4 for r in mine), sum(bool(r["flag"] & 4) for r in mine))
                continue
            for cb, ce in chunks:
                u0, u1 = T.voffset_to_u(starts, cb), T.voffset_to_u(starts, ce)
                assert begins[u0]["ref"] == tid and u1 in ends
                inside = [r for r in mine if u0 <= r["u0"] < u1 and T.reg2bin(r["pos"], r["pos"] + 36) == b]
                covered.update(r["u0"] for r in inside)
        assert covered == {r["u0"] for r in mine}                      # every record of the reference is in a chunk of its bin
        for w, v in enumerate(lin):
            first = [r for r in mine if r["pos"] >> 14 <= w <= (r["pos"] + 35) >> 14]
            if first:
                assert T.voffset_to_u(starts, v) == first[0]["u0"]
