"""CPU tier: the draw of the randomised GPU parity sweep (tests/fuzz_parity.py, draw_case) without a GPU.

test_gpu_fuzz.py runs seeds 11, 12 and 13 of the default draw; adding the opt-in ranges="edges" must not move one draw of that
stream.  The values below were recorded from the sweep as it stood before draw_case existed (its GPU and oracle calls replaced
by recorders): per case the genome kind, read length, ragged flag, read count, cost model (stock -n, or -X, the profile's T->C
and T->T entries, insertion and deletion rates), tier sizes, and the first 16 hex digits of the SHA-256 of the FASTA and FASTQ
files it wrote."""
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PINNED = {
    11: [
        ('plain', 150, False, 1500, ('profile', 3, 0.02, 0.972, 2.1e-05, 0.00059), None, '0347a99462d3ca58', '78a6b7f9328f6e7c'),
        ('lowcomplexity', 65, False, 3000, ('stock', '0.04'), None, '4b4bf54881be83a2', '3deda968ecd2a22d'),
        ('plain', 75, False, 3000, ('profile', 1, 0.005, 0.987, 0.0, 0.0), None, 'cd6ed99e3ee9959b', 'ea9bed5f232077dc'),
        ('lowcomplexity', 150, False, 1500, ('profile', 1, 0.3, 0.692, 2.1e-05, 0.00059), None, 'a3bebe380cced853', 'f16416a731febbca'),
        ('repeats', 65, False, 3000, ('profile', 3, 0.12, 0.872, 2.1e-05, 0.01), ([64, 4096, 2000064], [2, 64, 65536], 0), 'b08ae0e6a1056f95', 'c6bb9613acf8d46f'),
        ('repeats', 150, False, 1500, ('stock', '2'), None, 'c14d8729665eac8b', 'fdda95b3b647398f'),
        ('tiny', 100, True, 1500, ('profile', 3, 0.12, 0.872, 2.1e-05, 0.0), None, '95cae89db41f6043', '27c8ddc623b4321d'),
        ('lowcomplexity', 51, False, 3000, ('stock', '0.04'), ([512, 4096, 2000064], [2, 64, 65536], 0), 'ad3ff8fd0c8afd67', 'db271d84fae50b8f'),
    ],
    12: [
        ('plain', 20, False, 3000, ('stock', '0'), None, '2ef0d82d0f69e0b7', '0651f2317fe34dd2'),
        ('plain', 20, False, 3000, ('profile', 3, 0.02, 0.972, 0.001, 0.00059), None, '1476cf17f6a2a29b', '6b6168cdfe9860f0'),
        ('repeats', 20, False, 3000, ('stock', '1'), None, '0e33694781123bcc', '1ce7bad5ed38c36d'),
        ('plain', 75, False, 3000, ('profile', 1, 0.12, 0.872, 0.001, 0.01), ([512, 4096, 2000064], [2, 64, 65536], 0), '4e22145e9172fe01', 'e761cafa892df81a'),
        ('repeats', 100, False, 1500, ('profile', 1, 0.005, 0.987, 0.001, 0.01), ([512, 4096, 2000064], [2, 64, 65536], 0), '7f905a09707cbfa7', '2db21ac4180387b8'),
        ('tiny', 100, False, 1500, ('stock', '1'), None, '85bf536127406478', '612b12de5872d97a'),
        ('repeats', 36, False, 3000, ('stock', '0.02'), ([512, 4096, 2000064], [2, 64, 65536], 0), 'a4d1917a3ea4f2f3', 'a1265cf4eef5c4b9'),
        ('plain', 51, False, 3000, ('stock', '0.02'), None, 'd303fcd74695b963', '95c98206772e734b'),
    ],
    13: [
        ('tiny', 64, False, 3000, ('stock', '2'), None, '681810c2db39e269', 'eb9c2917837a5393'),
        ('lowcomplexity', 50, False, 3000, ('profile', -1, 0.005, 0.987, 2.1e-05, 0.01), None, '96de7e4e350aeaef', 'cd2b224805dda88b'),
        ('repeats', 150, False, 1500, ('profile', -1, 0.12, 0.872, 2.1e-05, 0.0), None, 'd90dfe184e4d0ffa', '8b58c986eb553d58'),
        ('lowcomplexity', 65, False, 3000, ('profile', -1, 0.005, 0.987, 0.0, 0.0), None, 'e01d072965e6b3ae', '5db741a2e54f28c1'),
        ('repeats', 150, False, 1500, ('stock', '0.04'), None, '5ba163a160b9da14', 'f5470e67f5ce22eb'),
        ('tiny', 36, True, 3000, ('profile', -1, 0.005, 0.987, 0.001, 0.00059), ([64, 4096, 2000064], [2, 64, 65536], 0), 'ca757df613d57661', '2cd650566dd34b04'),
        ('lowcomplexity', 150, False, 1500, ('profile', 3, 0.005, 0.987, 0.0, 0.0), ([64, 4096, 2000064], [2, 64, 65536], 0), 'f88e48649a98c98e', '0a207b15f63a60f7'),
        ('plain', 150, False, 1500, ('stock', '0'), None, 'c077df94dc3dc8ee', 'ca72382798033dbe'),
    ],
}


def _digest(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]


def _cost(c):
    if c["mode"] == "stock":
        return ("stock", c["n"])
    return ("profile", c["x"], float(c["P"][3, 1]), float(c["P"][3, 3]), c["ins"], c["dele"])


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_default_draw_is_pinned(tmp_path, seed):
    import fuzz_parity
    rng = np.random.default_rng(seed)
    for case, exp in enumerate(PINNED[seed]):
        c = fuzz_parity.draw_case(rng, case, str(tmp_path))
        tiers = None if c["tiers"] is None else (list(c["tiers"][0]), list(c["tiers"][1]), c["tiers"][2])
        got = (c["kind"], c["L"], c["mixed"], c["n_reads"], _cost(c), tiers, _digest(c["fa"]), _digest(c["fq"]))
        assert got == exp, (seed, case)


def test_edge_draw_stays_inside_the_accepted_ranges(tmp_path):
    """ranges="edges": profile -X 4..15, stock -n 5..37, reads of 33..250 bp (none without a seed rule), ragged cases among them,
    and both sides of the wide / narrow line"""
    import fuzz_parity
    rng = np.random.default_rng(5)
    seen = set()
    for case in range(40):
        c = fuzz_parity.draw_case(rng, case, str(tmp_path), ranges="edges")
        if c["mode"] == "stock":
            assert 5 <= int(c["n"]) <= 37
            seen.add("stock wide" if int(c["n"]) >= 17 else "stock narrow")
        else:
            assert 4 <= c["x"] <= 15
            seen.add("profile wide" if c["x"] >= 8 else "profile narrow")
        lens = []
        with open(c["fq"]) as f:
            for i, line in enumerate(f):
                if i % 4 == 1:
                    lens.append(len(line.rstrip("\n")))
        assert len(lens) == c["n_reads"] and 33 <= min(lens) and max(lens) <= c["L"] <= 250
        if c["mixed"]:
            seen.add("mixed")
        if c["L"] > 150:
            seen.add("long")
        os.remove(c["fa"]); os.remove(c["fq"])
    assert seen == {"stock wide", "stock narrow", "profile wide", "profile narrow", "mixed", "long"}, seen
