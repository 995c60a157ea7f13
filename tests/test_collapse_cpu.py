"""The grouping rule of the collapsed search (csrc/ps_collapse.h) on the host.  tests/collapse_check.cpp includes that header, packs
reads the way a bin does and runs key -> stable sort -> heads -> rep_of; it is built by the host compiler with AddressSanitizer and
UBSan and runs as a plain executable.  The reference is a Python dict keyed on (length, sequence text)."""
import os
import re
import subprocess

import numpy as np
import pytest

import collapse_reads as R
from test_capi_cpu import ROOT

CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
GROUP_SIZES = [1, 2, 63, 64, 65, 256, 257]
LENGTHS = [16, 17, 32, 33, 250]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("collapse") / "collapse_check")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                           "-Wno-unknown-pragmas", "-I", CSRC, os.path.join(ROOT, "tests", "collapse_check.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    rng = np.random.default_rng(20240)
    distinct = [R.random_seq(rng, int(rng.integers(36, 51))) for _ in GROUP_SIZES]
    mult = list(GROUP_SIZES)
    for l in LENGTHS:                       # every length alone and as a pair of copies
        distinct += [R.random_seq(rng, l), R.random_seq(rng, l)]
        mult += [1, 2]
    adv = R.adversarial_reads(rng)
    distinct += adv
    mult += [1 + (i % 3) for i in range(len(adv))]      # the partners of a pair in different numbers
    assert len(set(distinct)) == len(distinct)
    seqs = R.with_multiplicities(distinct, mult, rng)
    path = str(tmp_path_factory.mktemp("collapse_in") / "reads.txt")
    with open(path, "w") as f:
        f.write("\n".join(seqs) + "\n")
    return seqs, path


def _rep_of(exe, bits, path):
    out = subprocess.run([exe, str(bits), path], check=True, timeout=120, stdout=subprocess.PIPE, text=True).stdout.split()
    return [int(v) for v in out]


def test_the_header_needs_no_hip():
    """every header reachable from ps_collapse.h is a system header without `hip` in its name or a project header of which the same holds"""
    seen, todo = set(), ["ps_collapse.h"]
    while todo:
        h = todo.pop()
        if h in seen:
            continue
        seen.add(h)
        for inc in re.findall(r"^\s*#\s*include\s+(\S+)", open(os.path.join(CSRC, h)).read(), re.M):
            assert "hip" not in inc.lower(), (h, inc)
            if inc.startswith('"'):
                todo.append(inc.strip('"'))
    assert {"ps_collapse.h", "ps_types.h"} <= seen


def test_full_key_groups_equal_the_dict(exe, reads):
    seqs, path = reads
    want = R.groups_of(seqs)
    assert sorted(len(v) for v in want.values())[-len(GROUP_SIZES):][-2:] == [256, 257]
    rep_of = _rep_of(exe, 64, path)
    assert len(rep_of) == len(seqs)
    R.check_groups_exact(seqs, rep_of)
    assert R.partition(rep_of) == {tuple(v) for v in want.values()}
    # a stable sort of (key, index): a group's representative is its first copy
    assert all(rep_of[i] == want[(len(s), s)][0] for i, s in enumerate(seqs))


def test_four_key_bits_groups_stay_exact(exe, reads):
    """16 keys for 39 different reads: colliding keys are the rule, and only the comparison in full separates them"""
    seqs, path = reads
    want = R.groups_of(seqs)
    rep_of = _rep_of(exe, 4, path)
    assert len(rep_of) == len(seqs)
    R.check_groups_exact(seqs, rep_of)
    assert len(R.partition(rep_of)) >= len(want)


def test_the_adversarial_pairs_are_kept_apart(exe, tmp_path):
    """alone, without copies: no two of them share a group, whatever the key width"""
    adv = R.adversarial_reads(np.random.default_rng(7))
    path = str(tmp_path / "adv.txt")
    with open(path, "w") as f:
        f.write("\n".join(adv) + "\n")
    for bits in (64, 4, 1):
        assert _rep_of(exe, bits, path) == list(range(len(adv))), bits
