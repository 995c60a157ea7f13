#!/usr/bin/env python3
"""Generates bam_writer_streams.json: what the files of tests/bamsink_check.cpp inflate to (tests/bam_writer_streams.py).  It was run
once, at the commit before the writer's host side was folded into one body hand-over and one block cutter, and pins every writer of
ps_bam.cpp to the bytes of that commit; run it again only when a change is meant to alter a file.
Run from the repo root:  python tests/golden/make_bam_writer_golden.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bam_writer_streams as W  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out, _ = W.build_and_run(tmp)
        d = W.digest(out)
    with open(W.GOLDEN, "w") as f:
        json.dump(d, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%s: %d files" % (W.GOLDEN, len(d)))


if __name__ == "__main__":
    main()
