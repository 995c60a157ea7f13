"""The stage kernels that run beside the other batch's search launch (ps_budget.h, ps_stage.hip), through the C ABI:
  - two batches on two lanes, driven the way bench.py drives them (the search of one while the other is in selection and
    locate), several rounds: every round's records equal the batch run alone;
  - the hand-out order's counting sort: a stable ascending sort of the 8-bit keys (numpy's stable argsort is the reference);
  - the tie-break offsets from per-group counts + ballot ranks: ragged lengths, N not a multiple of 64, unmapped / unique /
    repeat reads all present, SAM (which fixes every draw) against the oracle;
  - k_refine with its H/E rows in global scratch: indels next to either end of the read, both strands, against the oracle."""
import os
import re
import threading

import numpy as np
import pytest

from conftest import sam_records
from test_gpu_parity import _compare, _fastq

pytestmark = pytest.mark.gpu


def _profile():
    import simulate as S
    P = S.EXAMPLE_PROFILE.copy()
    P[3, 1], P[3, 3] = 0.12, 0.87
    return P


def test_two_batches_in_flight_equal_each_alone(example, workdir):
    """two lanes used at the same time: races between the streams, the lanes' workspaces, the deferred stage timers.  It does NOT
    cover the stage budget: a 6,000-read search launch leaves most CUs empty, so nothing here has to fit beside a resident launch.
    That the stage kernels do is shown by tests/test_stage_budget_cpu.py (resources) and the committed kernel traces
    (profiles/r04_timeline_*)."""
    import capi
    ctx = capi.Ctx.build(example["fa"])
    try:
        ctx.set_profile(_profile(), 2.1e-5, 5.9e-4, -1)
        ctx.set_lanes(2)
        fqs = [_fastq(example["genome"], workdir, "ovl%d" % j, n_reads=6000 + 37 * j, read_len=50, seed=31 + j, indel_scale=30, n_frac=0.002)
               for j in range(2)]
        batches = [ctx.batch_from_fastq(fq) for fq in fqs]
        alone = []
        for b in batches:                        # each batch alone: all four stages, nothing else on the device
            b.run(4)
            alone.append((b.hits().copy(), b.n_aln().copy()))
            assert int((alone[-1][0]["type"] != 0).sum()) > 1000
        rounds, n_steps = 4, 8
        searched = [threading.Event() for _ in range(n_steps)]
        chosen = [threading.Event() for _ in range(n_steps)]
        err, got = [], [None] * n_steps

        def lane(k):
            b = batches[k % 2]
            try:
                b.search()
                searched[k].set()
                chosen[k].wait()
                if err:
                    return
                b.select_easy(4)
                b.locate()
                got[k] = (b.hits().copy(), b.n_aln().copy())
            except Exception as e:               # noqa: BLE001
                err.append(e)
                searched[k].set()

        th = [threading.Thread(target=lane, args=(k,)) for k in range(n_steps)]
        started = 0
        for k in range(n_steps):
            while started < min(n_steps, k + 2):     # step k + 1 (the other batch) searches while step k selects and locates
                if started >= 2:
                    th[started - 2].join()           # its batch is free when that batch's previous step is through
                th[started].start(); started += 1
            searched[k].wait()
            if not err:
                batches[k % 2].select_hard(0)
            chosen[k].set()
        for t in th:
            t.join()
        assert not err, err
        assert n_steps == 2 * rounds
        for k in range(n_steps):
            hits, n_aln = got[k]
            assert np.array_equal(n_aln, alone[k % 2][1]), k
            assert hits.tobytes() == alone[k % 2][0].tobytes(), k
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096, 4097, 300001, 9000017])
def test_order_sort_is_a_stable_sort(example, n):
    import capi
    ctx = capi.Ctx.build(example["fa"])
    try:
        rng = np.random.default_rng(n)
        cases = [rng.integers(0, 256, n).astype(np.uint8),                    # every bin
                 np.full(n, 200, dtype=np.uint8),                              # one bin
                 (255 - np.minimum(255, rng.geometric(0.08, n))).astype(np.uint8),   # a few heavy classes, as the effort keys are
                 (np.arange(n) % 256).astype(np.uint8)[::-1].copy()]           # 64 distinct keys in every tile
        for keys in cases:
            order = ctx.order_sort(keys)
            assert np.array_equal(order, np.argsort(keys, kind="stable").astype(np.int32))
    finally:
        ctx.close()


def test_group_offsets_ragged_three_classes(multi, workdir):
    import capi
    import orc
    import simulate as S
    from test_gpu_option_edges import repeat_genome
    P = _profile()
    g = list(multi["genome"]) + [("rep", repeat_genome()[0][1])]     # contig edges, N runs -- and diverged repeat copies: several best-score intervals
    fa = os.path.join(workdir, "grp_ragged.fa")
    S.write_fasta(fa, g)
    n = 64 * 57 + 29                                            # not a multiple of 64
    sim = S.simulate_reads(g, n, 75, seed=41, indel_scale=40, n_frac=0.003, min_len=36)
    rng = np.random.default_rng(5)
    junk = rng.random(n) < 0.1                                  # reads from nowhere: class 0, scattered through the input
    sim["codes"][junk] = np.where(sim["codes"][junk] != 255, rng.integers(0, 4, sim["codes"][junk].shape).astype(np.uint8), 255)
    fq = os.path.join(workdir, "grp_ragged.fq")
    S.write_fastq(fq, sim)
    oix = orc.Index.from_fasta(fa)
    ctx = capi.Ctx.build(fa)
    try:
        for tag, setter, opt in (("grp_prof", lambda: ctx.set_profile(P, 2.1e-5, 5.9e-4, -1), orc.profile_opt(P, 2.1e-5, 5.9e-4, -1)),
                                 ("grp_stock", lambda: ctx.set_stock("0.04"), orc.stock_opt("0.04"))):
            setter()
            _compare(ctx, oix, opt, fq, workdir, tag)
            sai = orc.read_sai(os.path.join(workdir, tag + ".orc.sai"))      # the reference's own hit lists show what was tested
            assert len(sai) == n and n % 64 != 0
            c0 = sum(1 for x in sai if len(x) == 0)
            c2 = sum(1 for x in sai if len(x) >= 2 and int(x[1]["score"]) == int(x[0]["score"]))
            c1 = n - c0 - c2
            print(tag, "no hit", c0, "one best-score interval", c1, "several", c2)
            assert c0 >= 50 and c1 >= 500 and c2 >= 50
    finally:
        ctx.close()


def test_refine_gaps_next_to_both_read_ends(example, workdir):
    import capi
    import orc
    import simulate as S
    name, asc = example["genome"][0]
    codes = S.contig_codes(asc)
    rng = np.random.default_rng(77)
    L, comp = 50, np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    lut = np.frombuffer(b"ACGTN", dtype=np.uint8)
    lines = []
    near = [6, 7, 8, 9, L - 10, L - 9, L - 8, L - 7]            # indels may open 5 bases from an end (indel_end_skip)
    n = 0
    while n < 1600:
        s = int(rng.integers(1000, codes.size - 1000))
        win = codes[s:s + L + 2]
        if (win > 3).any():
            continue
        p = near[n % len(near)]
        if (n // len(near)) % 2 == 0:
            read = np.concatenate([win[:p], win[p + 1:L + 1]])                 # one reference base missing: a deletion
        else:
            read = np.concatenate([win[:p], [(win[p] + 1 + rng.integers(0, 3)) % 4], win[p:L - 1]]).astype(np.uint8)   # an inserted base
        if (n // (2 * len(near))) % 2:
            read = comp[read[::-1]]
        lines.append(b"@g%d\n" % n + lut[read].tobytes() + b"\n+\n" + b"I" * L + b"\n")
        n += 1
    fq = os.path.join(workdir, "gap_ends.fq")
    with open(fq, "wb") as f:
        f.write(b"".join(lines))
    ctx = capi.Ctx.build(example["fa"])
    try:
        ctx.set_stock("0.04")
        _compare(ctx, example["orc_index"], orc.stock_opt("0.04"), fq, workdir, "gap_ends")
        head = tail = 0
        for l in sam_records(os.path.join(workdir, "gap_ends.orc.sam")):
            ops = re.findall(r"(\d+)([MIDS])", l.split("\t")[5])
            if any(o in "ID" for _, o in ops):
                head += int(ops[0][0]) <= 10 and ops[1][1] in "ID"
                tail += int(ops[-1][0]) <= 10 and ops[-2][1] in "ID"
        print("oracle: gapped hits with the gap within 10 bases of the read's start", head, "of its end", tail)
        assert head >= 100 and tail >= 100
    finally:
        ctx.close()
