"""CPU tier: the kernels of the collapsed search (para-suite_amd/csrc/ps_collapse.hip) fit beside a resident first-tier search
launch, by the method of tests/test_stage_budget_cpu.py: the device code is compiled for gfx950 with
-Rpass-analysis=kernel-resource-usage and every kernel is held to ps_budget.h -- at most PS_STAGE_VGPRS registers, no LDS,
nothing spilled, no scratch.  The LSD passes of the sort are the hand-out order's counting sort, which that test holds."""
import os
import re
import subprocess

from test_stage_budget_cpu import CSRC, HIPCC, STAGE_KERNELS, _header_constants

UNIT = "ps_collapse.hip"
COLLAPSE_KERNELS = {
    "15k_collapse_keysE": "keys", "15k_collapse_stepE": "between two sort passes", "16k_collapse_headsE": "heads", "15k_collapse_repsE": "representative of every read",
    "16k_collapse_countE": "representatives per chunk", "18k_collapse_compactE": "representatives in bin order", "17k_collapse_gatherE": "gather",
    "17k_collapse_expandE": "expand",
}


def _remarks():
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", UNIT, "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return usage


def test_collapse_kernels_fit_beside_a_search_launch(tmp_path):
    usage = _remarks()
    budget = _header_constants(tmp_path)["stage_vgprs"]
    assert budget == 64
    src = open(os.path.join(CSRC, UNIT)).read()
    declared = re.findall(r"__global__[^{;]*?\b(k_\w+)\(", src)
    assert "__shared__" not in src
    # every kernel of the unit is in the table, and none of their names is taken for one of the stage test's kernels
    assert sorted("%d%sE" % (len(k), k) for k in declared) == sorted(COLLAPSE_KERNELS)
    assert not [(f, k) for f in STAGE_KERNELS for k in COLLAPSE_KERNELS if f in k]
    for frag, what in COLLAPSE_KERNELS.items():
        hit = [(k, v) for k, v in usage.items() if frag in k]
        assert len(hit) == 1, (frag, what, sorted(usage))
        u = hit[0][1]
        print("%-34s %3d VGPRs, %5d B LDS, %d spilled, %d B scratch" % (what, u["VGPRs"], u["LDS Size [bytes/block]"], u["VGPRs Spill"], u["ScratchSize [bytes/lane]"]))
        assert u["VGPRs"] <= budget, (what, u)
        assert u["LDS Size [bytes/block]"] == 0, (what, u)
        assert u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (what, u)
