"""CPU tier: the stage kernels fit beside a resident first-tier search launch (para-suite_amd/csrc/ps_budget.h).

The device code is compiled for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU needed) and the remark is held
against the budget: VGPRs <= 512 - 4 x (the search kernel's allocation), static + dynamic LDS <= 163,840 - 4 x 256 x
lm_bytes(50, 32, 25), no register spilled.  The header's constants are held against the same compile and against lm_bytes().
No stage kernel can use dynamic LDS any more (no `extern __shared__` outside the search kernels: asserted on the source text),
so the static figure of the remark is the whole request."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "para-suite_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ["ps_kernels.hip", "ps_effort.hip", "ps_stage.hip", "ps_search.hip", "ps_samse.hip"]

# every kernel the two in-flight batches run between their search launches: mangled-name fragment -> what it is
STAGE_KERNELS = {
    "7k_widthE": "width stage", "8k_effortE": "effort scans", "14k_effort_modelILi16E": "effort model, 16 lanes per read",
    "14k_effort_modelILi32E": "effort model, 32 lanes per read", "14k_effort_modelILi64E": "effort model, 64 lanes per read",
    "12k_order_keysE": "order keys (PS_ORDER=2)", "11k_sort_histE": "order sort: counts", "11k_sort_scanE": "order sort: offsets",
    "14k_sort_scatterE": "order sort: placement", "10k_classifyE": "classes", "12k_gather_subE": "host subset's hit lists",
    "13k_class_ranksE": "tie-break offsets", "8k_selectE": "selection", "8k_sa2posE": "SA walk", "6k_postE": "strand / MAPQ",
    "8k_refineE": "banded DP",
}
SEARCH_KERNEL = "13k_backtrack_nILb0ELb1EE"       # the timed first-tier kernel: no counters, one-word bucket bitmap
GONE = ["k_class_flags", "k_iota"]               # passes this budget removed


def _remarks():
    usage = {}
    for u in UNITS:
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--cuda-device-only", "-c", u, "-o", os.devnull,
                            "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        cur = None
        for line in r.stderr.splitlines():
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = usage.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+(VGPRs|VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and cur is not None:
                cur[m.group(1)] = int(m.group(2))
    return usage


def _header_constants(tmp_path):
    src = tmp_path / "budget.cpp"
    src.write_text('#include <cstdio>\n#include "ps_core.h"\n#include "ps_budget.h"\n'
                   'int main() { using namespace ps; std::printf("%d %d %d %d %zu %zu %zu %d\\n", PS_SIMD_VGPRS, PS_SEARCH_WAVES, PS_SEARCH_VGPRS, '
                   'PS_STAGE_VGPRS, PS_CU_LDS, PS_SEARCH_LDS_PER_LANE, PS_STAGE_LDS, lm_bytes(50, 32, 25, false)); }\n')
    exe = tmp_path / "budget"
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", "-I", CSRC, "-o", str(exe), str(src)])
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    return dict(zip(["simd", "waves", "search_vgprs", "stage_vgprs", "cu_lds", "lds_per_lane", "stage_lds", "lm_bytes"], v))


def test_stage_kernels_fit_beside_a_search_launch(tmp_path):
    usage = _remarks()
    hc = _header_constants(tmp_path)
    search = [v for k, v in usage.items() if SEARCH_KERNEL in k]
    assert len(search) == 1, sorted(usage)
    alloc = (search[0]["VGPRs"] + 7) // 8 * 8                   # gfx950 allocates VGPRs in units of 8
    free_vgprs = 512 - 4 * alloc
    free_lds = 163840 - 4 * 256 * hc["lm_bytes"]
    # the header's numbers are these
    assert (hc["simd"], hc["waves"], hc["cu_lds"]) == (512, 4, 163840)
    assert hc["search_vgprs"] == alloc and hc["stage_vgprs"] == free_vgprs
    assert hc["lds_per_lane"] == hc["lm_bytes"] and hc["stage_lds"] == free_lds
    assert free_vgprs > 0 and free_lds >= 0
    # dynamic LDS can only be used through an `extern __shared__` array: none but the search kernels declares one
    for u in UNITS:
        src = open(os.path.join(CSRC, u)).read()
        for m in re.finditer(r"__global__[^{;]*?\b(k_\w+)\(", src):
            if "extern __shared__" in src[m.end():src.find("\n}\n", m.end())]:
                assert m.group(1).startswith("k_backtrack"), m.group(1)
    for frag, what in STAGE_KERNELS.items():
        hit = [(k, v) for k, v in usage.items() if frag in k and "rocprim" not in k]
        assert len(hit) == 1, (frag, what, [k for k, _ in hit])
        name, u = hit[0]
        lds = u["LDS Size [bytes/block]"]
        print("%-34s %3d VGPRs, %5d B LDS, %d spilled, %d B scratch" % (what, u["VGPRs"], lds, u["VGPRs Spill"], u["ScratchSize [bytes/lane]"]))
        assert u["VGPRs"] <= free_vgprs, (what, u)
        assert lds <= free_lds, (what, u)
        assert lds == 0, (what, u)             # a workgroup's LDS may be rounded up to a coarser unit: the 4 KB on paper are not relied on
        assert u["VGPRs Spill"] == 0 and u["ScratchSize [bytes/lane]"] == 0, (what, u)
    for k in usage:
        assert not any(g in k for g in GONE), k
