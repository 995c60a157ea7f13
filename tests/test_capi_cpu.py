"""CPU tier: the C-ABI library loads, exports every symbol include/parasuite_hip.h declares, binds each with the header's
signature, mirrors every struct of the header field for field, and fails loudly (no CPU fallback) when asked to compute
without a HIP device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "parasuite_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ps_[a-z0-9_]+)\s*\(", text)))


def test_exports_match_header():
    import capi
    lib = capi.lib()
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), n
    assert sorted(capi.EXPORTS) == names
    assert lib.ps_version().startswith(b"parasuite-hip")


def _header():
    text = open(os.path.join(ROOT, "include", "parasuite_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _mirror_layout(mirror):
    """(size, {field: (offset, size)}) of a ctypes.Structure mirror or a numpy record dtype"""
    if isinstance(mirror, np.dtype):
        return mirror.itemsize, {f: (off, dt.itemsize) for f, (dt, off) in mirror.fields.items()}
    return C.sizeof(mirror), {f: (getattr(mirror, f).offset, getattr(mirror, f).size) for f, _ in mirror._fields_}


def _header_layouts(tmp_path, structs):
    """the same from the header: a C program generated from the mapping, built with $CC -I include"""
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "parasuite_hip.h"', 'int main(void) {']
    for name, mirror in structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f in _mirror_layout(mirror)[1]:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (name, f, name, f, name, f))
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / "layouts.c", str(tmp_path / "layouts")
    src.write_text("\n".join(lines))
    subprocess.check_call([os.environ.get("CC", "cc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    out = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        key, *nums = line.split()
        name, _, field = key.partition(".")
        if field:
            out[name][1][field] = tuple(int(x) for x in nums)
        else:
            out[name] = (int(nums[0]), {})
    return out


def test_every_struct_matches_the_header(tmp_path):
    """every struct typedef of the header has a mirror in capi.STRUCTS with the header's size and, field by field, its offsets and
    member sizes; the numbers that pin the ABI itself are asserted as numbers"""
    import capi
    declared = re.findall(r"typedef\s+struct\s*\{[^{}]*\}\s*(ps_\w+)\s*;", _header())
    assert len(declared) == len(set(declared)) >= 21 and sorted(capi.STRUCTS) == sorted(declared)
    want = _header_layouts(tmp_path, capi.STRUCTS)
    for name, mirror in capi.STRUCTS.items():
        assert _mirror_layout(mirror) == want[name], name

    class SwappedKStats(C.Structure):                     # negative control: two fields of one mirror swapped
        _fields_ = [capi.KStats._fields_[1], capi.KStats._fields_[0]] + capi.KStats._fields_[2:]
    assert C.sizeof(SwappedKStats) == want["ps_kstats"][0] and _mirror_layout(SwappedKStats) != want["ps_kstats"]

    size = {name: _mirror_layout(m)[0] for name, m in capi.STRUCTS.items()}
    assert size["ps_aln"] == capi.ALN_DTYPE.itemsize == 32 and size["ps_hit"] == capi.HIT_DTYPE.itemsize == 128
    assert size["ps_index_info"] == 8 * 11 + 4 * 4 + 8 + 4 * 2 and size["ps_kstats"] == 64
    assert size["ps_route_opts"] == 8 * 8 + 5 * 4 + 4 and size["ps_route_stats"] == 8 + 3 * 24 + 32 + 13 * 8 + 9 * 8 + 4 * 4
    R = capi.RouteOpts2
    assert (size["ps_route_opts2"], R.reads_fq.offset, R.ref_refine.offset) == (112, 24, 88)
    assert capi.ROUTE_OPTS_OLD_SIZE == 88 and R.struct_size.offset == 0
    assert size["ps_resident_opts"] == 8 and size["ps_resident_stats"] == 8 + 7 * 8
    assert size["ps_fetch_stats"] == C.sizeof(capi.FetchStats) == 8 * 15


_C_CLASS = {"int": "i32", "int32_t": "i32", "uint32_t": "i32", "int64_t": "i64", "uint64_t": "i64", "double": "double", "void": "void"}
_CTYPES_CLASS = {"i": "i32", "I": "i32", "l": "i64", "L": "i64", "q": "i64", "Q": "i64", "d": "double", "z": "pointer", "P": "pointer"}


def _c_class(decl):
    """a return type or one parameter of a prototype -> pointer, i32, i64, double or void"""
    if "*" in decl or "[" in decl:
        return "pointer"
    return _C_CLASS[[w for w in decl.split() if w != "const"][0]]


def _ctypes_class(t):
    if t is None:
        return "void"
    if issubclass(t, C._Pointer):
        return "pointer"
    assert C.sizeof(t) == {"i32": 4, "i64": 8, "double": 8, "pointer": 8}[_CTYPES_CLASS[t._type_]], t
    return _CTYPES_CLASS[t._type_]


def _prototypes():
    """{function: (return class, [parameter classes])} of every prototype of the header"""
    out = {}
    for ret, name, params in re.findall(r"([\w \*]+?)\b(ps_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in out, name
        params = [p.strip() for p in params.split(",")]
        out[name] = (_c_class(ret), [] if params == ["void"] else [_c_class(p) for p in params])
    return out


def _signature_mismatches(table, protos):
    return sorted(n for n in set(table) | set(protos) if n not in table or n not in protos or
                  (_ctypes_class(table[n][0]), [_ctypes_class(a) for a in table[n][1]]) != protos[n])


def test_signatures_match_header():
    """capi.SIGNATURES declares every function of the header with the header's return and parameter classes, and lib() has
    applied it to every function before any wrapper runs"""
    import capi
    protos = _prototypes()
    assert sorted(protos) == sorted(capi.SIGNATURES) == _declared() and len(protos) >= 65
    assert protos["ps_parse_check"] == ("i32", ["pointer", "i32", "i64", "pointer"]) and protos["ps_ctx_clone"] == ("pointer", ["pointer", "i32"])
    assert protos["ps_release_host_cache"] == ("void", []) and protos["ps_ctx_set_profile_matrix"][1] == ["pointer", "pointer", "double", "double", "i32"]
    assert _signature_mismatches(capi.SIGNATURES, protos) == []
    restype, argtypes = capi.SIGNATURES["ps_parse_check"]             # negative control: a uint64_t parameter declared as a C int
    wrong = dict(capi.SIGNATURES, ps_parse_check=(restype, [argtypes[0], argtypes[1], C.c_int, argtypes[3]]))
    assert _signature_mismatches(wrong, protos) == ["ps_parse_check"]
    lib = capi.lib()
    for name, (restype, argtypes) in capi.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes) and fn.restype is restype, name
    assert lib.ps_ctx_clone.restype is C.c_void_p and lib.ps_batch_from_codes.restype is C.c_void_p and lib.ps_ctx_close.restype is None


def _no_gpu():
    try:
        import torch
        return not torch.cuda.is_available()
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_compute_fails_loudly_without_device(example, workdir):
    import capi
    with pytest.raises(capi.PsError, match="no HIP device"):
        capi.Ctx.build(example["fa"])
    with pytest.raises(capi.PsError):
        capi.ps_index(example["fa"])
    with pytest.raises(capi.PsError):
        capi.ps_map(1, "2", None, None, example["fa"], os.path.join(workdir, "x.fq"), os.path.join(workdir, "x.sam"))


@pytest.mark.skipif(not _no_gpu(), reason="checks the no-device behaviour")
def test_mapping_mirror_error_contract(example, workdir):
    """non-zero status from the library surfaces as ExternalCallErrorException carrying the command
    (Mapping.java:170-172,189-197)"""
    import __graft_entry__ as ge
    mod = ge.load_package()
    m = mod.mapping.PARAsuiteMapping()
    m.setErrorProfileFilename(os.path.join(workdir, "none.errorprofile"))
    m.setIndelProfileFilename(os.path.join(workdir, "none.indelprofile"))
    with pytest.raises(mod.mapping.ExternalCallErrorException) as ei:
        m.executeMapping(4, example["fa"], os.path.join(workdir, "x.fq"), os.path.join(workdir, "out"), 10, "-1")
    assert "bwa" in ei.value.getMappingCommand()


def test_mapq_filter_on_sam(tmp_path):
    import __graft_entry__ as ge
    mod = ge.load_package()
    src = tmp_path / "a.sam"
    src.write_text("@SQ\tSN:c\tLN:10\nr1\t0\tc\t1\t37\t5M\t*\t0\t0\tACGTA\tIIIII\nr2\t0\tc\t2\t0\t5M\t*\t0\t0\tACGTA\tIIIII\n"
                   "r3\t4\t*\t0\t0\t*\t*\t0\t0\tACGTA\tIIIII\n")
    mod.mapping.Mapping.filter_sam_mapq(str(src), str(tmp_path / "b.sam"), 10)
    assert [l.split("\t")[0] for l in open(tmp_path / "b.sam")] == ["@SQ", "r1"]
